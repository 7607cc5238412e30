// sc_own.h -- who frees what on the host side of spacecarve.hip (included there, ahead of sc_engine.h).  Host code only.
// One move-only owner of a handle and the function that gives it back, and the one way a buffer grows behind the
// stream.  The free function is a template parameter: the engine's aliases name the runtime's, tools/own_rehearsal.cpp
// a fake that counts.
#ifndef SC_OWN_H
#define SC_OWN_H

#include <hip/hip_runtime.h>

#include <cstddef>
#include <utility>

namespace scown {

template <class H, auto Free>
class Own {
    H h_{};

public:
    Own() = default;
    explicit Own(H h) : h_(h) {}
    Own(Own &&o) noexcept : h_(o.release()) {}
    Own &operator=(Own &&o) noexcept {
        if (this != &o) reset(o.release());
        return *this;
    }
    ~Own() { reset(); }
    H get() const { return h_; }
    operator H() const { return h_; }  // launches, copies and pointer arithmetic read as with the bare handle
    explicit operator bool() const { return h_ != H{}; }
    H release() { return std::exchange(h_, H{}); }
    void reset(H h = H{}) {
        if (h_ != H{}) (void)Free(h_);
        h_ = h;
    }
    H *out() {  // where an allocating call puts a new handle (what was held goes first)
        reset();
        return &h_;
    }
};

// `need` > `cap`: wait() until nothing on the device uses the old blocks, give them back in the order named, alloc()
// new ones into the same owners, and only then set the capacity.  A failure leaves every owner empty and `cap` 0.
// Returns what wait() / alloc() return, whose zero value is success.
template <class Wait, class Alloc, class... Owner>
auto grow(size_t &cap, size_t need, Wait &&wait, Alloc &&alloc, Owner &...own) -> decltype(wait()) {
    using R = decltype(wait());
    if (need <= cap) return R{};
    if (R r = wait(); r != R{}) return r;
    (own.reset(), ...);
    cap = 0;
    if (R r = alloc(); r != R{}) {
        (own.reset(), ...);
        return r;
    }
    cap = need;
    return R{};
}

}  // namespace scown

template <class T>
using DevPtr = scown::Own<T *, hipFree>;
template <class T>
using PinPtr = scown::Own<T *, hipHostFree>;
using Event = scown::Own<hipEvent_t, hipEventDestroy>;

#endif
