// own_rehearsal.cpp -- csrc/sc_own.h on the CPU: the owner with a free function that counts its calls and keeps the
// handles it was given, and scown::grow with allocators that fail.  Host code only: no kernel runs, no device.
//   hipcc -x hip --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined \
//       -I plant-3d-vision_amd/csrc tools/own_rehearsal.cpp -o build/own_rehearsal && build/own_rehearsal
#include "sc_own.h"

#include <cstdio>
#include <cstdlib>
#include <vector>

static std::vector<int *> g_freed;
static int fake_free(int *p) {
    g_freed.push_back(p);
    free(p);  // (ASan: a handle freed twice, or never, is reported)
    return 0;
}
using Ptr = scown::Own<int *, fake_free>;

static int g_fail = 0, g_checks = 0;
static void expect(bool ok, const char *what) {
    ++g_checks;
    if (ok) return;
    printf("FAILED: %s\n", what);
    ++g_fail;
}
static int *fresh() { return static_cast<int *>(malloc(sizeof(int))); }
static bool freed_are(std::initializer_list<int *> want) { return g_freed == std::vector<int *>(want); }

int main() {
    {  // destruction frees exactly once; an empty owner frees nothing
        int *p = fresh();
        {
            Ptr a(p), none;
            expect(a && a.get() == p && !none && none.get() == nullptr, "what an owner holds");
            int *raw = a;  // the conversion call sites rely on
            expect(raw == p && g_freed.empty(), "conversion to the handle");
        }
        expect(freed_are({p}), "destruction frees once");
    }
    g_freed.clear();
    {  // reset() twice frees once; reset(h) takes a new handle
        int *p = fresh(), *q = fresh();
        Ptr a(p);
        a.reset();
        a.reset();
        expect(freed_are({p}) && !a, "reset twice frees once");
        a.reset(q);
        expect(freed_are({p}) && a.get() == q, "reset to a new handle");
        *a.out() = nullptr;  // out(): what was held goes first
        expect(freed_are({p, q}) && !a, "out() frees what was held");
    }
    expect(g_freed.size() == 2, "an emptied owner's destruction frees nothing");
    g_freed.clear();
    {  // release() hands the handle over without freeing it
        int *p = fresh();
        {
            Ptr a(p);
            expect(a.release() == p && !a, "release hands over");
        }
        expect(g_freed.empty(), "release does not free");
        free(p);
    }
    {  // moves
        int *p = fresh(), *q = fresh();
        {
            Ptr a(p);
            Ptr b(std::move(a));
            expect(!a && b.get() == p && g_freed.empty(), "move construction transfers");
            Ptr c(q);
            c = std::move(b);
            expect(!b && c.get() == p && freed_are({q}), "assignment over a live handle frees the old one once");
            Ptr &self = c;
            c = std::move(self);
            expect(c.get() == p && freed_are({q}), "self-move is harmless");
        }
        expect(freed_are({q, p}), "the moved-to owner frees at its end");
    }
    g_freed.clear();
    {  // a vector of owners that reallocates frees nothing until it is destroyed
        std::vector<int *> made;
        {
            std::vector<Ptr> v;
            for (int i = 0; i < 100; ++i) {
                made.push_back(fresh());
                v.push_back(Ptr(made.back()));
            }
            expect(g_freed.empty(), "a growing vector frees nothing");
            Ptr last = std::move(v.back());
            v.pop_back();
            expect(g_freed.empty() && last.get() == made.back(), "taking one out of the vector");
        }
        expect(g_freed.size() == made.size(), "the vector's end frees every handle once");
    }
    g_freed.clear();
    {  // grow
        Ptr a, b;
        size_t cap = 0;
        int waits = 0;
        auto wait = [&] { ++waits; return 0; };
        auto both = [&] { *a.out() = fresh(); *b.out() = fresh(); return 0; };
        expect(scown::grow(cap, 8, wait, both, a, b) == 0 && cap == 8 && a && b && waits == 1 && g_freed.empty(), "grow from nothing");
        int *a0 = a, *b0 = b;
        expect(scown::grow(cap, 8, wait, both, a, b) == 0 && a.get() == a0 && waits == 1 && g_freed.empty(), "enough capacity: nothing happens");
        expect(scown::grow(cap, 9, wait, both, a, b) == 0 && cap == 9 && waits == 2 && freed_are({a0, b0}), "grow frees the old blocks in order, once");
        g_freed.clear();
        int *a1 = a, *b1 = b;
        // a wait that fails: nothing is touched
        expect(scown::grow(cap, 10, [] { return 7; }, both, a, b) == 7 && cap == 9 && a.get() == a1 && g_freed.empty(), "a failed wait leaves everything");
        // an allocator that fails at once: empty and consistent, no second free
        expect(scown::grow(cap, 10, wait, [] { return 2; }, a, b) == 2 && cap == 0 && !a && !b && freed_are({a1, b1}), "a failing allocator leaves owners and capacity empty");
        // ... and one that fails half way: what it had allocated goes back
        int *half = nullptr;
        auto halfway = [&] { *a.out() = half = fresh(); return 2; };
        expect(scown::grow(cap, 10, wait, halfway, a, b) == 2 && cap == 0 && !a && !b && freed_are({a1, b1, half}), "an allocator failing half way");
        expect(scown::grow(cap, 4, wait, both, a, b) == 0 && cap == 4 && a && b && g_freed.size() == 3, "grow again after a failure");
    }
    expect(g_freed.size() == 5, "the grown blocks go with their owners");
    if (g_fail) printf("FAILED: %d of %d\n", g_fail, g_checks);
    else printf("ok: %d checks\n", g_checks);
    return g_fail ? 1 : 0;
}
