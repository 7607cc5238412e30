// sc_unit.h -- the host scaffold of the stand-alone device units (vol2pcd, label_points, masks_rgb, dbscan, evaluate, class_select, nearest, undistort, graph): the
// "last error" of a unit, the layout of a work buffer, the per-device work-buffer slot of DESIGN.md 12 and the scope
// of one call on it.  (Device text that units share: sc_quads.h, sc_bitplane.h, sc_points.h, sc_unionfind.h.)
// Host only, internal linkage: every unit that includes it has its own copy and its own state.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <mutex>

#include "spacecarve.h"

namespace {

constexpr int kUnitDevices = 64;  // device ordinals a unit keeps state for

// A unit declares `thread_local UnitError g_err;` and returns g_err.msg from its sc_*_last_error.
struct UnitError {
    char msg[256];
    int fail(int code, const char *text) {
        strncpy(msg, text, sizeof msg - 1);
        msg[sizeof msg - 1] = 0;
        return code;
    }
    int hip(hipError_t e) { return fail(e == hipErrorOutOfMemory ? SC_ERR_NOMEM : SC_ERR_DEVICE, hipGetErrorString(e)); }
};

// For functions with `int rc` and a `done:` label that cleans up.
#define UNIT_TRY(expr)                                          \
    do {                                                        \
        hipError_t _e = (expr);                                 \
        if (_e != hipSuccess) { rc = g_err.hip(_e); goto done; } \
    } while (0)

size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// Buffers one after the other in one allocation, each on a 256-byte boundary: take() gives the next buffer's offset,
// `total` is what to allocate.  The offsets and the total come from the same statements.
struct Layout {
    size_t total = 0;
    size_t take(size_t bytes) {
        const size_t at = total;
        total += al256(bytes);
        return at;
    }
};

// Remembers the caller's current device and puts it back when the scope ends: no runtime call then where the scope
// only ever went to `going`, the caller's own device.
struct CallerDevice {
    int was = -1;
    const int going;
    explicit CallerDevice(int going_to = -1) : going(going_to) { if (hipGetDevice(&was) != hipSuccess) was = -1; }
    ~CallerDevice() { if (was >= 0 && was != going) (void)hipSetDevice(was); }
};

// f(d) for every device ordinal; the caller's current device stays what it was.
template <class F>
void on_each_device(F f) {
    CallerDevice keep;
    for (int d = 0; d < kUnitDevices; ++d) f(d);
}

// The work buffers a unit keeps per device; they grow as needed.  Calls are serialised by `mu` while they ENQUEUE; a
// call waits (on the device, through `last`) for the previous call's work before it touches the buffers, so calls on
// different streams of one device never overlap in them.  An entry point judges its arguments, then opens a UnitCall
// (below), which fixes the order of the rest.
struct WorkSlot {
    std::mutex mu;
    char *base = nullptr;
    size_t cap = 0;
    hipEvent_t last = nullptr;  // recorded behind the latest call's work
    bool checked = false;       // the device is a gfx950

    int first_use(UnitError &err, int device, hipStream_t stream) {
        if (checked) return SC_OK;
        hipDeviceProp_t prop;
        hipError_t e = hipGetDeviceProperties(&prop, device);
        if (e != hipSuccess) return err.hip(e);
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            char text[200];
            snprintf(text, sizeof text, "device %d is %s; this library is built for gfx950 only", device, prop.gcnArchName);
            return err.fail(SC_ERR_DEVICE, text);
        }
        if ((e = hipEventCreateWithFlags(&last, hipEventDisableTiming)) != hipSuccess) return err.hip(e);
        if ((e = hipEventRecord(last, stream)) != hipSuccess) return err.hip(e);
        checked = true;
        return SC_OK;
    }

    int grow(UnitError &err, size_t need) {
        if (cap >= need) return SC_OK;
        hipError_t e = hipEventSynchronize(last);  // nobody reads the old buffers any more
        if (e != hipSuccess) return err.hip(e);
        if (base) (void)hipFree(base);
        base = nullptr;
        cap = 0;
        if ((e = hipMalloc(reinterpret_cast<void **>(&base), need)) != hipSuccess) return err.hip(e);
        cap = need;
        return SC_OK;
    }

    hipError_t wait(hipStream_t stream) { return hipStreamWaitEvent(stream, last, 0); }  // behind the previous call, whatever its stream was
    hipError_t record(hipStream_t stream) { return hipEventRecord(last, stream); }
};

// One call of an entry point on its device's slot; declared after `int rc` and before the first `goto done`.  The
// constructor locks the slot and remembers the caller's device.  enter: hipSetDevice, first_use; grow: the buffers
// (open is both; a unit that asks the device for a size in between calls the two).  The unit's staging, sl.wait, its
// work, sl.record and its own hipStreamSynchronize stay explicit.  When the scope ends -- rc is the entry's result
// by then -- a call that failed on the device waits for the stream (settle: nothing of ours still touches the
// caller's memory or the unit's staging), then the caller's device is put back and the slot unlocked.
struct UnitCall {
    CallerDevice caller;
    WorkSlot &sl;
    std::lock_guard<std::mutex> lock;
    UnitError &err;
    const int device;
    const hipStream_t stream;
    const int &rc;
    bool sync_failures = true;  // masks_rgb: only while it holds staging buffers

    UnitCall(UnitError &e, WorkSlot *slots, int dev, hipStream_t st, const int &result)
        : caller(dev), sl(slots[dev]), lock(sl.mu), err(e), device(dev), stream(st), rc(result) {}
    ~UnitCall() { settle(); }

    int enter() {
        const hipError_t e = hipSetDevice(device);
        return e != hipSuccess ? err.hip(e) : sl.first_use(err, device, stream);
    }
    int grow(size_t need) { return sl.grow(err, need); }
    int open(size_t need) { const int r = enter(); return r != SC_OK ? r : grow(need); }
    void settle() {  // (a second wait on a drained stream costs nothing)
        if (sync_failures && rc != SC_OK && rc != SC_ERR_INVALID) (void)hipStreamSynchronize(stream);
    }
};

void release_slots(WorkSlot *slots) {
    on_each_device([slots](int d) {
        WorkSlot &sl = slots[d];
        std::lock_guard<std::mutex> lock(sl.mu);
        if (sl.base && hipSetDevice(d) == hipSuccess) {
            if (sl.last) (void)hipEventSynchronize(sl.last);
            (void)hipFree(sl.base);
            sl.base = nullptr;
            sl.cap = 0;
        }
    });
}

}  // namespace
