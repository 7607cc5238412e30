// spacecarve.hip -- MI355X (gfx950 / CDNA4) voxel back-projection engine + its C ABI.
//
// Replaces, behind include/spacecarve.h, the device layer of the reference:
//   plant3dvision/kernels/backprojection.c  carve :57-84, average :36-55,
//                                           backproject_point :3-34
//   plant3dvision/kernels/common.h          unravel_index :1-12
//   plant3dvision/cl.py                     Backprojection buffer lifecycle :118-311
//
// Design:
//   * State stays in the reference's layout: C-order [nx][ny][nz], int32 / float32.
//   * One lane owns 4 consecutive z-voxels of one (i,j) column: one 16-byte load and one
//     16-byte store per lane, 1 KiB per wavefront instruction; one owner per voxel, so
//     there are no atomics and no races (as in the reference, one work-item per voxel).
//   * A launch applies a CHUNK of views to the state it holds in registers (1 view per
//     launch = the reference's schedule).  The carve update is order-independent, so
//     dead lanes drop out and a wavefront leaves the view loop as soon as a ballot says
//     every one of its voxels is carved.
//   * A fused carve (many views) first settles whole 16x64-voxel BRICKS from four corner
//     projections each: bricks some view sees entirely over background are EMPTY (-1, filled
//     by store blocks beside the final stage), bricks every view sees entirely over
//     foreground are FULL (0 -> 1).  Only the remaining LIVE bricks are projected voxel by
//     voxel, for two views; the voxels still alive are compacted into survivor lists
//     (wave-aggregated atomics on 256 sharded counters) and finished by persistent kernels
//     with one lane per survivor.
//   * Carve masks live in HBM as 1 bit per pixel in 32x32-pixel tiles (one 128-byte line
//     per tile): the 64..256 z-neighbours a wavefront projects land on a short image
//     segment of arbitrary orientation, i.e. on a handful of lines, whatever the camera roll.
//   * The x/y partial sums of every dot product are hoisted per column WITHOUT changing
//     the reference's left-to-right rounding: ((R0*x + R1*y) + R2*z) + t0.
//   * Arithmetic contract: IEEE binary32, no FMA contraction (built with
//     -ffp-contract=off), correctly rounded division, and the (int) cast guarded so
//     that NaN / inf / out-of-range are rejected exactly like x86 cvttss2si -> INT_MIN.
//
// gfx950 only.  No fallback path: every entry point fails with SC_ERR_DEVICE when HIP
// cannot run the kernels.

#include <hip/hip_runtime.h>

#include "hostwait.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "hostpack.h"
#include "spacecarve.h"
#include "spacecarve_tuning.h"

// SC_TRACE_ALLOC=1 in the environment: every allocation of this file reports "sc_alloc <call>:<line> <bytes> <ms>"
// on stderr (bench.py's cold-process leg reads them: what a first batch pays the driver for memory).  Off: a flag test.
namespace sctrace {
inline bool on() {
    static const bool v = [] { const char *s = getenv("SC_TRACE_ALLOC"); return s && *s && *s != '0'; }();
    return v;
}
template <class F>
inline hipError_t timed(const char *what, int line, size_t bytes, F &&f) {
    if (!on()) return f();
    const auto t0 = std::chrono::steady_clock::now();
    const hipError_t r = f();
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    fprintf(stderr, "sc_alloc %s:%d %zu %.3f\n", what, line, bytes, ms);
    return r;
}
template <class T>
inline hipError_t dev(T **p, size_t bytes, int line) {
    return timed("hipMalloc", line, bytes, [&] { return hipMalloc(reinterpret_cast<void **>(p), bytes); });
}
template <class T>
inline hipError_t host(T **p, size_t bytes, unsigned flags, int line) {
    return timed("hipHostMalloc", line, bytes, [&] { return hipHostMalloc(reinterpret_cast<void **>(p), bytes, flags); });
}
}  // namespace sctrace
// every allocation of the engine goes through these two (names of their own: round 5 had #define'd the runtime's)
#define sc_dev_malloc(p, n) sctrace::dev((p), (n), __LINE__)
#define sc_pin_malloc(p, n, f) sctrace::host((p), (n), (f), __LINE__)

#include "sc_own.h"

namespace {

// ------------------------------------------------------------------------------------------
// device side
// ------------------------------------------------------------------------------------------
#include "sc_types.h"
#include "sc_project.h"
#include "sc_stream.h"
#include "sc_pack.h"
#include "sc_verdicts.h"
#include "sc_bricks.h"
#include "sc_lists.h"
#include "sc_average.h"
#include "sc_misc.h"
#include "sc_sparse.h"


// ------------------------------------------------------------------------------------------
// host side
// ------------------------------------------------------------------------------------------

thread_local std::string g_err;
std::atomic<int64_t> g_avg_labels_fused{0};  // sc_average_labels calls that took the shared-launch form

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t _e = (expr);                                                              \
        if (_e != hipSuccess)                                                                \
            return fail(_e == hipErrorOutOfMemory ? SC_ERR_NOMEM : SC_ERR_DEVICE,            \
                        "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,     \
                        __LINE__);                                                           \
    } while (0)

struct Chunk {
    DevPtr<char> base;
    size_t cap = 0, used = 0;
};

struct TimedLaunch {
    Event start, stop;
};

constexpr int kSlots = 4;
constexpr int kNumKernels = 7;

}  // namespace

#include "sc_engine.h"
#include "sc_flush.inl"

// ------------------------------------------------------------------------------------------
// C ABI
// ------------------------------------------------------------------------------------------

#include "sc_api_engine.inl"
#include "sc_api_values.inl"
#include "sc_api_group.inl"

#ifdef SC_TRACE_DENSE  // diagnostic builds only (tools/probes/dense_trace.py)
extern "C" int sc_debug_dense_trace(uint32_t *out) {
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_dense_trace), sizeof(uint32_t) * 8192 * 8);
}
#endif

#include "sc_api_sparse.inl"
#include "sc_comm.inl"
