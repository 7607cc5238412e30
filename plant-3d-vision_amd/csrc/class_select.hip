// class_select.hip -- the decision step of the multiclass PointCloud task on the GPU.
//
// sc_select_classes replaces plant3dvision/tasks/proc3d.py::PointCloud.run :84-115: the float64 [nx, ny, nz, L] copy,
// the arg-max and, per class, an np.delete copy, a max and two comparisons -- as ONE pass over the L class volumes
// that writes ONE byte per voxel, the winner: the index of the class the voxel belongs to, or 255 for none.  Per
// voxel, in binary64 (the background's value times background_prior first):
//   m  = np.argmax of the L values: the first index of the greatest one, or of the first NaN if there is one;
//   v2 = np.max of the other L - 1 values: NaN if one of them is NaN;
//   the voxel belongs to class m iff m is not the background, and (min_contrast > 1.0 is false or
//   1.0 > min_contrast * v2), and 1.0 > min_score; it belongs to no other class.
// Class c's volume of the reference (pred_c, :112-115) is `winner == c`.
//
// Every result is an integer: nothing depends on the order of the atomics.  Stand-alone unit: nothing shared with the
// carve's engine.  The quad walk (loads, geometry, run plan, slabs) is sc_quads.h, shared with evaluate.hip.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "sc_quads.h"
#include "sc_unit.h"

namespace {

constexpr int kB = kQuadThreads;
constexpr int kMaxL = 32;
constexpr uint32_t kNone = 255u;
constexpr uint32_t kLocked = 0x100u, kNan2 = 0x200u;
constexpr int kGroup = 3;  // classes whose loads are in flight together in a WIDE launch

thread_local UnitError g_err;
ChunkLimit g_chunk;

// The quad walk of sc_quads.h.  The quad's 4 winners are one 4-byte store where the quad is whole and its address
// aligned, byte stores otherwise: nothing is written beyond the quad's own voxels.
//
// Counting: per class, `winner == c` is a wave-wide ballot whose bit count lands in a scalar register; lane 0 adds
// the quad's four to the block's 32-bit counters in LDS (a block handles at most 1024 * xc < 2^32 voxels), which are
// flushed as 64-bit adds when the block ends.
struct SelArgs {
    const void *vol[kMaxL];
    QuadGeom g;
    double background_prior, min_contrast;
    int contrast_on;  // min_contrast > 1.0
    int score_ok;     // 1.0 > min_score
};

// The arg-max state of a quad: v1, v2 the greatest and the second greatest of the values that are not NaN; st the
// arg-max so far, with kLocked: it is the first NaN's index, kNan2: a second value was NaN.
struct Best {
    double v1[4], v2[4];
    uint32_t st[4];
};

// class c's values v (the background's already have their prior).  Selects only, no branch: the loads of the classes
// that follow need not wait for this one's verdict.
__device__ __forceinline__ void take(Best &b, const double v[4], double scale, int c) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const double x = v[j] * scale;  // :89, in binary64; x * 1.0 is x
        const bool isnan = x != x, greater = x > b.v1[j], locked = (b.st[j] & kLocked) != 0u;  // NaN is not greater
        b.v2[j] = greater ? b.v1[j] : (x > b.v2[j] ? x : b.v2[j]);  // a later equal value is no new maximum
        b.v1[j] = greater ? x : b.v1[j];
        b.st[j] = isnan ? (locked ? (b.st[j] | kNan2) : ((uint32_t)c | kLocked)) : ((greater && !locked) ? (uint32_t)c : b.st[j]);
    }
}

// WIDE: the host has seen that every quad of the launch is whole and aligned (nz a multiple of 4, aligned base
// pointers): the wide loads are taken without a test, kGroup classes at a time, so that several are in flight.
template <class T, bool WIDE>
__global__ __launch_bounds__(kB) void select_classes_kernel(SelArgs a, uint8_t *__restrict__ winner,
                                                            unsigned long long *__restrict__ counts) {
    __shared__ uint32_t scnt[kMaxL];
    if (threadIdx.x < kMaxL) scnt[threadIdx.x] = 0u;
    __syncthreads();
    const QuadGeom &g = a.g;
    const QuadAt t = quad_at(g);  // a thread beyond the plane has the address of quad 0, which a WIDE launch may read
    const int y = t.y, z0 = t.z0, nv = t.nv;
    const int lane = (int)(threadIdx.x & 63);
    const double ninf = -__builtin_huge_val(), qnan = __builtin_nan("");
    for (int64_t x = t.x0; x < t.x1; ++x) {  // block-uniform: every ballot below is taken by whole wavefronts
        const int64_t at = (x * g.ny + y) * (int64_t)g.nz + z0;
        Best b;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            b.v1[j] = ninf;
            b.v2[j] = ninf;
            b.st[j] = 0u;
        }
        int c = 0;
        if (WIDE) {
            for (; c + kGroup <= g.L; c += kGroup) {
                Quad<T> raw[kGroup];
#pragma unroll
                for (int k = 0; k < kGroup; ++k) raw[k].load(static_cast<const T *>(a.vol[c + k]) + at);
#pragma unroll
                for (int k = 0; k < kGroup; ++k) {
                    double v[4];
                    raw[k].widen(v);
                    take(b, v, c + k == g.background ? a.background_prior : 1.0, c + k);
                }
            }
        }
        for (; c < g.L; ++c) {
            double v[4];
            if (WIDE) {
                Quad<T> raw;
                raw.load(static_cast<const T *>(a.vol[c]) + at);
                raw.widen(v);
            } else {
                load4<T>(static_cast<const T *>(a.vol[c]) + at, nv, 0.0, v);
            }
            take(b, v, c == g.background ? a.background_prior : 1.0, c);
        }
        uint32_t w[4];  // the class the voxel belongs to, or kNone
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            // with one NaN the arg-max is its index and the others' maximum is v1; with two the maximum is NaN too.
            // (L >= 2: without a NaN v2 has seen a value, with one NaN v1 has.)
            const uint32_t mm = b.st[j] & 255u;
            const double others = (b.st[j] & kNan2) ? qnan : (b.st[j] & kLocked) ? b.v1[j] : b.v2[j];
            const bool contrast = !a.contrast_on || 1.0 > a.min_contrast * others;  // a NaN product compares false
            w[j] = (j < nv && (int)mm != g.background && contrast && a.score_ok) ? mm : kNone;
        }
        for (int c = 0; c < g.L; ++c) {  // (ballots inside: the compiler does not unroll it)
            if (c == g.background) continue;
            uint32_t tot = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) tot += (uint32_t)__popcll(__ballot(w[j] == (uint32_t)c));
            if (lane == 0 && tot != 0u) atomicAdd(&scnt[c], tot);
        }
        uint8_t *dst = winner + at;
        if (WIDE ? t.live : (nv == 4 && (reinterpret_cast<uintptr_t>(dst) & 3) == 0)) {
            *reinterpret_cast<uint32_t *>(dst) = w[0] | (w[1] << 8) | (w[2] << 16) | (w[3] << 24);
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (j < nv) dst[j] = (uint8_t)w[j];
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < g.L && scnt[threadIdx.x] != 0u) atomicAdd(&counts[threadIdx.x], (unsigned long long)scnt[threadIdx.x]);
}

// ---- host side -------------------------------------------------------------------------------------------------
// Work buffers (the counters, the slabs of host inputs and of their winners) are kept per device: the slot protocol
// of sc_unit.h.
WorkSlot g_slots[kUnitDevices];

// One launch over `planes` x-planes; a.vol and winner are device pointers to plane 0 of the launch.
void launch_select(int dtype, hipStream_t stream, SelArgs a, int64_t planes, uint8_t *winner, unsigned long long *counts) {
    const dim3 grid = plan_quads(a.g, planes);
    // every quad whole and aligned: rows of whole quads and base pointers on 16 (uint8: 4) and 4 bytes
    uintptr_t low = reinterpret_cast<uintptr_t>(winner) & 3;
    for (int c = 0; c < a.g.L; ++c) low |= reinterpret_cast<uintptr_t>(a.vol[c]) & (dtype == SC_EVAL_U8 ? 3 : 15);
    const bool wide = low == 0 && a.g.nz % 4 == 0;
#define SEL_LAUNCH(T)                                                                                             \
    do {                                                                                                          \
        if (wide)                                                                                                 \
            hipLaunchKernelGGL((select_classes_kernel<T, true>), grid, dim3(kB), 0, stream, a, winner, counts);   \
        else                                                                                                      \
            hipLaunchKernelGGL((select_classes_kernel<T, false>), grid, dim3(kB), 0, stream, a, winner, counts);  \
    } while (0)
    if (dtype == SC_EVAL_F32)
        SEL_LAUNCH(float);
    else if (dtype == SC_EVAL_F64)
        SEL_LAUNCH(double);
    else
        SEL_LAUNCH(uint8_t);
#undef SEL_LAUNCH
}

}  // namespace

extern "C" {

const char *sc_select_last_error(void) { return g_err.msg; }

void sc_select_set_chunk_bytes(int64_t bytes) { g_chunk.set(bytes); }

int sc_select_classes(const void *const *volumes, int dtype, int L, int background, int64_t nx, int64_t ny, int64_t nz,
                      double background_prior, double min_contrast, double min_score, int on_device, int device,
                      void *hip_stream, uint8_t *winner, int64_t *counts) {
    // every argument is judged before the first device call
    if (!volumes || !winner || !counts) return g_err.fail(SC_ERR_INVALID, "null argument (volumes, winner, counts)");
    if (L < 2 || L > kMaxL) return g_err.fail(SC_ERR_INVALID, "L must be 2..32 classes");
    if (dtype != SC_EVAL_F32 && dtype != SC_EVAL_F64 && dtype != SC_EVAL_U8)
        return g_err.fail(SC_ERR_INVALID, "dtype: 1 float32, 2 float64, 3 uint8");
    if (background < -1 || background >= L) return g_err.fail(SC_ERR_INVALID, "background must be -1 (none) or a class index");
    if (nx < 1 || ny < 1 || nz < 1) return g_err.fail(SC_ERR_INVALID, "nx, ny and nz must be at least 1");
    if (nx >= ((int64_t)1 << 31) || ny >= ((int64_t)1 << 31) || nz >= ((int64_t)1 << 31))
        return g_err.fail(SC_ERR_INVALID, "every axis must be below 2^31");
    if ((double)nx * (double)ny * (double)nz >= 4.0e18 / 8.0) return g_err.fail(SC_ERR_INVALID, "volume too large");
    for (int c = 0; c < L; ++c)
        if (!volumes[c]) return g_err.fail(SC_ERR_INVALID, "null volume pointer");
    if (device < 0 || device >= kUnitDevices) return g_err.fail(SC_ERR_INVALID, "device ordinal out of range");
    if (!one_launch_holds(nx, ny, nz)) return g_err.fail(SC_ERR_INVALID, "volume too large for one launch");

    const size_t plane = (size_t)ny * nz, vplane = plane * dtype_bytes(dtype);  // one x-plane: of winners, of a volume

    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    unsigned long long raw[kMaxL];
    SelArgs a;
    memset(&a, 0, sizeof a);
    set_quads(a.g, L, background, ny, nz);
    a.background_prior = background_prior;
    a.min_contrast = min_contrast;
    a.contrast_on = min_contrast > 1.0 ? 1 : 0;
    a.score_ok = 1.0 > min_score ? 1 : 0;

    // layout of the work buffer: counters, then (host volumes) one slab of whole x-planes per volume and one of winners
    Layout lay;
    const size_t o_cnt = lay.take(sizeof raw);
    int64_t slab = nx;  // x-planes per slab
    size_t o_vol[kMaxL], o_win = 0;
    if (!on_device) {
        slab = std::min(nx, slab_planes(g_chunk.get(), lay.total, (size_t)L * vplane + plane, (size_t)(L + 1) * 256));
        for (int c = 0; c < L; ++c) o_vol[c] = lay.take((size_t)slab * vplane);
        o_win = lay.take((size_t)slab * plane);
    }

    if ((rc = call.open(lay.total)) != SC_OK) goto done;
    {
        char *const w = call.sl.base;
        unsigned long long *cnt_d = reinterpret_cast<unsigned long long *>(w + o_cnt);
        UNIT_TRY(call.sl.wait(stream));
        UNIT_TRY(hipMemsetAsync(cnt_d, 0, sizeof raw, stream));
        if (on_device) {
            for (int c = 0; c < L; ++c) a.vol[c] = volumes[c];
            launch_select(dtype, stream, a, nx, winner, cnt_d);
            UNIT_TRY(hipGetLastError());
        } else {
            uint8_t *win_d = reinterpret_cast<uint8_t *>(w + o_win);
            for (int64_t xa = 0; xa < nx; xa += slab) {
                const int64_t planes = std::min(slab, nx - xa);
                for (int c = 0; c < L; ++c) {
                    UNIT_TRY(hipMemcpyAsync(w + o_vol[c], static_cast<const char *>(volumes[c]) + (size_t)xa * vplane,
                                            (size_t)planes * vplane, hipMemcpyHostToDevice, stream));
                    a.vol[c] = w + o_vol[c];
                }
                launch_select(dtype, stream, a, planes, win_d, cnt_d);
                UNIT_TRY(hipGetLastError());
                // (the next slab's copies follow this one on the stream)
                UNIT_TRY(hipMemcpyAsync(winner + (size_t)xa * plane, win_d, (size_t)planes * plane, hipMemcpyDeviceToHost, stream));
            }
        }
        UNIT_TRY(hipMemcpyAsync(raw, cnt_d, sizeof raw, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        UNIT_TRY(hipStreamSynchronize(stream));
        for (int c = 0; c < L; ++c) counts[c] = (int64_t)raw[c];
    }

done:
    return rc;
}

void sc_select_release(void) { release_slots(g_slots); }

}  // extern "C"
