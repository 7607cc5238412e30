// evaluate.hip -- the two evaluation tasks' counting passes on the GPU.
//
// sc_eval_voxels replaces the body of plant3dvision/tasks/evaluation.py::VoxelsEvaluation.evaluate (:421-477): the
// float64 [nx, ny, nz, L] copy, the argmax, and per class an np.delete copy, a max, a comparison and four
// boolean-index sums -- as ONE pass over the L prediction and the L ground-truth volumes.  Per voxel, in binary64:
//   m = first index of the greatest prediction, v1 = that value, v2 = the greatest of the other L - 1 values;
//   the voxel predicts class m iff v1 > min_contrast * v2 and none of its L values is NaN; it predicts no other class.
// Per class c other than the background, with g = gt_c at the voxel: g > 0.5 counts into tp or fn, g < 0.5 into fp or
// tn, anything else (0.5, NaN) nowhere.  Only m can be predicted, so the kernel counts pos (g > 0.5), neg (g < 0.5),
// tp and fp, and the host derives fn = pos - tp, tn = neg - fp.
//
// sc_eval_masks replaces plant3dvision/metrics.py::MaskEvaluator.evaluate (:246-272) for a stack of pictures:
// `dilation_amount` steps of scipy.ndimage.binary_dilation (the 4-connected cross, background outside the picture) on
// pred != 0, then four sums against gt != 0.  The steps run on bit planes (1 bit per pixel, 64-bit words), up to 32
// of them per launch on tiles in LDS; more steps take more launches; H + W steps saturate any picture.
//
// Every count is an integer: no result depends on the order of the atomics.  Nothing shared with the engine; the quad
// walk over volumes is sc_quads.h (with class_select.hip), the dilation of bit planes sc_bitplane.h (with masks_rgb.hip).

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>

#include "sc_bitplane.h"
#include "sc_quads.h"
#include "sc_unit.h"

namespace {

constexpr int kB = kQuadThreads;
constexpr int kMaxL = 32;

thread_local UnitError g_err;
ChunkLimit g_chunk;

// ---- volumes ---------------------------------------------------------------------------------------------------
// The quad walk of sc_quads.h: loads and planning come from there.  The geometry stays here: VoxArgs holds QuadGeom's
// fields flat and the kernel derives its place itself, the arithmetic of quad_at.  With the struct embedded or quad_at
// called, the compiler schedules this kernel differently and it ran 1 to 2% slower (profiles/units_refactor_ab.json).
// Ground truth is indexed with its own pitches (gy, gz); only its corner [0:nx, 0:ny, 0:nz] is touched.
//
// Counting: the four predicates of a class are wave-wide ballots whose bit counts land in scalar registers; lanes
// 0..3 add them to the block's 32-bit counters in LDS (a block handles at most 1024 * xc < 2^32 voxels), which are
// flushed as 64-bit adds when the block ends.  counts[c] = {pos, neg, tp, fp}; the background's row stays zero.
// Projection: a bit per class and voxel of the quad, set where some x-plane of the run predicts the class; bytes of
// 1 are stored at the end (the buffer was zeroed; several runs may store the same 1).
struct VoxArgs {
    const void *pred[kMaxL];
    const void *gt[kMaxL];  // gt[background] is not read
    int L, background;  // QuadGeom's fields: set_quads and plan_quads fill them
    int nx, ny, nz, Q, xc;
    uint32_t tiles;
    int64_t gy, gz;
    double min_contrast;
};

template <class TP, class TG>
__global__ __launch_bounds__(kB) void eval_voxels_kernel(VoxArgs a, unsigned long long *__restrict__ counts,
                                                         uint8_t *__restrict__ proj) {
    __shared__ uint32_t scnt[kMaxL * 4];
    if (threadIdx.x < kMaxL * 4) scnt[threadIdx.x] = 0u;
    __syncthreads();
    const uint32_t tile = blockIdx.x % a.tiles, run = blockIdx.x / a.tiles;
    const int64_t q = (int64_t)tile * kB + threadIdx.x, nq = (int64_t)a.ny * a.Q;
    const bool live = q < nq;
    const int y = live ? (int)(q / a.Q) : 0, z0 = live ? (int)(q % a.Q) * 4 : 0;
    const int nv = live ? min(4, a.nz - z0) : 0;  // voxels of this thread's quad: 0 for a thread beyond the plane
    const int64_t x0 = (int64_t)run * a.xc, x1 = min((int64_t)a.nx, x0 + a.xc);
    const int lane = (int)(threadIdx.x & 63);
    const double ninf = -__builtin_huge_val(), qnan = __builtin_nan("");
    uint32_t seen[4] = {0u, 0u, 0u, 0u};
    for (int64_t x = x0; x < x1; ++x) {  // block-uniform: every ballot below is taken by whole wavefronts
        const int64_t po = (x * a.ny + y) * (int64_t)a.nz + z0, go = (x * a.gy + y) * a.gz + z0;
        double v1[4], v2[4];
        int m[4];
        bool bad[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            v1[j] = ninf;
            v2[j] = ninf;
            m[j] = 0;
            bad[j] = false;
        }
#pragma unroll 2
        for (int c = 0; c < a.L; ++c) {
            double v[4];
            load4<TP>(static_cast<const TP *>(a.pred[c]) + po, nv, 0.0, v);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                bad[j] = bad[j] || (v[j] != v[j]);
                if (v[j] > v1[j]) {  // a later equal value is no new maximum: the first index stays
                    v2[j] = v1[j];
                    v1[j] = v[j];
                    m[j] = c;
                } else {
                    v2[j] = v[j] > v2[j] ? v[j] : v2[j];
                }
            }
        }
        int pm[4];  // the class the voxel predicts, or -1
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            pm[j] = (j < nv && !bad[j] && v1[j] > a.min_contrast * v2[j]) ? m[j] : -1;
            if (pm[j] >= 0) seen[j] |= 1u << pm[j];
        }
        for (int c = 0; c < a.L; ++c) {  // (ballots inside: the compiler does not unroll it)
            if (c == a.background) continue;
            double g[4];
            load4<TG>(static_cast<const TG *>(a.gt[c]) + go, nv, qnan, g);  // beyond the quad: NaN, counted nowhere
            uint32_t pos = 0u, neg = 0u, tp = 0u, fp = 0u;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const bool hi = g[j] > 0.5, lo = g[j] < 0.5, mine = pm[j] == c;
                pos += (uint32_t)__popcll(__ballot(hi));
                neg += (uint32_t)__popcll(__ballot(lo));
                tp += (uint32_t)__popcll(__ballot(hi && mine));
                fp += (uint32_t)__popcll(__ballot(lo && mine));
            }
            const uint32_t val = lane == 0 ? pos : lane == 1 ? neg : lane == 2 ? tp : fp;
            if (lane < 4 && val != 0u) atomicAdd(&scnt[c * 4 + lane], val);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x < a.L * 4 && scnt[threadIdx.x] != 0u) atomicAdd(&counts[threadIdx.x], (unsigned long long)scnt[threadIdx.x]);
    if (proj != nullptr && live) {
        for (int c = 0; c < a.L; ++c) {
            if (c == a.background) continue;
            uint8_t *row = proj + ((int64_t)c * a.ny + y) * (int64_t)a.nz + z0;
            for (int j = 0; j < nv; ++j)
                if ((seen[j] >> c) & 1u) row[j] = 1;
        }
    }
}

// ---- masks -----------------------------------------------------------------------------------------------------
// A segment is 64 consecutive pixels of one row = one 64-bit word of the row's bit mask (pixel x at bit x & 63 of
// word x >> 6; bits beyond W are 0): one byte per lane, one __ballot per segment, so W and the pointers need no
// alignment.  A wavefront takes kSegWave consecutive segments of one picture, a block 4 x kSegWave.
constexpr int kSegWave = 16, kSegBlock = kSegWave * (kB / 64);

__global__ __launch_bounds__(kB) void eval_pack_kernel(const uint8_t *__restrict__ pred, int H, int W, int Wd, int blocks_per_pic,
                                                       unsigned long long *__restrict__ bits) {
    const int v = (int)(blockIdx.x / (uint32_t)blocks_per_pic), b = (int)(blockIdx.x % (uint32_t)blocks_per_pic);
    const int lane = (int)(threadIdx.x & 63);
    const int64_t nseg = (int64_t)H * Wd;
    const int64_t s0 = (int64_t)b * kSegBlock + (int64_t)(threadIdx.x >> 6) * kSegWave, s1 = min(nseg, s0 + kSegWave);
    const uint8_t *pic = pred + (int64_t)v * H * W;
    for (int64_t s = s0; s < s1; ++s) {  // wave-uniform
        const int y = (int)(s / Wd), x = (int)(s % Wd) * 64 + lane;
        const bool on = x < W && pic[(int64_t)y * W + x] != 0;
        const unsigned long long word = __ballot(on);
        if (lane == 0) bits[(int64_t)v * nseg + s] = word;
    }
}

// counts[v] = {tp, fn, tn, fp} (the order of MaskEvaluator).  FROM_BITS: the prediction is the dilated bit plane,
// else pred != 0 read as bytes (dilation_amount 0: no bit plane is made).
template <bool FROM_BITS>
__global__ __launch_bounds__(kB) void eval_count_kernel(const uint8_t *__restrict__ gt, const uint8_t *__restrict__ pred,
                                                        const unsigned long long *__restrict__ bits, int H, int W, int Wd,
                                                        int blocks_per_pic, unsigned long long *__restrict__ counts) {
    __shared__ uint32_t s4[4];
    if (threadIdx.x < 4) s4[threadIdx.x] = 0u;
    __syncthreads();
    const int v = (int)(blockIdx.x / (uint32_t)blocks_per_pic), b = (int)(blockIdx.x % (uint32_t)blocks_per_pic);
    const int lane = (int)(threadIdx.x & 63);
    const int64_t nseg = (int64_t)H * Wd;
    const int64_t s0 = (int64_t)b * kSegBlock + (int64_t)(threadIdx.x >> 6) * kSegWave, s1 = min(nseg, s0 + kSegWave);
    const int64_t pic = (int64_t)v * H * W;
    uint32_t tp = 0u, fn = 0u, tn = 0u, fp = 0u;  // wave-uniform
    for (int64_t s = s0; s < s1; ++s) {
        const int y = (int)(s / Wd), wx = (int)(s % Wd), x = wx * 64 + lane;
        const bool in = x < W;
        const int64_t at = pic + (int64_t)y * W + x;
        const unsigned long long valid = __ballot(in);
        const unsigned long long g = __ballot(in && gt[at] != 0);
        unsigned long long p;
        if (FROM_BITS)
            p = bits[(int64_t)v * nseg + s];
        else
            p = __ballot(in && pred[at] != 0);
        tp += (uint32_t)__popcll(g & p);
        fn += (uint32_t)__popcll(g & ~p);
        tn += (uint32_t)__popcll(valid & ~g & ~p);
        fp += (uint32_t)__popcll(valid & ~g & p);
    }
    const uint32_t val = lane == 0 ? tp : lane == 1 ? fn : lane == 2 ? tn : fp;
    if (lane < 4 && val != 0u) atomicAdd(&s4[lane], val);
    __syncthreads();
    if (threadIdx.x < 4 && s4[threadIdx.x] != 0u) atomicAdd(&counts[(int64_t)v * 4 + threadIdx.x], (unsigned long long)s4[threadIdx.x]);
}

// `steps` (1..kMaxSteps) steps of the cross on the bit planes, `in` -> `out` (two different buffers): the tiles of
// sc_bitplane.h with the constant diamond as every step's footprint, which the compiler folds to the five-term cross.
struct CrossFoot { __device__ constexpr uint32_t operator()(int) const { return kDiamond; } };

__global__ __launch_bounds__(kB) void eval_dilate_kernel(const unsigned long long *__restrict__ in, int H, int W, int Wd, int tiles_x,
                                                         int tiles_y, int steps, unsigned long long *__restrict__ out) {
    __shared__ unsigned long long buf[2][kPlaneCells];
    const uint32_t per_pic = (uint32_t)tiles_x * (uint32_t)tiles_y;
    const int v = (int)(blockIdx.x / per_pic), t = (int)(blockIdx.x % per_pic);
    const int ty = t / tiles_x, tx = t % tiles_x;
    const unsigned long long *res = buf[dilate_tile<kB>(buf, in + (int64_t)v * H * Wd, H, W, Wd, ty, tx, steps, CrossFoot())];
    unsigned long long *dst = out + (int64_t)v * H * Wd;
    for (int c = threadIdx.x; c < kTR * kTW; c += kB) {
        const int lr = c / kTW, lw = c % kTW;
        const int y = ty * kTR + lr, w = tx * kTW + lw;
        if (y < H && w < Wd) dst[(int64_t)y * Wd + w] = res[(lr + steps) * kLW + 1 + lw];
    }
}

// ---- host side -------------------------------------------------------------------------------------------------
// Work buffers (counters, projection, bit planes, the slabs of host inputs) are kept per device: the slot protocol
// of sc_unit.h.
WorkSlot g_slots[kUnitDevices];

template <class TP>
void launch_voxels_gt(int gt_dtype, dim3 grid, hipStream_t stream, const VoxArgs &a, unsigned long long *counts, uint8_t *proj) {
    if (gt_dtype == SC_EVAL_F32)
        hipLaunchKernelGGL((eval_voxels_kernel<TP, float>), grid, dim3(kB), 0, stream, a, counts, proj);
    else if (gt_dtype == SC_EVAL_F64)
        hipLaunchKernelGGL((eval_voxels_kernel<TP, double>), grid, dim3(kB), 0, stream, a, counts, proj);
    else
        hipLaunchKernelGGL((eval_voxels_kernel<TP, uint8_t>), grid, dim3(kB), 0, stream, a, counts, proj);
}

// One launch over `planes` x-planes; a.pred / a.gt are device pointers to plane 0 of the launch.
void launch_voxels(int pred_dtype, int gt_dtype, hipStream_t stream, VoxArgs a, int64_t planes, unsigned long long *counts,
                   uint8_t *proj) {
    const dim3 grid = plan_quads(a, planes);
    if (pred_dtype == SC_EVAL_F32)
        launch_voxels_gt<float>(gt_dtype, grid, stream, a, counts, proj);
    else
        launch_voxels_gt<double>(gt_dtype, grid, stream, a, counts, proj);
}

}  // namespace

extern "C" {

const char *sc_eval_last_error(void) { return g_err.msg; }

void sc_eval_set_chunk_bytes(int64_t bytes) { g_chunk.set(bytes); }

int sc_eval_voxels(const void *const *pred, int pred_dtype, const void *const *gt, int gt_dtype, int L, int64_t nx, int64_t ny,
                   int64_t nz, int64_t gx, int64_t gy, int64_t gz, int background, double min_contrast, int on_device, int device,
                   void *hip_stream, int64_t *counts_out, uint8_t *projection_out) {
    // every argument is judged before the first device call
    if (!pred || !gt || !counts_out) return g_err.fail(SC_ERR_INVALID, "null argument (pred, gt, counts_out)");
    if (L < 2 || L > kMaxL) return g_err.fail(SC_ERR_INVALID, "L must be 2..32 classes");
    if (pred_dtype != SC_EVAL_F32 && pred_dtype != SC_EVAL_F64)
        return g_err.fail(SC_ERR_INVALID, "pred_dtype: 1 float32, 2 float64");
    if (gt_dtype != SC_EVAL_F32 && gt_dtype != SC_EVAL_F64 && gt_dtype != SC_EVAL_U8)
        return g_err.fail(SC_ERR_INVALID, "gt_dtype: 1 float32, 2 float64, 3 uint8");
    if (background < -1 || background >= L) return g_err.fail(SC_ERR_INVALID, "background must be -1 (none) or a class index");
    if (nx < 1 || ny < 1 || nz < 1) return g_err.fail(SC_ERR_INVALID, "nx, ny and nz must be at least 1");
    if (gx < nx || gy < ny || gz < nz) return g_err.fail(SC_ERR_INVALID, "ground truth smaller than the prediction");
    if (gx >= ((int64_t)1 << 31) || gy >= ((int64_t)1 << 31) || gz >= ((int64_t)1 << 31))
        return g_err.fail(SC_ERR_INVALID, "every axis must be below 2^31");
    if ((double)gx * (double)gy * (double)gz >= 4.0e18 / 8.0) return g_err.fail(SC_ERR_INVALID, "volume too large");
    for (int c = 0; c < L; ++c)
        if (!pred[c] || (!gt[c] && c != background)) return g_err.fail(SC_ERR_INVALID, "null volume pointer");
    if (device < 0 || device >= kUnitDevices) return g_err.fail(SC_ERR_INVALID, "device ordinal out of range");
    if (!one_launch_holds(nx, ny, nz)) return g_err.fail(SC_ERR_INVALID, "volume too large for one launch");

    const size_t sp = dtype_bytes(pred_dtype), sg = dtype_bytes(gt_dtype);
    const size_t pplane = (size_t)ny * nz * sp, gplane = (size_t)gy * gz * sg;  // one x-plane of a volume
    const int Lg = L - (background >= 0 ? 1 : 0);
    const size_t projbytes = projection_out ? (size_t)L * ny * nz : 0;

    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    unsigned long long raw[kMaxL * 4];
    VoxArgs a;
    memset(&a, 0, sizeof a);
    set_quads(a, L, background, ny, nz);
    a.gy = gy;
    a.gz = gz;
    a.min_contrast = min_contrast;

    // layout of the work buffer: counters, projection, then (host volumes) one slab of whole x-planes per volume
    Layout lay;
    const size_t o_cnt = lay.take(sizeof raw), o_proj = lay.take(projbytes);
    int64_t slab = nx;  // x-planes per slab
    size_t o_pred[kMaxL], o_gt[kMaxL];
    if (!on_device) {
        slab = std::min(nx, slab_planes(g_chunk.get(), lay.total, (size_t)L * pplane + (size_t)Lg * gplane, (size_t)(L + Lg) * 256));
        for (int c = 0; c < L; ++c) o_pred[c] = lay.take((size_t)slab * pplane);
        for (int c = 0; c < L; ++c) o_gt[c] = c == background ? 0 : lay.take((size_t)slab * gplane);
    }

    if ((rc = call.open(lay.total)) != SC_OK) goto done;
    {
        char *const w = call.sl.base;
        unsigned long long *counts = reinterpret_cast<unsigned long long *>(w + o_cnt);
        uint8_t *proj = projection_out ? reinterpret_cast<uint8_t *>(w + o_proj) : nullptr;
        UNIT_TRY(call.sl.wait(stream));
        UNIT_TRY(hipMemsetAsync(counts, 0, sizeof raw, stream));
        if (proj) UNIT_TRY(hipMemsetAsync(proj, 0, projbytes, stream));
        if (on_device) {
            for (int c = 0; c < L; ++c) {
                a.pred[c] = pred[c];
                a.gt[c] = c == background ? nullptr : gt[c];
            }
            launch_voxels(pred_dtype, gt_dtype, stream, a, nx, counts, proj);
            UNIT_TRY(hipGetLastError());
        } else {
            for (int64_t xa = 0; xa < nx; xa += slab) {
                const int64_t planes = std::min(slab, nx - xa);
                for (int c = 0; c < L; ++c) {
                    UNIT_TRY(hipMemcpyAsync(w + o_pred[c], static_cast<const char *>(pred[c]) + (size_t)xa * pplane,
                                            (size_t)planes * pplane, hipMemcpyHostToDevice, stream));
                    a.pred[c] = w + o_pred[c];
                    a.gt[c] = nullptr;
                    if (c == background) continue;
                    UNIT_TRY(hipMemcpyAsync(w + o_gt[c], static_cast<const char *>(gt[c]) + (size_t)xa * gplane,
                                            (size_t)planes * gplane, hipMemcpyHostToDevice, stream));
                    a.gt[c] = w + o_gt[c];
                }
                launch_voxels(pred_dtype, gt_dtype, stream, a, planes, counts, proj);  // the next slab's copies follow it on the stream
                UNIT_TRY(hipGetLastError());
            }
        }
        UNIT_TRY(hipMemcpyAsync(raw, counts, sizeof raw, hipMemcpyDeviceToHost, stream));
        if (proj) UNIT_TRY(hipMemcpyAsync(projection_out, proj, projbytes, hipMemcpyDeviceToHost, stream));
        UNIT_TRY(call.sl.record(stream));
        UNIT_TRY(hipStreamSynchronize(stream));
        for (int c = 0; c < L; ++c) {  // {pos, neg, tp, fp} -> {tp, fp, tn, fn}
            const int64_t pos = (int64_t)raw[4 * c], neg = (int64_t)raw[4 * c + 1], tp = (int64_t)raw[4 * c + 2], fp = (int64_t)raw[4 * c + 3];
            counts_out[4 * c] = tp;
            counts_out[4 * c + 1] = fp;
            counts_out[4 * c + 2] = neg - fp;
            counts_out[4 * c + 3] = pos - tp;
        }
    }

done:
    return rc;
}

int sc_eval_masks(const void *gt, const void *pred, int on_device, int n, int H, int W, int dilation_amount, int device,
                  void *hip_stream, int64_t *counts_out) {
    // every argument is judged before the first device call
    if (!gt || !pred || !counts_out) return g_err.fail(SC_ERR_INVALID, "null argument (gt, pred, counts_out)");
    if (n < 1 || H < 1 || W < 1) return g_err.fail(SC_ERR_INVALID, "n, H and W must be at least 1");
    if ((int64_t)H * W >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "picture too large: H * W must be below 2^31");
    if (dilation_amount < 0) return g_err.fail(SC_ERR_INVALID, "dilation_amount must not be negative");
    if (device < 0 || device >= kUnitDevices) return g_err.fail(SC_ERR_INVALID, "device ordinal out of range");
    const int64_t npix = (int64_t)H * W;
    const int Wd = (W + 63) / 64;
    const int64_t nseg = (int64_t)H * Wd;
    const int64_t sblocks = (nseg + kSegBlock - 1) / kSegBlock;  // blocks per picture of pack and count
    const int tiles_x = (Wd + kTW - 1) / kTW, tiles_y = (H + kTR - 1) / kTR;
    const int64_t dblocks = (int64_t)tiles_x * tiles_y;
    // H + W steps fill any picture that has a set pixel (its L1 diameter is H + W - 2): more change nothing
    const int64_t k = std::min<int64_t>(dilation_amount, (int64_t)H + W);
    // pictures per batch: what one launch can index and, for host pictures, what the chunk limit leaves room for
    const size_t planebytes = k > 0 ? (size_t)nseg * 8 : 0;
    const size_t per_pic = 32 + 2 * planebytes + (on_device ? 0 : 2 * (size_t)npix);
    int64_t nb = std::min<int64_t>(n, 0x7fffffffLL / std::max(sblocks, dblocks));
    if (!on_device) nb = std::min<int64_t>(nb, std::max<int64_t>(1, (int64_t)(g_chunk.get() / per_pic)));

    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    Layout lay;
    const size_t o_cnt = lay.take((size_t)nb * 32), o_b0 = lay.take((size_t)nb * planebytes), o_b1 = lay.take((size_t)nb * planebytes);
    const size_t o_gt = lay.take(on_device ? 0 : (size_t)nb * npix), o_pr = lay.take(on_device ? 0 : (size_t)nb * npix);

    if ((rc = call.open(lay.total)) != SC_OK) goto done;
    {
        char *const w = call.sl.base;
        unsigned long long *counts = reinterpret_cast<unsigned long long *>(w + o_cnt);
        unsigned long long *b0 = reinterpret_cast<unsigned long long *>(w + o_b0), *b1 = reinterpret_cast<unsigned long long *>(w + o_b1);
        UNIT_TRY(call.sl.wait(stream));
        for (int64_t v0 = 0; v0 < n; v0 += nb) {
            const int64_t m = std::min<int64_t>(nb, n - v0);
            const uint8_t *gt_d = static_cast<const uint8_t *>(gt) + (size_t)v0 * npix, *pr_d = static_cast<const uint8_t *>(pred) + (size_t)v0 * npix;
            if (!on_device) {
                UNIT_TRY(hipMemcpyAsync(w + o_gt, gt_d, (size_t)m * npix, hipMemcpyHostToDevice, stream));
                UNIT_TRY(hipMemcpyAsync(w + o_pr, pr_d, (size_t)m * npix, hipMemcpyHostToDevice, stream));
                gt_d = reinterpret_cast<const uint8_t *>(w + o_gt);
                pr_d = reinterpret_cast<const uint8_t *>(w + o_pr);
            }
            UNIT_TRY(hipMemsetAsync(counts, 0, (size_t)m * 32, stream));
            if (k == 0) {
                hipLaunchKernelGGL(eval_count_kernel<false>, dim3((uint32_t)(sblocks * m)), dim3(kB), 0, stream, gt_d, pr_d,
                                   (const unsigned long long *)nullptr, H, W, Wd, (int)sblocks, counts);
            } else {
                hipLaunchKernelGGL(eval_pack_kernel, dim3((uint32_t)(sblocks * m)), dim3(kB), 0, stream, pr_d, H, W, Wd, (int)sblocks, b0);
                unsigned long long *from = b0, *to = b1;
                for (int64_t done_steps = 0; done_steps < k; done_steps += kMaxSteps) {
                    const int steps = (int)std::min<int64_t>(kMaxSteps, k - done_steps);
                    hipLaunchKernelGGL(eval_dilate_kernel, dim3((uint32_t)(dblocks * m)), dim3(kB), 0, stream, from, H, W, Wd, tiles_x,
                                       tiles_y, steps, to);
                    std::swap(from, to);
                }
                hipLaunchKernelGGL(eval_count_kernel<true>, dim3((uint32_t)(sblocks * m)), dim3(kB), 0, stream, gt_d,
                                   (const uint8_t *)nullptr, from, H, W, Wd, (int)sblocks, counts);
            }
            UNIT_TRY(hipGetLastError());
            // (the next batch's memset follows this copy on the stream)
            UNIT_TRY(hipMemcpyAsync(counts_out + 4 * v0, counts, (size_t)m * 32, hipMemcpyDeviceToHost, stream));
        }
        UNIT_TRY(call.sl.record(stream));
        UNIT_TRY(hipStreamSynchronize(stream));
    }

done:
    return rc;
}

void sc_eval_release(void) { release_slots(g_slots); }

}  // extern "C"
