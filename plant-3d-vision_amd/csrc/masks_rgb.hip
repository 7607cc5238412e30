// masks_rgb.hip -- the geometric pipeline's mask producer on the GPU.
//
// Replaces the per-image chain of plant3dvision/tasks/proc2d.py::Masks.f (:224-249) over
// plant3dvision/proc2d.py (:69-220): float64 copy, rescale_intensity(out_range=(0, 1)), the `linear` or
// `excess_green` filter, `> threshold`, binary_dilation with disk(n, decomposition='sequence'), 255 * mask as
// uint8 -- for a batch of uint8 RGB pictures in HBM, every picture with its own range.
//
// Arithmetic is the reference's float64 operations in the reference's order:
//   * range: imin / imax over all three channels of a picture;  x' = (x - imin) / (imax - imin), or
//     min(x, 1.0) for a constant picture (the np.clip branch of skimage's rescale_intensity).  PARITY UNPINNED
//     (DESIGN.md 6): skimage is not available, this restates its source.
//   * linear (proc2d.py:115):  f = (c0 r' + c1 g') + c2 b'
//   * excess_green (proc2d.py:165-169):  s = ((r' + g') + b') + 1e-9;  f = ((2 (g'/s)) - (r'/s)) - (b'/s)
//   * dilation: 3x3 footprints one after the other, out[p] = OR_o in[p - o], outside the picture is background.
// Built with -ffp-contract=off like the rest (the v_fma_f64 in the ISA belong to the compiler's IEEE division).
//
// Four launches per call: range (min / max per picture), table (the 256 normalised values of every picture),
// filter (threshold -> 1 bit per pixel, a __ballot per 64 pixels of a row), dilate (the steps on 64-bit words in
// LDS, then 0 / 255 bytes).  Stand-alone unit: nothing shared with the carve's engine; the dilation of bit planes in
// LDS and the footprints are sc_bitplane.h, shared with evaluate.hip.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sc_bitplane.h"
#include "sc_unit.h"

namespace {

constexpr int kB = 256;

thread_local UnitError g_err;

// ---- range: least and greatest byte of each picture ------------------------------------------------------------
// work[v] = {255 - imin, imax}, zeroed before the launch: both are integer atomic maxima, one pair per block.
constexpr int kRangeBlocks = 64;  // blocks per picture at most (grid-stride inside)

__device__ __forceinline__ void fold4(uint32_t w, uint32_t &mn, uint32_t &mx) {
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t b = (w >> (8 * k)) & 255u;
        mn = min(mn, b);
        mx = max(mx, b);
    }
}

__global__ __launch_bounds__(kB) void masks_range_kernel(const uint8_t *__restrict__ rgb, int64_t n /* bytes per picture */,
                                                         int blocks_per_pic, uint32_t *__restrict__ work) {
    __shared__ uint32_t smn[kB / 64], smx[kB / 64];
    const int v = (int)(blockIdx.x / (uint32_t)blocks_per_pic), b = (int)(blockIdx.x % (uint32_t)blocks_per_pic);
    const uint8_t *p = rgb + (int64_t)v * n;
    const int64_t head = min(n, (int64_t)((16 - (reinterpret_cast<uintptr_t>(p) & 15)) & 15));
    const int64_t nvec = (n - head) / 16, tail0 = head + nvec * 16;
    const uint4 *q = reinterpret_cast<const uint4 *>(p + head);
    uint32_t mn = 255u, mx = 0u;
    for (int64_t i = (int64_t)b * kB + threadIdx.x; i < nvec; i += (int64_t)blocks_per_pic * kB) {
        const uint4 w = q[i];
        fold4(w.x, mn, mx);
        fold4(w.y, mn, mx);
        fold4(w.z, mn, mx);
        fold4(w.w, mn, mx);
    }
    if (b == 0) {  // the at most 15 + 15 bytes around the 16-byte body
        if ((int64_t)threadIdx.x < head) { const uint32_t x = p[threadIdx.x]; mn = min(mn, x); mx = max(mx, x); }
        if (tail0 + (int64_t)threadIdx.x < n) { const uint32_t x = p[tail0 + threadIdx.x]; mn = min(mn, x); mx = max(mx, x); }
    }
    for (int o = 32; o > 0; o >>= 1) {
        mn = min(mn, (uint32_t)__shfl_down(mn, o));
        mx = max(mx, (uint32_t)__shfl_down(mx, o));
    }
    if ((threadIdx.x & 63) == 0) { smn[threadIdx.x >> 6] = mn; smx[threadIdx.x >> 6] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kB / 64; ++w) { mn = min(mn, smn[w]); mx = max(mx, smx[w]); }
        atomicMax(&work[2 * v], 255u - mn);
        atomicMax(&work[2 * v + 1], mx);
    }
}

// ---- table: rescale_intensity's value of each of the 256 bytes, per picture ------------------------------------
__global__ __launch_bounds__(kB) void masks_table_kernel(const uint32_t *__restrict__ work, double *__restrict__ table,
                                                         int32_t *__restrict__ ranges) {
    const int v = (int)blockIdx.x;
    const int imin = 255 - (int)work[2 * v], imax = (int)work[2 * v + 1];
    const double x = (double)threadIdx.x;
    table[(int64_t)v * 256 + threadIdx.x] = imin != imax ? (x - (double)imin) / ((double)imax - (double)imin) : fmin(x, 1.0);
    if (threadIdx.x == 0) { ranges[2 * v] = imin; ranges[2 * v + 1] = imax; }
}

// ---- filter + threshold -> bits --------------------------------------------------------------------------------
// A segment is up to 256 consecutive pixels of one row (768 bytes): fetched with dword loads into LDS, one pixel
// per lane from there, one __ballot per wavefront = one 64-bit word of the row's bit mask (pixel x at bit x & 63 of
// word x >> 6; bits beyond W are 0).  A block takes kSegs consecutive segments of one picture.
constexpr int kSegs = 16;

struct FilterArgs {
    double c0, c1, c2, threshold;
    int filter;
};

template <int FILTER>
__global__ __launch_bounds__(kB) void masks_filter_kernel(const uint8_t *__restrict__ rgb, int64_t total_bytes, int H, int W,
                                                          int Wd, int segs_per_row, int64_t nseg, int blocks_per_pic,
                                                          const double *__restrict__ table, FilterArgs fa,
                                                          unsigned long long *__restrict__ bits) {
    __shared__ double tab[256];
    __shared__ uint32_t stage[2][kB * 3 / 4 + 4];
    const int v = (int)(blockIdx.x / (uint32_t)blocks_per_pic), b = (int)(blockIdx.x % (uint32_t)blocks_per_pic);
    tab[threadIdx.x] = table[(int64_t)v * 256 + threadIdx.x];
    const int64_t pic = (int64_t)v * 3 * H * W;
    const uintptr_t lo = reinterpret_cast<uintptr_t>(rgb), hi = lo + (uintptr_t)total_bytes;
    const int64_t s0 = (int64_t)b * kSegs, s1 = min(nseg, s0 + kSegs);
    for (int64_t s = s0; s < s1; ++s) {  // block-uniform
        const int y = (int)(s / segs_per_row), x0 = (int)(s % segs_per_row) * kB;
        const int npx = min(kB, W - x0);
        const uintptr_t p0 = lo + (uintptr_t)(pic + 3 * ((int64_t)y * W + x0));
        const uintptr_t pa = p0 & ~(uintptr_t)3;
        const int shift = (int)(p0 - pa), ndw = (shift + 3 * npx + 3) >> 2;  // <= 193
        uint32_t *st = stage[s & 1];
        if ((int)threadIdx.x < ndw) {
            const uintptr_t a = pa + 4u * threadIdx.x;
            uint32_t w = 0;
            if (a >= lo && a + 4 <= hi) {
                w = *reinterpret_cast<const uint32_t *>(a);
            } else {  // a word that straddles an end of the caller's buffer: its bytes inside only
                for (int k = 0; k < 4; ++k)
                    if (a + k >= lo && a + k < hi) w |= (uint32_t) * reinterpret_cast<const uint8_t *>(a + k) << (8 * k);
            }
            st[threadIdx.x] = w;
        }
        __syncthreads();  // (also orders tab[]; the buffer written next time was last read before this barrier)
        bool on = false;
        if ((int)threadIdx.x < npx) {
            const uint8_t *sb = reinterpret_cast<const uint8_t *>(st) + shift + 3 * threadIdx.x;
            const double r = tab[sb[0]], g = tab[sb[1]], bl = tab[sb[2]];
            double f;
            if (FILTER == SC_FILTER_LINEAR) {
                f = (fa.c0 * r + fa.c1 * g) + fa.c2 * bl;
            } else {
                const double sum = ((r + g) + bl) + 1e-9;
                f = ((2.0 * (g / sum)) - (r / sum)) - (bl / sum);
            }
            on = f > fa.threshold;
        }
        const unsigned long long word = __ballot(on);
        const int wx = (x0 >> 6) + (int)(threadIdx.x >> 6);
        if ((threadIdx.x & 63) == 0 && wx < Wd) bits[((int64_t)v * H + y) * Wd + wx] = word;
    }
}

// ---- dilate + expand -------------------------------------------------------------------------------------------
// The tiles of sc_bitplane.h with the call's table of footprints; the block writes its own part as bytes.
struct Steps {
    uint16_t foot[kMaxSteps];  // 9-bit sets (sc_bitplane.h)
    int n;
    __device__ uint32_t operator()(int k) const { return foot[k]; }
};

__device__ __forceinline__ uint32_t spread4(uint32_t b4) {  // 4 bits -> 4 bytes of 0 / 255
    return ((b4 * 0x00204081u) & 0x01010101u) * 0xffu;
}

__global__ __launch_bounds__(kB) void masks_dilate_kernel(const unsigned long long *__restrict__ bits, int H, int W, int Wd,
                                                          int tiles_x, int tiles_y, Steps steps, uint8_t *__restrict__ out) {
    __shared__ unsigned long long buf[2][kPlaneCells];
    const int n = steps.n;
    const uint32_t per_pic = (uint32_t)tiles_x * (uint32_t)tiles_y;
    const int v = (int)(blockIdx.x / per_pic), t = (int)(blockIdx.x % per_pic);
    const int ty = t / tiles_x, tx = t % tiles_x;
    const unsigned long long *res = buf[dilate_tile<kB>(buf, bits + (int64_t)v * H * Wd, H, W, Wd, ty, tx, n, steps)];
    // expand the block's own kTR x kTW words: 16 pixels per thread and turn
    uint8_t *dst = out + (int64_t)v * H * W;
    for (int c = threadIdx.x; c < kTR * kTW * 4; c += kB) {
        const int lr = c / (kTW * 4), q = c % (kTW * 4);
        const int y = ty * kTR + lr, x = (tx * kTW) * 64 + q * 16;
        if (y >= H || x >= W) continue;
        const uint32_t b16 = (uint32_t)(res[(lr + n) * kLW + 1 + (q >> 2)] >> (16 * (q & 3))) & 0xffffu;
        uint8_t *p = dst + (int64_t)y * W + x;
        if (x + 16 <= W && (reinterpret_cast<uintptr_t>(p) & 15) == 0) {
            *reinterpret_cast<uint4 *>(p) = make_uint4(spread4(b16 & 15u), spread4((b16 >> 4) & 15u),
                                                       spread4((b16 >> 8) & 15u), spread4(b16 >> 12));
        } else {
            const int m = min(16, W - x);
            for (int e = 0; e < m; ++e) p[e] = (uint8_t)(((b16 >> e) & 1u) ? 255 : 0);
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------
// Work buffers (bits, tables, ranges) are kept per device: the slot protocol of sc_unit.h.
WorkSlot g_slots[kUnitDevices];

}  // namespace

extern "C" {

const char *sc_masks_last_error(void) { return g_err.msg; }

int sc_masks_from_rgb(const void *rgb, int rgb_on_device, int V, int H, int W, int filter, const double coefs[3],
                      double threshold, const uint8_t *steps, int nsteps, int device, void *hip_stream,
                      void *masks_out, int out_on_device, int32_t *ranges_out) {
    // every argument is judged before the first device call
    if (!rgb || !masks_out || !coefs) return g_err.fail(SC_ERR_INVALID, "null argument (rgb, coefs, masks_out)");
    if (V < 1 || H < 1 || W < 1) return g_err.fail(SC_ERR_INVALID, "V, H and W must be at least 1");
    if ((int64_t)3 * H * W >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "picture too large: 3 * H * W must be below 2^31");
    if (filter != SC_FILTER_LINEAR && filter != SC_FILTER_EXCESS_GREEN)
        return g_err.fail(SC_ERR_INVALID, "filter: 0 linear, 1 excess_green");
    if (!std::isfinite(coefs[0]) || !std::isfinite(coefs[1]) || !std::isfinite(coefs[2]))
        return g_err.fail(SC_ERR_INVALID, "coefficients must be finite");
    if (!std::isfinite(threshold)) return g_err.fail(SC_ERR_INVALID, "threshold must be finite");
    if (nsteps < 0 || nsteps > kMaxSteps) return g_err.fail(SC_ERR_INVALID, "nsteps must be 0..32");
    if (nsteps > 0 && !steps) return g_err.fail(SC_ERR_INVALID, "null argument (steps)");
    Steps st;
    memset(&st, 0, sizeof st);
    st.n = nsteps;
    for (int k = 0; k < nsteps; ++k) {
        if (steps[k] > SC_FOOT_SQUARE) return g_err.fail(SC_ERR_INVALID, "step ids are 0..5 (SC_FOOT_*)");
        st.foot[k] = kFoot[steps[k]];
    }
    if (device < 0 || device >= kUnitDevices) return g_err.fail(SC_ERR_INVALID, "device ordinal out of range");
    const int64_t npix = (int64_t)H * W, nbytes = 3 * npix;
    const int Wd = (W + 63) / 64;
    const int segs_per_row = (W + kB - 1) / kB;
    const int64_t nseg = (int64_t)H * segs_per_row;
    const int64_t fblocks = (nseg + kSegs - 1) / kSegs;
    const int64_t rblocks = std::min<int64_t>(kRangeBlocks, (nbytes / 16 + kB * 4 - 1) / (kB * 4) + 1);
    const int tiles_x = (Wd + kTW - 1) / kTW, tiles_y = (H + kTR - 1) / kTR;
    if (fblocks * V > 0x7fffffffLL || (int64_t)tiles_x * tiles_y * V > 0x7fffffffLL)
        return g_err.fail(SC_ERR_INVALID, "batch too large for one launch: split it");

    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    uint8_t *rgb_d = nullptr, *out_d = nullptr;  // staging of host pointers (this call's own)
    Layout lay;
    const size_t o_work = lay.take((size_t)V * 8), o_rng = lay.take((size_t)V * 8), o_tab = lay.take((size_t)V * 2048),
                 o_bits = lay.take((size_t)V * H * Wd * 8);
    uint32_t *work;
    int32_t *ranges;
    double *table;
    unsigned long long *bits;
    FilterArgs fa{coefs[0], coefs[1], coefs[2], threshold, filter};
    call.sync_failures = !rgb_on_device || !out_on_device;  // nothing of ours may still use the staging buffers

    if ((rc = call.open(lay.total)) != SC_OK) goto done;
    work = reinterpret_cast<uint32_t *>(call.sl.base + o_work);
    ranges = reinterpret_cast<int32_t *>(call.sl.base + o_rng);
    table = reinterpret_cast<double *>(call.sl.base + o_tab);
    bits = reinterpret_cast<unsigned long long *>(call.sl.base + o_bits);
    if (rgb_on_device) {
        rgb_d = static_cast<uint8_t *>(const_cast<void *>(rgb));
    } else {
        UNIT_TRY(hipMalloc(reinterpret_cast<void **>(&rgb_d), (size_t)V * nbytes));
        UNIT_TRY(hipMemcpyAsync(rgb_d, rgb, (size_t)V * nbytes, hipMemcpyHostToDevice, stream));
    }
    if (out_on_device) {
        out_d = static_cast<uint8_t *>(masks_out);
    } else {
        UNIT_TRY(hipMalloc(reinterpret_cast<void **>(&out_d), (size_t)V * npix));
    }
    UNIT_TRY(call.sl.wait(stream));
    UNIT_TRY(hipMemsetAsync(work, 0, (size_t)V * 8, stream));
    hipLaunchKernelGGL(masks_range_kernel, dim3((uint32_t)(rblocks * V)), dim3(kB), 0, stream, rgb_d, nbytes, (int)rblocks, work);
    hipLaunchKernelGGL(masks_table_kernel, dim3((uint32_t)V), dim3(kB), 0, stream, work, table, ranges);
    if (filter == SC_FILTER_LINEAR)
        hipLaunchKernelGGL(masks_filter_kernel<SC_FILTER_LINEAR>, dim3((uint32_t)(fblocks * V)), dim3(kB), 0, stream, rgb_d,
                           (int64_t)V * nbytes, H, W, Wd, segs_per_row, nseg, (int)fblocks, table, fa, bits);
    else
        hipLaunchKernelGGL(masks_filter_kernel<SC_FILTER_EXCESS_GREEN>, dim3((uint32_t)(fblocks * V)), dim3(kB), 0, stream, rgb_d,
                           (int64_t)V * nbytes, H, W, Wd, segs_per_row, nseg, (int)fblocks, table, fa, bits);
    hipLaunchKernelGGL(masks_dilate_kernel, dim3((uint32_t)((int64_t)tiles_x * tiles_y * V)), dim3(kB), 0, stream, bits, H, W, Wd,
                       tiles_x, tiles_y, st, out_d);
    UNIT_TRY(hipGetLastError());
    if (ranges_out) UNIT_TRY(hipMemcpyAsync(ranges_out, ranges, (size_t)V * 8, hipMemcpyDeviceToHost, stream));
    if (!out_on_device) UNIT_TRY(hipMemcpyAsync(masks_out, out_d, (size_t)V * npix, hipMemcpyDeviceToHost, stream));
    UNIT_TRY(call.sl.record(stream));
    if (ranges_out || !out_on_device || !rgb_on_device) UNIT_TRY(hipStreamSynchronize(stream));

done:
    call.settle();
    if (!rgb_on_device && rgb_d) (void)hipFree(rgb_d);
    if (!out_on_device && out_d) (void)hipFree(out_d);
    return rc;
}

void sc_masks_release(void) { release_slots(g_slots); }

}  // extern "C"
