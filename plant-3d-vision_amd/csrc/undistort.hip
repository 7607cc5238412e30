// undistort.hip -- the geometric pipeline's lens correction on the GPU.
//
// Replaces plant3dvision/tasks/proc2d.py::Undistorted.f (:120-143) over plant3dvision/proc2d.py::undistort (:25-66),
// which is cv2.undistort(img, A, dist, None), for a batch of uint8 RGB pictures of one camera in HBM.
//
// PARITY UNPINNED: OpenCV is not available, this restates its published algorithm --
// initUndistortRectifyMap with identity rectification and newCameraMatrix = A, map type CV_16SC2, INTER_BITS = 5, then
// remap(INTER_LINEAR, BORDER_CONSTANT 0) on 8-bit pixels with 15-bit weights.  Per output pixel (row i, column j), every
// operation IEEE binary64, one rounding each, in the order written (built with -ffp-contract=off like the rest):
//   x = (j - cx) / fx   y = (i - cy) / fy   x2 = x*x   y2 = y*y   r2 = x2 + y2   _2xy = (2*x)*y
//   kr = 1 + ((k3*r2 + k2)*r2 + k1)*r2
//   xd = (x*kr + p1*_2xy) + p2*(r2 + 2*x2)      yd = (y*kr + p1*(r2 + 2*y2)) + p2*_2xy
//   u = fx*xd + cx   v = fy*yd + cy   iu = rint(32*u)   iv = rint(32*v)        (round half to even)
// unmapped (u or v not finite, |iu| or |iv| >= 2^30): output 0, map entry (INT32_MIN, INT32_MIN).  Else sx = iu >> 5,
// sy = iv >> 5, a = iu & 31, b = iv & 31 and per channel, a tap outside the picture counting 0,
//   S = (32-a)(32-b) p(sy,sx) + a(32-b) p(sy,sx+1) + (32-a)b p(sy+1,sx) + ab p(sy+1,sx+1)      out = (S + 512) >> 10
// which is OpenCV's (sum w p + 2^14) >> 15 with w = 32 (..)(..).  Two deviations from OpenCV: the ray is evaluated
// directly per pixel (OpenCV: running sums along a row), and sx / sy beyond +-32768 lie outside (OpenCV: a (short) wrap).
//
// Two launches per call: map (the binary64 chain once per pixel -> (iu, iv), 8 bytes per pixel, which stay in the
// caches) and remap (a lane takes 4 neighbouring pixels of a row, keeps their map entries in registers and walks up to
// kPics pictures with them).  Stand-alone unit on the scaffold of sc_unit.h.

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sc_unit.h"

namespace {

constexpr int kB = 256;
constexpr int kPx = 4;    // pixels of one row per lane: 12 bytes of output
constexpr int kPics = 8;  // pictures a lane walks with one set of map entries

thread_local UnitError g_err;

struct Camera {
    double fx, fy, cx, cy, k1, k2, p1, p2, k3;
};

// ---- map: (iu, iv) of every pixel --------------------------------------------------------------------------------
__global__ __launch_bounds__(kB) void undistort_map_kernel(int H, int W, Camera c, int2 *__restrict__ map) {
    const int64_t q = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (q >= (int64_t)H * W) return;
    const int i = (int)(q / W), j = (int)(q - (int64_t)i * W);
    const double x = ((double)j - c.cx) / c.fx, y = ((double)i - c.cy) / c.fy;
    const double x2 = x * x, y2 = y * y, r2 = x2 + y2, _2xy = (2.0 * x) * y;
    const double kr = 1.0 + ((c.k3 * r2 + c.k2) * r2 + c.k1) * r2;
    const double xd = (x * kr + c.p1 * _2xy) + c.p2 * (r2 + 2.0 * x2);
    const double yd = (y * kr + c.p1 * (r2 + 2.0 * y2)) + c.p2 * _2xy;
    const double u = c.fx * xd + c.cx, v = c.fy * yd + c.cy;
    const double fu = rint(32.0 * u), fv = rint(32.0 * v);
    const bool mapped = isfinite(u) && isfinite(v) && fabs(fu) < 1073741824.0 && fabs(fv) < 1073741824.0;
    map[q] = mapped ? make_int2((int)fu, (int)fv) : make_int2(INT32_MIN, INT32_MIN);
}

// ---- remap -------------------------------------------------------------------------------------------------------
// What a lane keeps of one pixel's map entry.  off >= 0: all four taps lie inside the picture and the 8 bytes at `off`
// and at `off + 3 W` (two pixels of 3 bytes and 2 more) lie inside it as well: two 8-byte loads.  off < 0: the taps
// one by one (edge()), each read only if its weight is not 0 and it lies inside.
struct Entry {
    int off;          // 3 (sy W + sx), or -1
    int sx, sy;       // used by edge() only
    uint32_t w[4];    // (32-a)(32-b), a(32-b), (32-a)b, ab
};

__device__ __forceinline__ Entry make_entry(int2 m, int H, int W) {
    Entry e;
    e.sx = m.x >> 5;
    e.sy = m.y >> 5;
    const uint32_t a = (uint32_t)m.x & 31u, b = (uint32_t)m.y & 31u;
    e.w[0] = (32u - a) * (32u - b);
    e.w[1] = a * (32u - b);
    e.w[2] = (32u - a) * b;
    e.w[3] = a * b;
    const bool inside = e.sx >= 0 && e.sx + 1 < W && e.sy >= 0 && e.sy + 1 < H;
    const int64_t off = 3 * ((int64_t)e.sy * W + e.sx);
    e.off = inside && off + 3 * (int64_t)W + 8 <= 3 * (int64_t)H * W ? (int)off : -1;
    return e;
}

__device__ __forceinline__ uint64_t load8(const uint8_t *p) {  // no alignment: the target reads unaligned words
    uint64_t w;
    __builtin_memcpy(&w, p, 8);
    return w;
}

__device__ __forceinline__ uint32_t blend(const Entry &e, uint64_t top, uint64_t bot, int ch) {
    const uint32_t s = e.w[0] * (uint32_t)((top >> (8 * ch)) & 255u) + e.w[1] * (uint32_t)((top >> (8 * ch + 24)) & 255u) +
                       e.w[2] * (uint32_t)((bot >> (8 * ch)) & 255u) + e.w[3] * (uint32_t)((bot >> (8 * ch + 24)) & 255u);
    return (s + 512u) >> 10;
}

// A pixel with a tap outside the picture (or in the picture's last bytes): 0 for what lies outside, and no read of a
// tap whose weight is 0.  An unmapped pixel has sx = sy = -2^26: nothing inside.
__device__ __forceinline__ uint32_t edge(const Entry &e, const uint8_t *__restrict__ pic, int H, int W) {
    uint32_t s[3] = {0u, 0u, 0u};
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int xx = e.sx + (t & 1), yy = e.sy + (t >> 1);
        if (e.w[t] != 0u && xx >= 0 && xx < W && yy >= 0 && yy < H) {
            const uint8_t *p = pic + 3 * ((int64_t)yy * W + xx);
            s[0] += e.w[t] * p[0];
            s[1] += e.w[t] * p[1];
            s[2] += e.w[t] * p[2];
        }
    }
    return ((s[0] + 512u) >> 10) | (((s[1] + 512u) >> 10) << 8) | (((s[2] + 512u) >> 10) << 16);
}

// Block b of a chunk takes the pixel groups b kB .. of the picture (a group: kPx pixels of one row, the last of a row
// may be short); chunk c takes the pictures c kPics ...  Blocks of one chunk follow one another.
__global__ __launch_bounds__(kB) void undistort_remap_kernel(const uint8_t *__restrict__ rgb, uint8_t *__restrict__ out, int V, int H,
                                                             int W, int groups_per_row, int64_t ngroups, uint32_t blocks_per_chunk,
                                                             const int2 *__restrict__ map) {
    const uint32_t chunk = blockIdx.x / blocks_per_chunk, b = blockIdx.x % blocks_per_chunk;
    const int64_t g = (int64_t)b * kB + threadIdx.x;
    if (g >= ngroups) return;
    const int y = (int)(g / groups_per_row), x0 = (int)(g - (int64_t)y * groups_per_row) * kPx;
    const int npx = min(kPx, W - x0);
    const int64_t pix0 = (int64_t)y * W + x0, nbytes = 3 * (int64_t)H * W;
    Entry e[kPx];
    bool fast = npx == kPx;
#pragma unroll
    for (int k = 0; k < kPx; ++k) {
        e[k] = make_entry(k < npx ? map[pix0 + k] : make_int2(INT32_MIN, INT32_MIN), H, W);
        fast = fast && e[k].off >= 0;
    }
    const int v0 = (int)chunk * kPics, v1 = min(V, v0 + kPics);
    const int64_t row = 3 * (int64_t)W;
    if (fast) {  // most lanes of most pictures: 8 loads of 8 bytes and one store of 12 per picture
        for (int v = v0; v < v1; ++v) {
            const uint8_t *pic = rgb + (int64_t)v * nbytes;
            uint64_t top[kPx], bot[kPx];
#pragma unroll
            for (int k = 0; k < kPx; ++k) {
                top[k] = load8(pic + e[k].off);
                bot[k] = load8(pic + e[k].off + row);
            }
            uint32_t px[kPx];
#pragma unroll
            for (int k = 0; k < kPx; ++k)
                px[k] = blend(e[k], top[k], bot[k], 0) | (blend(e[k], top[k], bot[k], 1) << 8) | (blend(e[k], top[k], bot[k], 2) << 16);
            const uint32_t w3[3] = {px[0] | (px[1] << 24), (px[1] >> 8) | (px[2] << 16), (px[2] >> 16) | (px[3] << 8)};
            __builtin_memcpy(out + (int64_t)v * nbytes + 3 * pix0, w3, 12);
        }
        return;
    }
    for (int v = v0; v < v1; ++v) {
        const uint8_t *pic = rgb + (int64_t)v * nbytes;
        uint8_t *dst = out + (int64_t)v * nbytes + 3 * pix0;
#pragma unroll
        for (int k = 0; k < kPx; ++k) {  // (unrolled: e[] stays in registers)
            if (k >= npx) break;
            uint32_t px;
            if (e[k].off >= 0) {
                const uint64_t top = load8(pic + e[k].off), bot = load8(pic + e[k].off + row);
                px = blend(e[k], top, bot, 0) | (blend(e[k], top, bot, 1) << 8) | (blend(e[k], top, bot, 2) << 16);
            } else {
                px = edge(e[k], pic, H, W);
            }
            dst[3 * k] = (uint8_t)px;
            dst[3 * k + 1] = (uint8_t)(px >> 8);
            dst[3 * k + 2] = (uint8_t)(px >> 16);
        }
    }
}

// ---- host side -------------------------------------------------------------------------------------------------
// The work buffer (the map) is kept per device: the slot protocol of sc_unit.h.
WorkSlot g_slots[kUnitDevices];

}  // namespace

extern "C" {

const char *sc_undistort_last_error(void) { return g_err.msg; }

int sc_undistort_rgb(const void *rgb, int rgb_on_device, int V, int H, int W, const double K[4], const double dist[5],
                     int device, void *hip_stream, void *rgb_out, int out_on_device, int32_t *map_out) {
    // every argument is judged before the first device call
    if (!rgb || !rgb_out || !K || !dist) return g_err.fail(SC_ERR_INVALID, "null argument (rgb, K, dist, rgb_out)");
    if (V < 1 || H < 1 || W < 1) return g_err.fail(SC_ERR_INVALID, "V, H and W must be at least 1");
    if ((int64_t)3 * H * W >= ((int64_t)1 << 31)) return g_err.fail(SC_ERR_INVALID, "picture too large: 3 * H * W must be below 2^31");
    for (int k = 0; k < 4; ++k)
        if (!std::isfinite(K[k])) return g_err.fail(SC_ERR_INVALID, "camera matrix entries must be finite");
    for (int k = 0; k < 5; ++k)
        if (!std::isfinite(dist[k])) return g_err.fail(SC_ERR_INVALID, "distortion coefficients must be finite");
    if (K[0] == 0.0 || K[1] == 0.0) return g_err.fail(SC_ERR_INVALID, "focal lengths fx and fy must not be zero");
    const int64_t npix = (int64_t)H * W, nbytes = 3 * npix;
    {
        const uintptr_t a = reinterpret_cast<uintptr_t>(rgb), b = reinterpret_cast<uintptr_t>(rgb_out);
        const uintptr_t n = (uintptr_t)V * (uintptr_t)nbytes;
        if (a < b + n && b < a + n) return g_err.fail(SC_ERR_INVALID, "rgb and rgb_out overlap");
    }
    if (device < 0 || device >= kUnitDevices) return g_err.fail(SC_ERR_INVALID, "device ordinal out of range");
    const int groups_per_row = (W + kPx - 1) / kPx;
    const int64_t ngroups = (int64_t)H * groups_per_row;
    const int64_t rblocks = (ngroups + kB - 1) / kB, chunks = ((int64_t)V + kPics - 1) / kPics, mblocks = (npix + kB - 1) / kB;
    if (rblocks * chunks > 0x7fffffffLL) return g_err.fail(SC_ERR_INVALID, "batch too large for one launch: split it");

    int rc = SC_OK;
    hipStream_t stream = static_cast<hipStream_t>(hip_stream);
    UnitCall call(g_err, g_slots, device, stream, rc);
    uint8_t *rgb_d = nullptr, *out_d = nullptr;  // staging of host pointers (this call's own)
    Layout lay;
    const size_t o_map = lay.take((size_t)npix * sizeof(int2));
    int2 *map;
    const Camera cam{K[0], K[1], K[2], K[3], dist[0], dist[1], dist[2], dist[3], dist[4]};
    call.sync_failures = !rgb_on_device || !out_on_device;  // nothing of ours may still use the staging buffers

    if ((rc = call.open(lay.total)) != SC_OK) goto done;
    map = reinterpret_cast<int2 *>(call.sl.base + o_map);
    if (rgb_on_device) {
        rgb_d = static_cast<uint8_t *>(const_cast<void *>(rgb));
    } else {
        UNIT_TRY(hipMalloc(reinterpret_cast<void **>(&rgb_d), (size_t)V * nbytes));
        UNIT_TRY(hipMemcpyAsync(rgb_d, rgb, (size_t)V * nbytes, hipMemcpyHostToDevice, stream));
    }
    if (out_on_device) {
        out_d = static_cast<uint8_t *>(rgb_out);
    } else {
        UNIT_TRY(hipMalloc(reinterpret_cast<void **>(&out_d), (size_t)V * nbytes));
    }
    UNIT_TRY(call.sl.wait(stream));
    hipLaunchKernelGGL(undistort_map_kernel, dim3((uint32_t)mblocks), dim3(kB), 0, stream, H, W, cam, map);
    hipLaunchKernelGGL(undistort_remap_kernel, dim3((uint32_t)(rblocks * chunks)), dim3(kB), 0, stream, rgb_d, out_d, V, H, W,
                       groups_per_row, ngroups, (uint32_t)rblocks, map);
    UNIT_TRY(hipGetLastError());
    if (map_out) UNIT_TRY(hipMemcpyAsync(map_out, map, (size_t)npix * sizeof(int2), hipMemcpyDeviceToHost, stream));
    if (!out_on_device) UNIT_TRY(hipMemcpyAsync(rgb_out, out_d, (size_t)V * nbytes, hipMemcpyDeviceToHost, stream));
    UNIT_TRY(call.sl.record(stream));
    if (map_out || !out_on_device || !rgb_on_device) UNIT_TRY(hipStreamSynchronize(stream));

done:
    call.settle();
    if (!rgb_on_device && rgb_d) (void)hipFree(rgb_d);
    if (!out_on_device && out_d) (void)hipFree(out_d);
    return rc;
}

void sc_undistort_release(void) { release_slots(g_slots); }

}  // extern "C"
