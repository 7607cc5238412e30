// sc_bitplane.h -- dilation of pictures kept as bit planes, on tiles in LDS: shared by masks_rgb.hip (any 3x3
// footprint per step, bytes out) and evaluate.hip (the cross, words out).  Internal linkage like sc_unit.h.
//
// A bit plane has 1 bit per pixel in 64-bit words, Wd = (W + 63) / 64 of them per row: pixel x at bit x & 63 of word
// x >> 6, bits beyond W are 0.  A block owns kTR rows x kTW words (512 pixels) of one picture.  It loads them with a
// halo of n rows above and below and one word left and right (n <= kMaxSteps = 32 < 64 bits), runs the n steps on
// the words in LDS (ping-pong) and writes its own part itself.  What is wrong at the rim of the halo after k steps
// has moved k pixels inward: never into the block's own part.  Pixels outside the picture are background after every
// step.  A step is out[p] = OR over the offsets o of its footprint of in[p - o].
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace {

constexpr int kMaxSteps = 32;  // steps per launch
constexpr int kTR = 32, kTW = 8, kLW = kTW + 2;
constexpr int kPlaneCells = (kTR + 2 * kMaxSteps) * kLW;  // a kernel declares `__shared__ unsigned long long buf[2][kPlaneCells]`

// A footprint is a 9-bit set: bit (dy + 1) * 3 + (dx + 1) = it holds offset (dy, dx).  The six of masks2d._FOOTPRINTS,
// indexed by SC_FOOT_*:
constexpr uint16_t fbit(int dy, int dx) { return (uint16_t)(1u << ((dy + 1) * 3 + (dx + 1))); }
constexpr uint16_t kDiamond = fbit(-1, 0) | fbit(0, -1) | fbit(0, 0) | fbit(0, 1) | fbit(1, 0);  // the 4-connected cross
const uint16_t kFoot[6] = {
    (uint16_t)(fbit(-1, -1) | fbit(-1, 0) | fbit(-1, 1) | fbit(0, 0) | fbit(1, 0)),   // t0
    (uint16_t)(fbit(1, -1) | fbit(0, -1) | fbit(-1, -1) | fbit(0, 0) | fbit(0, 1)),   // t90
    (uint16_t)(fbit(1, 1) | fbit(1, 0) | fbit(1, -1) | fbit(0, 0) | fbit(-1, 0)),     // t180
    (uint16_t)(fbit(-1, 1) | fbit(0, 1) | fbit(1, 1) | fbit(0, 0) | fbit(0, -1)),     // t270
    kDiamond,
    (uint16_t)0x1ff,                                                                  // square
};

// Tile (ty, tx) of the plane `src` (one picture, H rows of Wd words): loads it with its halo into buf[0], runs steps
// 0 .. n - 1 and returns which of buf[0], buf[1] holds the result; the tile's word (lr, lw) is cell
// (lr + n) * kLW + 1 + lw of it.  foot(k) is the footprint of step k: a functor, so that a constant one folds.
// For all kB threads of the block; ends behind a barrier.
template <int kB, class Foot>
__device__ __forceinline__ int dilate_tile(unsigned long long (*buf)[kPlaneCells], const unsigned long long *__restrict__ src, int H,
                                           int W, int Wd, int ty, int tx, int n, const Foot &foot) {
    const int r0 = ty * kTR - n, w0 = tx * kTW - 1;  // picture row / word of LDS cell (0, 0)
    const int LR = kTR + 2 * n, cells = LR * kLW;
    const unsigned long long last_mask = (W & 63) ? (~0ull >> (64 - (W & 63))) : ~0ull;
    for (int c = threadIdx.x; c < cells; c += kB) {
        const int y = r0 + c / kLW, w = w0 + c % kLW;
        buf[0][c] = (y >= 0 && y < H && w >= 0 && w < Wd) ? src[(int64_t)y * Wd + w] : 0ull;
    }
    __syncthreads();
    int cur = 0;
    for (int k = 0; k < n; ++k) {
        const uint32_t fp = foot(k);
        const unsigned long long *in = buf[cur];
        unsigned long long *o = buf[cur ^ 1];
        for (int c = threadIdx.x; c < cells; c += kB) {
            const int lr = c / kLW, lw = c % kLW;
            const int y = r0 + lr, w = w0 + lw;
            unsigned long long acc = 0ull;
            if (y >= 0 && y < H && w >= 0 && w < Wd) {
#pragma unroll
                for (int i = 0; i < 3; ++i) {
                    // The cell's own row, the row above, the row below: a deliberate order, not a loop to tidy into
                    // -1, 0, +1.  It is the order of eval_dilate_kernel's cross before the units shared this step; in
                    // it the constant diamond folds to that kernel's old VGPRs and occupancy (tools/kernel_resources.sh).
                    const int dy = i == 0 ? 0 : i == 1 ? 1 : -1;
                    const uint32_t f3 = (fp >> ((dy + 1) * 3)) & 7u;  // bit 0: dx = -1, bit 1: dx = 0, bit 2: dx = +1
                    // out[p] |= in[p - o]: LDS row lr - dy, which only the first and the last row lack
                    if (f3 == 0u || (dy > 0 && lr == 0) || (dy < 0 && lr == LR - 1)) continue;
                    const unsigned long long *row = in + (c - dy * kLW);  // cell (lr - dy, lw)
                    const unsigned long long m = row[0];
                    const unsigned long long l = lw > 0 ? row[-1] : 0ull, r = lw < kLW - 1 ? row[1] : 0ull;
                    if (f3 & 1u) acc |= (m >> 1) | (r << 63);  // dx = -1: in[x + 1]
                    if (f3 & 2u) acc |= m;
                    if (f3 & 4u) acc |= (m << 1) | (l >> 63);  // dx = +1: in[x - 1]
                }
                if (w == Wd - 1) acc &= last_mask;
            }
            o[c] = acc;
        }
        __syncthreads();
        cur ^= 1;
    }
    return cur;
}

}  // namespace
