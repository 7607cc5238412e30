// vol2pcd.hip -- the carve's immediate consumer on the GPU.
//
// Replaces plant3dvision/proc3d.py::vol2pcd (:490-570), which tasks/proc3d.py:134 calls on the
// Voxels output: binarise (> 0.5), two exact Euclidean distance transforms, signed distance,
// np.gradient, three Gaussian filters (sigma 1), pick the voxels of the level-set shell and
// move each along its normalised gradient.  Running it here means the 4N-byte volume never
// has to cross PCIe: only the shell's points and normals come back.
//
// Arithmetic follows the reference's float64 operations and their order:
//   * EDT: squared distances are integers, sqrt is correctly rounded -> identical to
//     scipy.ndimage.distance_transform_edt.  Only voxels within RADIUS of the surface can
//     influence the output (shell |d| <= lsv + sqrt(3); gradient reach 1 + Gaussian reach 4 per
//     axis), so the transform is exact up to RADIUS and clamped beyond ("far", never used).
//   * np.gradient (unit spacing, edge_order 1): (f[i+1]-f[i-1])/2 inside, one-sided at the ends.
//   * scipy.ndimage.gaussian_filter(sigma=1): radius 4, mode "reflect", axes 0,1,2 in turn,
//     and scipy's symmetric correlate1d order  tmp = f[l]*w0; for j=4..1: tmp += (f[l-j]+f[l+j])*wj
//     (reproduces scipy 1.15 bit for bit; weights are computed by the host with NumPy).
//   * per point: n = g/|g|, p = idx - n*(d + lsv - sqrt(3)/2), normal = -n; the reference takes
//     |g| from BLAS (np.linalg.norm) and open3d renormalises, so the last bits of points and
//     normals are machine-dependent there; here |g| = sqrt((gx*gx+gy*gy)+gz*gz).
// Built with -ffp-contract=off like the rest.

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <vector>

#include "sc_unit.h"

namespace {

constexpr int kB = 256;
constexpr uint32_t kFar = 0xffffu;
constexpr int kBlk = 8;  // activity is tracked per 8x8x8 block of voxels

thread_local UnitError g_err;

// The work buffers (49 bytes per voxel) are kept between calls while they are small (up to 1 GiB: volumes up to
// ~280^3) -- allocating and freeing them was 2.8 of a call's 4.6 ms -- one per device, handed to one caller at a time
// (a second caller on the device takes its own, freed when its call ends); sc_vol2pcd_release() gives them back.
// Larger ones go back when the call ends: 6.6 GB at 512^3 and 52 GB at 1024^3 are HBM that later engines, survivor
// lists and two-engine runs need -- against 1 ms of a 4.6 ms call saved by keeping them.  (Not sc_unit.h's WorkSlot, on
// purpose: that one serialises its callers and orders them by an event on their streams; this unit stays on the null
// stream, waits for the device before a call ends, and lets a second caller work beside the first.)
struct ScratchSlot {
    char *base = nullptr; size_t cap = 0; bool busy = false;
    void drop() { if (base) (void)hipFree(base); base = nullptr; cap = 0; }
};
std::mutex g_scratch_mu;
ScratchSlot g_scratch[kUnitDevices];
constexpr size_t kScratchKeepMax = (size_t)1 << 30;

// What one call holds on the device: the work buffers (the device's slot if it is free, else its own allocation), the
// staged copy of a host volume, the points.  The end of the scope WAITS for the device, then frees or gives back.
struct Held {
    char *work = nullptr;
    ScratchSlot *slot = nullptr;  // the device's, where `work` is its cached buffer
    void *staged = nullptr, *points = nullptr;

    bool take_work(int device, size_t bytes) {
        if (device >= 0 && device < kUnitDevices) {
            std::lock_guard<std::mutex> lock(g_scratch_mu);
            ScratchSlot &sl = g_scratch[device];
            if (!sl.busy) {
                if (sl.cap < bytes) {
                    sl.drop();
                    char *p = nullptr;
                    if (hipMalloc(reinterpret_cast<void **>(&p), bytes) != hipSuccess) return false;
                    sl.base = p;
                    sl.cap = bytes;
                }
                sl.busy = true;
                slot = &sl;
                work = sl.base;
                return true;
            }
        }
        return hipMalloc(reinterpret_cast<void **>(&work), bytes) == hipSuccess;
    }
    ~Held() {
        (void)hipDeviceSynchronize();
        if (staged) (void)hipFree(staged);
        if (points) (void)hipFree(points);
        if (work && !slot) (void)hipFree(work);
        if (!slot) return;
        std::lock_guard<std::mutex> lock(g_scratch_mu);
        slot->busy = false;
        if (slot->cap > kScratchKeepMax) slot->drop();
    }
};

// Where a Held owns what is allocated, a failed runtime call is the function's result.
#define HIP_TRY(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return g_err.hip(_e); } while (0)

// Geometry shared by the per-voxel kernels.  They run on the ACTIVE 8^3 blocks only (a list built
// on the device: a few per cent of a plant's volume): thread block b takes list entry b, thread t
// the voxels t and t + 256 of its 512.
struct Vol {
    int nx, ny, nz;          // the planes at hand: the whole volume, or a slab of it with its halo
    int nby, nbz;            // blocks along y and z
    const uint8_t *active;   // [nbx][nby][nbz], 1 = within reach of the surface
    const uint32_t *list;    // linear ids of the blocks a kernel walks (active, or halo)
    const uint32_t *cols;    // columns of blocks (bx * nby + by) holding an active block (shell kernels)
    int xoff;                // plane 0 at hand is plane xoff of the volume (a point's x index is the volume's)
    int cx0, cx1;            // only shell voxels of planes [cx0, cx1) at hand are put out (the slab without its halo)
};

// linear block id -> block coordinates, in I's arithmetic (the lists hold 32-bit ids, the block maps are walked in 64)
struct Blk { int z, y, x; };
template <typename I>
__device__ __forceinline__ Blk block_split(I b, I nby, I nbz) {
    return Blk{(int)(b % nbz), (int)((b / nbz) % nby), (int)(b / (nbz * nby))};
}

// OR of a block map over the blocks within rb of block k, clipped to the map
__device__ __forceinline__ uint32_t near_or(const uint8_t *__restrict__ map, Blk k, int rb, int nbx, int nby, int nbz) {
    uint32_t near = 0;
    for (int x = max(0, k.x - rb); x <= min(nbx - 1, k.x + rb); ++x)
        for (int y = max(0, k.y - rb); y <= min(nby - 1, k.y + rb); ++y)
            for (int z = max(0, k.z - rb); z <= min(nbz - 1, k.z + rb); ++z)
                near |= map[((int64_t)x * nby + y) * nbz + z];
    return near;
}

// list[*count ...] takes `value` of the lanes with `mine`, in lane order: one atomic per wavefront; all lanes call it
__device__ __forceinline__ void wave_append(bool mine, uint32_t value, uint32_t *__restrict__ list,
                                            uint32_t *__restrict__ count) {
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(mine), below = lane ? (~0ull >> (64 - lane)) : 0ull;
    uint32_t base = 0;
    if (lane == 0 && m) base = atomicAdd(count, (uint32_t)__popcll(m));
    base = __shfl(base, 0);
    if (mine) list[base + (uint32_t)__popcll(m & below)] = value;
}

// Sum over the 256 threads of a block through s[kB / 64] in LDS; every thread calls it (one barrier) and gets the sum.
template <typename T>
__device__ __forceinline__ T block_sum(T mine, T *s) {
    for (int o = 32; o > 0; o >>= 1) mine += __shfl_down(mine, o);
    if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = mine;
    __syncthreads();
    return s[0] + s[1] + s[2] + s[3];
}

__device__ __forceinline__ bool voxel(const Vol &v, int q, int &x, int &y, int &z, int64_t &i) {
    const Blk k = block_split<uint32_t>(v.list[blockIdx.x], v.nby, v.nbz);
    const int l = (int)threadIdx.x + q * kB;  // 0..511: dx = l >> 6, dy = (l >> 3) & 7, dz = l & 7
    x = k.x * kBlk + (l >> 6);
    y = k.y * kBlk + ((l >> 3) & 7);
    z = k.z * kBlk + (l & 7);
    if (x >= v.nx || y >= v.ny || z >= v.nz) return false;
    i = ((int64_t)x * v.ny + y) * v.nz + z;
    return true;
}

// binarise (proc3d.py:515), occ[i] = on(in[i]): 16 voxels per thread, one 16-byte store.  The predicates: a value above
// one half, compared in float64 like the reference's `volume > 0.5`; a class of a winner volume (class_select.hip;
// DESIGN.md 15), winner == cls.
struct Above {
    template <typename T>
    __device__ __forceinline__ bool operator()(T value) const { return (double)value > 0.5; }
};

struct IsClass {
    uint32_t cls;
    __device__ __forceinline__ bool operator()(uint8_t winner) const { return (uint32_t)winner == cls; }
};

template <typename T, class On>
__global__ __launch_bounds__(kB) void occ_kernel(const T *__restrict__ in, uint8_t *__restrict__ occ, int64_t n, On on) {
    int64_t i0 = ((int64_t)blockIdx.x * kB + threadIdx.x) * 16;
    if (i0 >= n) return;
    if (i0 + 16 <= n && (reinterpret_cast<uintptr_t>(occ) & 15) == 0) {
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t bits = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) bits |= (on(in[i0 + q * 4 + e]) ? 1u : 0u) << (8 * e);
            w[q] = bits;
        }
        *reinterpret_cast<uint4 *>(occ + i0) = make_uint4(w[0], w[1], w[2], w[3]);
    } else {
        for (int64_t i = i0; i < min(n, i0 + 16); ++i) occ[i] = on(in[i]) ? 1 : 0;
    }
}

// The same from carve labels as the ranks of a sharded run leave them after an all-gather: `world` ranks' planes at
// 2 bits (label & 3) or 1 bit (label == 1) per voxel, rank-major ([world][rank_words] words; plane i of the grid is
// plane i / world of rank i % world, or plane i - first(r) of the rank whose slab holds it).  A label is one of
// -1, 0, 1, so `volume > 0.5` (proc3d.py:515) is `label == 1`: the occupancy is read off the packed form and the
// full-size int8 / int32 grid is never written.  occ[0] is voxel 0 of global plane x0.
struct PackedIn {
    const uint32_t *recv;
    uint64_t rank_words;
    uint32_t world, nx_total;
    int32_t cyclic, bits;
};

// A kernel of its own for the word-at-once path: where a plane is whole words, a thread's 16 voxels share a plane and a
// word, located once.  (It repeats occ_kernel's assemble-and-store and tail: with those shared through helpers the
// compiler changed the instructions of every occupancy kernel, the four threshold instances included.)
template <int BITS>
__global__ __launch_bounds__(kB) void occ_packed_kernel(PackedIn pk, uint8_t *__restrict__ occ, int64_t n, uint64_t plane,
                                                        uint32_t x0) {
    constexpr uint32_t PER = 32u / BITS;
    const int64_t i0 = ((int64_t)blockIdx.x * kB + threadIdx.x) * 16;
    if (i0 >= n) return;
    auto locate = [&](uint64_t v, uint32_t &r, uint64_t &src) {  // v: voxel of the GLOBAL grid
        const uint32_t i = (uint32_t)(v / plane);
        const uint64_t within = v - (uint64_t)i * plane;
        uint32_t p;
        if (pk.cyclic) {
            r = i % pk.world;
            p = i / pk.world;
        } else {  // slabs [nx r / world, nx (r + 1) / world)
            r = (uint32_t)(((uint64_t)i * pk.world + pk.world - 1) / pk.nx_total);
            while ((uint64_t)pk.nx_total * r / pk.world > i) --r;
            while ((uint64_t)pk.nx_total * (r + 1) / pk.world <= i) ++r;
            p = i - (uint32_t)((uint64_t)pk.nx_total * r / pk.world);
        }
        src = (uint64_t)p * plane + within;
    };
    const uint64_t g0 = (uint64_t)x0 * plane + (uint64_t)i0;
    if (plane % PER == 0 && i0 + 16 <= n && (reinterpret_cast<uintptr_t>(occ) & 15) == 0) {  // the 16 voxels share a plane and a word
        uint32_t r;
        uint64_t src;
        locate(g0, r, src);
        const uint32_t word = pk.recv[(uint64_t)r * pk.rank_words + src / PER] >> (BITS * (uint32_t)(src % PER));
        uint32_t w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            uint32_t bits = 0;
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const uint32_t lab = (word >> (BITS * (q * 4 + e))) & (BITS == 2 ? 3u : 1u);
                bits |= (lab == 1u ? 1u : 0u) << (8 * e);
            }
            w[q] = bits;
        }
        *reinterpret_cast<uint4 *>(occ + i0) = make_uint4(w[0], w[1], w[2], w[3]);
        return;
    }
    for (int64_t i = i0; i < min(n, i0 + 16); ++i) {
        uint32_t r;
        uint64_t src;
        locate(g0 + (uint64_t)(i - i0), r, src);
        const uint32_t lab = (pk.recv[(uint64_t)r * pk.rank_words + src / PER] >> (BITS * (uint32_t)(src % PER))) & (BITS == 2 ? 3u : 1u);
        occ[i] = lab == 1u ? 1 : 0;
    }
}

// per 8^3 block: bit 0 = holds a foreground voxel, bit 1 = holds a background voxel
__global__ __launch_bounds__(kB) void block_class_kernel(const uint8_t *__restrict__ occ, int nx, int ny,
                                                         int nz, int nbx, int nby, int nbz,
                                                         uint8_t *__restrict__ cls) {
    int64_t b = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (b >= (int64_t)nbx * nby * nbz) return;
    const Blk k = block_split<int64_t>(b, nby, nbz);
    uint32_t fg = 0, bg = 0;
    for (int dx = 0; dx < kBlk; ++dx) {
        int x = k.x * kBlk + dx;
        if (x >= nx) break;
        for (int dy = 0; dy < kBlk; ++dy) {
            int y = k.y * kBlk + dy;
            if (y >= ny) break;
            const uint8_t *row = occ + ((int64_t)x * ny + y) * nz;
            for (int dz = 0; dz < kBlk; ++dz) {
                int z = k.z * kBlk + dz;
                if (z >= nz) break;
                uint8_t o = row[z];
                fg |= o;
                bg |= (uint8_t)(o ^ 1);
            }
        }
    }
    cls[b] = (uint8_t)(fg | (bg << 1));
}

// A voxel can matter only if a voxel of the other class lies within R of it.  Block-level,
// conservative: the block holds class c and some block within rb = ceil(R/8) blocks holds the
// other class.
__global__ __launch_bounds__(kB) void block_active_kernel(const uint8_t *__restrict__ cls, int nbx, int nby,
                                                          int nbz, int rb, uint8_t *__restrict__ active) {
    int64_t b = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (b >= (int64_t)nbx * nby * nbz) return;
    const Blk k = block_split<int64_t>(b, nby, nbz);
    const uint32_t near = near_or(cls, k, rb, nbx, nby, nbz);
    uint32_t own = cls[b];
    // own has fg and a bg block is near, or own has bg and an fg block is near
    active[b] = (uint8_t)((((own & 1u) && (near & 2u)) || ((own & 2u) && (near & 1u))) ? 1 : 0);
}

// Compact the block map into two lists: ACTIVE blocks (the per-voxel kernels walk these) and HALO
// blocks (inactive, but within rb blocks of an active one: the EDT passes of active voxels read
// them, so they must hold "far").  counts[0] / counts[1] receive the list lengths.
__global__ __launch_bounds__(kB) void block_lists_kernel(const uint8_t *__restrict__ active, int nbx, int nby,
                                                         int nbz, int rb, uint32_t *__restrict__ act_list,
                                                         uint32_t *__restrict__ halo_list,
                                                         uint32_t *__restrict__ counts) {
    int64_t b = (int64_t)blockIdx.x * kB + threadIdx.x;
    bool is_act = false, is_halo = false;
    if (b < (int64_t)nbx * nby * nbz) {
        is_act = active[b] != 0;
        if (!is_act) {
            is_halo = near_or(active, block_split<int64_t>(b, nby, nbz), rb, nbx, nby, nbz) != 0;
        }
    }
    wave_append(is_act, (uint32_t)b, act_list, &counts[0]);
    wave_append(is_halo, (uint32_t)b, halo_list, &counts[1]);
}

// halo blocks: (far, far) in both EDT buffers
__global__ __launch_bounds__(kB) void halo_fill_kernel(uint32_t *__restrict__ g0, uint32_t *__restrict__ g1, Vol v) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        int x, y, z;
        int64_t i;
        if (!voxel(v, q, x, y, z, i)) continue;
        g0[i] = 0xffffffffu;
        g1[i] = 0xffffffffu;
    }
}

// columns of blocks (bx, by) that hold an active block: the shell kernels visit only their rows
__global__ __launch_bounds__(kB) void column_list_kernel(const uint8_t *__restrict__ active, int ncols, int nbz,
                                                         uint32_t *__restrict__ col_list,
                                                         uint32_t *__restrict__ count) {
    int c = (int)(blockIdx.x * kB + threadIdx.x);
    bool any = false;
    if (c < ncols)
        for (int bz = 0; bz < nbz; ++bz) any |= active[(int64_t)c * nbz + bz] != 0;
    wave_append(any, (uint32_t)c, col_list, count);
}

// EDT pass along z (the contiguous axis).  Two channels per voxel, packed lo/hi 16 bits:
// A = squared distance to the nearest BACKGROUND voxel of the line, B = to the nearest FOREGROUND
// voxel; a voxel's own class gives 0 in the other channel.  Exact up to R, kFar beyond.
// Inactive voxels count as (far, far): no active voxel of the other class lies within R of them,
// so they are never anybody's nearest site (halo blocks are filled with that, the rest is never read).
__global__ __launch_bounds__(kB) void edt_z_kernel(const uint8_t *__restrict__ occ,
                                                   uint32_t *__restrict__ g, Vol v, int R) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        int x, y, k;
        int64_t i;
        if (!voxel(v, q, x, y, k, i)) continue;
        uint8_t c = occ[i];
        uint32_t best = kFar;
        for (int d = 1; d <= R; ++d) {
            bool hit = (k - d >= 0 && occ[i - d] != c) || (k + d < v.nz && occ[i + d] != c);
            if (hit) { best = (uint32_t)(d * d); break; }
        }
        g[i] = c ? best : (best << 16);  // fg: A=best,B=0 ; bg: A=0,B=best
    }
}

// EDT pass along y: both channels,  H(p) = min_j ( j^2 + G(p + j*stride) ), |j| <= R.
__global__ __launch_bounds__(kB) void edt_y_kernel(const uint32_t *__restrict__ g,
                                                   uint32_t *__restrict__ h, Vol v, int R) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        int x, p, z;
        int64_t i;
        if (!voxel(v, q, x, p, z, i)) continue;
        const int64_t stride = v.nz;
        uint32_t w0 = g[i];
        uint32_t a = w0 & 0xffffu, b = w0 >> 16;
        for (int j = 1; j <= R; ++j) {
            uint32_t jj = (uint32_t)(j * j);
            if (jj >= a && jj >= b) break;  // nothing farther can improve either channel
            if (p - j >= 0) {
                uint32_t w = g[i - j * stride];
                a = min(a, (w & 0xffffu) + jj);
                b = min(b, (w >> 16) + jj);
            }
            if (p + j < v.ny) {
                uint32_t w = g[i + j * stride];
                a = min(a, (w & 0xffffu) + jj);
                b = min(b, (w >> 16) + jj);
            }
        }
        h[i] = min(a, kFar) | (min(b, kFar) << 16);
    }
}

// last EDT pass (along x) fused with the signed distance of proc3d.py:518-522:
//   dist = where(dist > 0.5, dist - 0.5, -mdist + 0.5)
__global__ __launch_bounds__(kB) void edt_x_kernel(const uint32_t *__restrict__ g,
                                                   const uint8_t *__restrict__ occ,
                                                   double *__restrict__ sd, Vol v, int R) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        int p, y, z;
        int64_t i;
        if (!voxel(v, q, p, y, z, i)) continue;
        const int64_t stride = (int64_t)v.ny * v.nz;
        bool fg = occ[i] != 0;
        int sh = fg ? 0 : 16;
        uint32_t a = (g[i] >> sh) & 0xffffu;
        for (int j = 1; j <= R; ++j) {
            uint32_t jj = (uint32_t)(j * j);
            if (jj >= a) break;
            if (p - j >= 0) a = min(a, ((g[i - j * stride] >> sh) & 0xffffu) + jj);
            if (p + j < v.nx) a = min(a, ((g[i + j * stride] >> sh) & 0xffffu) + jj);
        }
        double d = sqrt((double)a);  // exact integer in, correctly rounded sqrt
        sd[i] = fg ? d - 0.5 : -d + 0.5;
    }
}

// np.gradient along one axis (unit spacing, edge_order 1).  At the rim of the active region a
// neighbour may be an inactive voxel holding anything: such values can only reach voxels farther
// from the shell than anything the shell's points depend on (see R).
template <int AXIS>
__global__ __launch_bounds__(kB) void gradient_kernel(const double *__restrict__ f,
                                                      double *__restrict__ out, Vol v) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        int x, y, z;
        int64_t i;
        if (!voxel(v, q, x, y, z, i)) continue;
        const int64_t stride = AXIS == 0 ? (int64_t)v.ny * v.nz : AXIS == 1 ? v.nz : 1;
        const int p = AXIS == 0 ? x : AXIS == 1 ? y : z;
        const int len = AXIS == 0 ? v.nx : AXIS == 1 ? v.ny : v.nz;
        double r;
        if (p == 0) r = f[i + stride] - f[i];
        else if (p == len - 1) r = f[i] - f[i - stride];
        else r = (f[i + stride] - f[i - stride]) / 2.0;
        out[i] = r;
    }
}

__device__ __forceinline__ int reflect_index(int q, int len) {  // scipy "reflect": d c b a | a b c d | d c b a
    int period = 2 * len;
    q %= period;
    if (q < 0) q += period;
    return q < len ? q : period - 1 - q;
}

struct GaussW { double w[5]; };  // w[0] centre .. w[4] farthest

// scipy.ndimage.correlate1d, symmetric branch, radius 4, along one axis
template <int AXIS>
__global__ __launch_bounds__(kB) void gauss_kernel(const double *__restrict__ f, double *__restrict__ out,
                                                   Vol v, GaussW gw) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
        int x, y, z;
        int64_t i;
        if (!voxel(v, q, x, y, z, i)) continue;
        const int64_t stride = AXIS == 0 ? (int64_t)v.ny * v.nz : AXIS == 1 ? v.nz : 1;
        const int p = AXIS == 0 ? x : AXIS == 1 ? y : z;
        const int len = AXIS == 0 ? v.nx : AXIS == 1 ? v.ny : v.nz;
        int64_t base = i - (int64_t)p * stride;
        double tmp = f[i] * gw.w[0];
        if (p >= 4 && p + 4 < len) {
#pragma unroll
            for (int j = 4; j >= 1; --j) tmp += (f[i - j * stride] + f[i + j * stride]) * gw.w[j];
        } else {
#pragma unroll
            for (int j = 4; j >= 1; --j)
                tmp += (f[base + (int64_t)reflect_index(p - j, len) * stride] +
                        f[base + (int64_t)reflect_index(p + j, len) * stride]) * gw.w[j];
        }
        out[i] = tmp;
    }
}

// shell test of proc3d.py:535: (dist > -lsv) * (dist <= -lsv + sqrt(3)), on active voxels only (the
// signed distance of the others is never computed).  A chunk is up to 1024 voxels of one (x, y)
// row, chunk id = (x * ny + y) * nzseg + segment -- C order, like the reference's np.argwhere.  Only
// rows of block columns that hold an active block are visited (the counts of the others stay 0).
constexpr int kChunk = 1024;

__device__ __forceinline__ bool on_shell(const double *__restrict__ sd, const Vol &v, int x, int y, int z,
                                         double lo, double hi, int64_t &i, double &d) {
    if (z >= v.nz || x < v.cx0 || x >= v.cx1) return false;
    if (v.active[((int64_t)(x / kBlk) * v.nby + (y / kBlk)) * v.nbz + (z / kBlk)] == 0) return false;
    i = ((int64_t)x * v.ny + y) * v.nz + z;
    d = sd[i];
    return (d > lo) & (d <= hi);
}

// blockIdx.x = 64 * (entry of the active-column list) + row inside the column, blockIdx.y = z segment
__device__ __forceinline__ bool shell_row(const Vol &v, int &x, int &y) {
    const uint32_t c = v.cols[blockIdx.x >> 6], l = blockIdx.x & 63u;
    x = (int)(c / (uint32_t)v.nby) * kBlk + (int)(l >> 3);
    y = (int)(c % (uint32_t)v.nby) * kBlk + (int)(l & 7u);
    return x < v.nx && y < v.ny;
}

__global__ __launch_bounds__(kB) void shell_count_kernel(const double *__restrict__ sd, Vol v,
                                                         double lo, double hi,
                                                         uint32_t *__restrict__ counts) {
    __shared__ uint32_t s[kB / 64];
    int x, y;
    if (!shell_row(v, x, y)) return;  // block-uniform
    uint32_t c = 0;
    for (int q = 0; q < kChunk / kB; ++q) {
        int z = (int)blockIdx.y * kChunk + q * kB + (int)threadIdx.x;
        int64_t i;
        double d;
        c += on_shell(sd, v, x, y, z, lo, hi, i, d) ? 1u : 0u;
    }
    c = block_sum(c, s);
    if (threadIdx.x == 0) counts[((int64_t)x * v.ny + y) * gridDim.y + blockIdx.y] = c;
}

// C-order compaction of the shell + the per-point step of proc3d.py:539-553,563
__global__ __launch_bounds__(kB) void shell_points_kernel(const double *__restrict__ sd,
                                                          const double *__restrict__ gx,
                                                          const double *__restrict__ gy,
                                                          const double *__restrict__ gz, Vol v,
                                                          double lo, double hi,
                                                          double lsv, double ox, double oy, double oz,
                                                          double vs, const uint32_t *__restrict__ counts,
                                                          const uint64_t *__restrict__ offsets,
                                                          double *__restrict__ pts,
                                                          double *__restrict__ nrm) {
    __shared__ uint32_t wsum[kB / 64];
    int x, y;
    if (!shell_row(v, x, y)) return;  // block-uniform
    const int64_t chunk = ((int64_t)x * v.ny + y) * gridDim.y + blockIdx.y;
    if (counts[chunk] == 0) return;  // block-uniform
    uint64_t off = offsets[chunk];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int q = 0; q < kChunk / kB; ++q) {
        int z = (int)blockIdx.y * kChunk + q * kB + (int)threadIdx.x;
        int64_t i = 0;
        double d = 0.0;
        bool on = on_shell(sd, v, x, y, z, lo, hi, i, d);
        unsigned long long b = __ballot(on);
        if (lane == 0) wsum[wave] = (uint32_t)__popcll(b);
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (uint32_t w = 0; w < kB / 64; ++w) {
            if (w < wave) before += wsum[w];
            total += wsum[w];
        }
        if (on) {
            unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
            uint64_t r = off + before + (uint32_t)__popcll(b & below);
            double a = gx[i], bq = gy[i], c = gz[i];
            double nn = sqrt((a * a + bq * bq) + c * c);
            double px = NAN, py = NAN, pz = NAN, n0 = NAN, n1 = NAN, n2 = NAN;
            if (nn > 0.0) {
                double u0 = a / nn, u1 = bq / nn, u2 = c / nn;
                double val = d + lsv - sqrt(3.0) / 2.0;
                double xi = (double)(x + v.xoff), yi = (double)y, zi = (double)z;
                // index2point (proc3d.py:45): voxel_size * idx + origin
                px = vs * (xi - u0 * val) + ox;
                py = vs * (yi - u1 * val) + oy;
                pz = vs * (zi - u2 * val) + oz;
                // -grad_normalized, then open3d's normalize_normals
                double m0 = -u0, m1 = -u1, m2 = -u2;
                double mm = sqrt((m0 * m0 + m1 * m1) + m2 * m2);
                n0 = m0 / mm; n1 = m1 / mm; n2 = m2 / mm;
            }
            pts[3 * r] = px; pts[3 * r + 1] = py; pts[3 * r + 2] = pz;
            nrm[3 * r] = n0; nrm[3 * r + 1] = n1; nrm[3 * r + 2] = n2;
        }
        off += total;
        __syncthreads();
    }
}

// Exclusive prefix sum of the chunk counts (C order) on the device, so that only the total
// crosses PCIe: per x-plane sums, then every plane scans its own counts from its base.
__global__ __launch_bounds__(kB) void plane_sums_kernel(const uint32_t *__restrict__ counts, int64_t per_plane,
                                                        uint64_t *__restrict__ plane_sum) {
    __shared__ uint64_t s[kB / 64];
    const uint32_t *c = counts + (int64_t)blockIdx.x * per_plane;
    uint64_t sum = 0;
    for (int64_t i = threadIdx.x; i < per_plane; i += kB) sum += c[i];
    sum = block_sum(sum, s);
    if (threadIdx.x == 0) plane_sum[blockIdx.x] = sum;
}

__global__ __launch_bounds__(kB) void chunk_offsets_kernel(const uint32_t *__restrict__ counts, int64_t per_plane,
                                                           const uint64_t *__restrict__ plane_sum,
                                                           uint64_t *__restrict__ offsets,
                                                           uint64_t *__restrict__ total) {
    __shared__ uint64_t s[kB / 64];
    __shared__ uint64_t carry;
    // base of this plane = sum of the planes before it
    uint64_t before = 0;
    for (uint32_t x = threadIdx.x; x < blockIdx.x; x += kB) before += plane_sum[x];
    before = block_sum(before, s);
    if (threadIdx.x == 0) carry = before;
    __syncthreads();
    const uint32_t *c = counts + (int64_t)blockIdx.x * per_plane;
    uint64_t *o = offsets + (int64_t)blockIdx.x * per_plane;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    for (int64_t t = 0; t < per_plane; t += kB) {
        const int64_t i = t + threadIdx.x;
        const uint64_t mine = i < per_plane ? c[i] : 0;
        uint64_t inc = mine;  // inclusive scan inside the wavefront
        for (int d = 1; d < 64; d <<= 1) {
            uint64_t up = __shfl_up(inc, d);
            if ((int)lane >= d) inc += up;
        }
        if (lane == 63) s[wave] = inc;
        __syncthreads();
        uint64_t base = carry;
        for (uint32_t w = 0; w < wave; ++w) base += s[w];
        if (i < per_plane) o[i] = base + inc - mine;
        __syncthreads();
        if (threadIdx.x == kB - 1) carry = base + inc;
        __syncthreads();
    }
    if (blockIdx.x == gridDim.x - 1 && threadIdx.x == 0) *total = carry;
}

inline uint32_t blocks_for(int64_t n) { return (uint32_t)((n + kB - 1) / kB); }

// Every launch of this unit: blocks of kB threads on the null stream.
template <class... P, class... A>
void launch(void (*kernel)(P...), dim3 grid, A... args) { hipLaunchKernelGGL(kernel, grid, dim3(kB), 0, nullptr, args...); }

// What can reach a shell voxel: |d| <= |lsv| + sqrt(3) there, gradient 1 + Gaussian 4 per axis.
int reach_of(double level_set_value) {
    return (int)std::ceil(std::fabs(level_set_value) + 1.7321 + 5.0 * 1.7321 + 3.0);
}

// The constants of one call: an entry's arguments as they came and, once the driver has judged them, what they imply.
struct Call {
    const double *origin;  // [3]
    double voxel_size, level_set_value;
    const double *gauss_w;  // [5]
    int device;
    int R = 0, rb = 0;          // derived: the reach in voxels and in blocks,
    double lo = 0.0, hi = 0.0;  // the shell lo < d <= hi
    void derive() {
        R = reach_of(level_set_value), rb = (R + kBlk - 1) / kBlk;
        lo = -level_set_value, hi = -level_set_value + std::sqrt(3.0);
    }
};

// The planes at hand as the driver names them: a Vol whose buffers vol2pcd_range fills in.
Vol planes_at_hand(int64_t nx, int64_t ny, int64_t nz, int xoff, int cx0, int cx1) {
    const int nby = (int)((ny + kBlk - 1) / kBlk), nbz = (int)((nz + kBlk - 1) / kBlk);
    return Vol{(int)nx, (int)ny, (int)nz, nby, nbz, nullptr, nullptr, nullptr, xoff, cx0, cx1};
}

// The work buffers for `planes` x-planes of ny x nz voxels in one allocation of `bytes`, each on a 256-byte boundary:
// one statement per buffer gives its place and its pointer (null without a `base`: the driver only asks for `bytes`).
struct ScratchLayout {
    uint8_t *occ, *cls, *act;                             // the occupancy per voxel; class bits and activity per block
    uint32_t *list_act, *list_halo, *list_cols, *list_n;  // the lists of blocks and columns, their three lengths
    uint64_t *total, *plane_sum, *offsets;                // the shell's voxels: all, per x-plane, before each chunk
    uint32_t *counts, *g0, *g1;                           // ... in each chunk; the EDT's two buffers
    double *sd, *ga, *gb, *gx, *gy, *gz;                  // signed distance, two intermediates, the smoothed gradient
    size_t bytes;

    ScratchLayout(int64_t planes, int64_t ny, int64_t nz, char *base = nullptr) {
        const size_t n = (size_t)(planes * ny * nz), nchunks = (size_t)(planes * ny * ((nz + kChunk - 1) / kChunk));
        const size_t nbxy = (size_t)(((planes + kBlk - 1) / kBlk) * ((ny + kBlk - 1) / kBlk));
        const size_t nb = nbxy * (size_t)((nz + kBlk - 1) / kBlk);
        Layout lay;
        auto put = [base](auto *&p, size_t at) { p = base ? reinterpret_cast<decltype(+p)>(base + at) : nullptr; };
        size_t at;
        put(occ, lay.take(n));
        put(cls, lay.take(nb));
        put(act, lay.take(nb));
        put(list_act, lay.take(nb * 4));
        put(list_halo, lay.take(nb * 4));
        put(list_cols, lay.take(nbxy * 4));
        put(list_n, at = lay.take(64));
        put(total, at + 16);  // ALIAS: the total lies in list_n's 64 bytes, behind the three lengths (one memset)
        put(plane_sum, lay.take((size_t)planes * 8));
        put(counts, lay.take(nchunks * 4));
        put(offsets, lay.take(nchunks * 8));
        put(sd, lay.take(n * 8));
        put(ga, at = lay.take(n * 8));
        put(g0, at);          // ALIAS: the EDT's two 4-byte buffers are the halves of ga's 8 n bytes; its last pass has
        put(g1, at + n * 4);  // read them before the first gradient is written there
        put(gb, lay.take(n * 8));
        put(gx, lay.take(n * 8));
        put(gy, lay.take(n * 8));
        put(gz, lay.take(n * 8));
        bytes = lay.total;
    }
};

// What a call makes the occupancy from: a volume to compare with one half (four dtypes; host or device memory), a
// class of a winner volume (likewise), or the packed labels of a sharded run.
struct Input {
    enum Form { kDense, kWinner, kPacked } form;
    const char *volume = nullptr;  // kDense, kWinner: plane 0 of [nx][ny][nz] ...
    bool on_device = false;        // ... in the memory of the call's device, else in the host's
    int dtype = 3;                 // 0 int32, 1 float32, 2 float64, 3 uint8 (a winner volume's)
    uint32_t cls = 0;              // kWinner
    PackedIn pk = {};              // kPacked

    size_t elem() const { return dtype == 3 ? 1 : dtype == 2 ? 8 : 4; }  // bytes per voxel of `volume`

    // occ = the occupancy of planes [a, b) of `plane` voxels each; a host volume's go to the device through `staged`
    int occupancy(int64_t a, int64_t b, uint64_t plane, void *&staged, uint8_t *occ) const {
        const int64_t n = (b - a) * (int64_t)plane;
        const dim3 grid(blocks_for((n + 15) / 16));
        if (form == kPacked) {
            if (pk.bits == 2) launch(occ_packed_kernel<2>, grid, pk, occ, n, plane, (uint32_t)a);
            else launch(occ_packed_kernel<1>, grid, pk, occ, n, plane, (uint32_t)a);
            return SC_OK;
        }
        const void *at = volume + (size_t)a * plane * elem();
        if (!on_device) {
            HIP_TRY(hipMalloc(&staged, (size_t)n * elem()));
            HIP_TRY(hipMemcpy(staged, at, (size_t)n * elem(), hipMemcpyHostToDevice));
            at = staged;
        }
        if (form == kWinner) launch(occ_kernel<uint8_t, IsClass>, grid, (const uint8_t *)at, occ, n, IsClass{cls});
        else if (dtype == 0) launch(occ_kernel<int32_t, Above>, grid, (const int32_t *)at, occ, n, Above{});
        else if (dtype == 1) launch(occ_kernel<float, Above>, grid, (const float *)at, occ, n, Above{});
        else if (dtype == 2) launch(occ_kernel<double, Above>, grid, (const double *)at, occ, n, Above{});
        else launch(occ_kernel<uint8_t, Above>, grid, (const uint8_t *)at, occ, n, Above{});
        return SC_OK;
    }
};

// The pipeline on the planes at hand (`v` comes without its buffers), in four stages; a failure simply returns.
int vol2pcd_range(const Input &in, const Call &c, Vol v, double **points_out, double **normals_out, int64_t *count) {
    *points_out = *normals_out = nullptr, *count = 0;
    const int nbx = (v.nx + kBlk - 1) / kBlk, nby = v.nby, nbz = v.nbz;
    const uint32_t nzseg = (uint32_t)((v.nz + kChunk - 1) / kChunk);
    const int64_t nb = (int64_t)nbx * nby * nbz, per_plane = v.ny * (int64_t)nzseg, nchunks = v.nx * per_plane;
    if (nb > 0xffffffffLL || nchunks > 0x7fffffffLL) return g_err.fail(SC_ERR_INVALID, "volume too large");
    Held held;  // waits for the device, then frees, however the function is left
    HIP_TRY(hipSetDevice(c.device));
    if (!held.take_work(c.device, ScratchLayout(v.nx, v.ny, v.nz).bytes))
        return g_err.fail(SC_ERR_NOMEM, "device allocation of the work buffers failed");
    const ScratchLayout at(v.nx, v.ny, v.nz, held.work);
    v.active = at.act, v.list = at.list_act, v.cols = at.list_cols;

    // 1: the occupancy, the block map, the lists of active blocks, halo blocks and active columns, and their lengths
    const dim3 per_block(blocks_for(nb));
    const int rc = in.occupancy(v.xoff, v.xoff + v.nx, (uint64_t)v.ny * (uint64_t)v.nz, held.staged, at.occ);
    if (rc != SC_OK) return rc;
    launch(block_class_kernel, per_block, at.occ, v.nx, v.ny, v.nz, nbx, nby, nbz, at.cls);
    launch(block_active_kernel, per_block, at.cls, nbx, nby, nbz, c.rb, at.act);
    HIP_TRY(hipMemsetAsync(at.list_n, 0, 64, nullptr));
    launch(block_lists_kernel, per_block, at.act, nbx, nby, nbz, c.rb, at.list_act, at.list_halo, at.list_n);
    launch(column_list_kernel, dim3(blocks_for((int64_t)nbx * nby)), at.act, nbx * nby, nbz, at.list_cols, at.list_n + 2);
    HIP_TRY(hipMemsetAsync(at.counts, 0, (size_t)nchunks * 4, nullptr));  // rows the shell kernels skip count nothing
    HIP_TRY(hipGetLastError());
    uint32_t nlist[3] = {0, 0, 0};  // blocks in the active list, in the halo list; columns in the column list
    // the only host round trip before the result: how many blocks the per-voxel kernels walk
    HIP_TRY(hipMemcpy(nlist, at.list_n, sizeof nlist, hipMemcpyDeviceToHost));
    if (nlist[0] == 0) return SC_OK;

    // 2: the signed distance; per axis its gradient, then gaussian_filter over axes 0, 1, 2 in turn (proc3d.py:525-531)
    const dim3 active(nlist[0]);
    Vol halo = v;  // halo blocks hold (far, far) in both EDT buffers; other inactive voxels are never read
    halo.list = at.list_halo;
    if (nlist[1] > 0) launch(halo_fill_kernel, dim3(nlist[1]), at.g0, at.g1, halo);
    launch(edt_z_kernel, active, at.occ, at.g0, v, c.R);
    launch(edt_y_kernel, active, at.g0, at.g1, v, c.R);
    launch(edt_x_kernel, active, at.g1, at.occ, at.sd, v, c.R);
    HIP_TRY(hipGetLastError());
    decltype(&gradient_kernel<0>) const gradient[3] = {gradient_kernel<0>, gradient_kernel<1>, gradient_kernel<2>};
    double *const smoothed[3] = {at.gx, at.gy, at.gz};
    GaussW gw;
    memcpy(gw.w, c.gauss_w, sizeof gw.w);
    for (int axis = 0; axis < 3; ++axis) {
        launch(gradient[axis], active, at.sd, at.ga, v);
        launch(gauss_kernel<0>, active, at.ga, at.gb, v, gw);
        launch(gauss_kernel<1>, active, at.gb, at.ga, v, gw);
        launch(gauss_kernel<2>, active, at.ga, smoothed[axis], v, gw);
    }
    HIP_TRY(hipGetLastError());

    // 3: the shell's voxels per chunk, their C-order offsets, the total
    const dim3 rows(nlist[2] * 64u, nzseg), per_x((uint32_t)v.nx);
    uint64_t total = 0;
    launch(shell_count_kernel, rows, at.sd, v, c.lo, c.hi, at.counts);
    launch(plane_sums_kernel, per_x, at.counts, per_plane, at.plane_sum);
    launch(chunk_offsets_kernel, per_x, at.counts, per_plane, at.plane_sum, at.offsets, at.total);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpy(&total, at.total, sizeof total, hipMemcpyDeviceToHost));
    if (total == 0) return SC_OK;

    // 4: the points and normals, on the device and then in malloc'ed host arrays
    const size_t bytes = (size_t)total * 24;
    HIP_TRY(hipMalloc(&held.points, 2 * bytes));
    double *const pts_d = static_cast<double *>(held.points), *const nrm_d = pts_d + total * 3;
    launch(shell_points_kernel, rows, at.sd, at.gx, at.gy, at.gz, v, c.lo, c.hi, c.level_set_value, c.origin[0],
           c.origin[1], c.origin[2], c.voxel_size, at.counts, at.offsets, pts_d, nrm_d);
    hipError_t e = hipGetLastError();
    double *P = static_cast<double *>(malloc(bytes)), *N = static_cast<double *>(malloc(bytes));
    const bool have = P && N;
    if (have && e == hipSuccess) e = hipMemcpy(P, pts_d, bytes, hipMemcpyDeviceToHost);
    if (have && e == hipSuccess) e = hipMemcpy(N, nrm_d, bytes, hipMemcpyDeviceToHost);
    if (!have || e != hipSuccess) {
        free(P); free(N);
        return e != hipSuccess ? g_err.hip(e) : g_err.fail(SC_ERR_NOMEM, "host allocation failed");
    }
    *points_out = P, *normals_out = N, *count = (int64_t)total;
    return SC_OK;
}

// Largest work buffers a call may take (0: no limit).  49 bytes per voxel is 6.6 GB at 512^3 and 52 GB at
// 1024^3; above the limit the volume goes through in x-SLABS: every step of the pipeline has a finite reach
// along x (the distance transform is exact up to the reach R and clamped beyond, the gradient reaches 1 plane,
// the three Gaussians 4), so the planes [c0, c1) with H = R + 8 planes of halo on either side give the shell
// voxels of [c0, c1) the values the whole volume would give them -- the one-sided differences and the
// reflections at a slab's artificial ends stay inside the halo.  Slabs come in x order, which is the order of
// the output (C order of the shell voxels).
// (Default 8 GiB: a 512^3 volume still goes through in one piece, 4.6 ms against 7.5 in 1 GiB slabs; buffers above
// 1 GiB are given back when the call ends either way, see ScratchLease.)
int64_t g_scratch_limit = (int64_t)8 << 30;

int vol2pcd_driver(const Input &in, int64_t nx, int64_t ny, int64_t nz, Call c, double **points_out,
                   double **normals_out, int64_t *count) {
    if ((in.form != Input::kPacked && !in.volume) || !c.origin || !c.gauss_w || !points_out || !normals_out || !count)
        return g_err.fail(SC_ERR_INVALID, "null argument");
    if (nx < 2 || ny < 2 || nz < 2) return g_err.fail(SC_ERR_INVALID, "np.gradient needs at least 2 voxels per axis");
    if (nx > 65535 || ny > 65535) return g_err.fail(SC_ERR_INVALID, "x and y are limited to 65535 voxels");
    if (in.dtype < 0 || in.dtype > 3) return g_err.fail(SC_ERR_INVALID, "volume dtype: 0 int32, 1 float32, 2 float64, 3 uint8");
    if (!(std::fabs(c.level_set_value) < 200.0)) return g_err.fail(SC_ERR_INVALID, "level_set_value out of range");
    *points_out = *normals_out = nullptr, *count = 0;
    c.derive();
    CallerDevice caller(c.device);  // put back when the call ends
    const int64_t limit = g_scratch_limit;
    const int H = c.R + 8;
    int64_t planes = nx;
    if (limit > 0 && ScratchLayout(nx, ny, nz).bytes > (size_t)limit) {
        const size_t per_plane = ScratchLayout(64, ny, nz).bytes / 64 + 1;
        planes = std::max<int64_t>((int64_t)((size_t)limit / per_plane), 2 * H + 8);  // at least 8 planes of its own per slab
    }
    if (planes >= nx)
        return vol2pcd_range(in, c, planes_at_hand(nx, ny, nz, 0, 0, (int)nx), points_out, normals_out, count);
    const int64_t S = planes - 2 * H;
    std::vector<double *> ps, ns;
    std::vector<int64_t> cs;
    int rc = SC_OK;
    int64_t total = 0;
    for (int64_t c0 = 0; c0 < nx && rc == SC_OK; c0 += S) {
        const int64_t c1 = std::min(nx, c0 + S), a = std::max<int64_t>(0, c0 - H), b = std::min(nx, c1 + H);
        double *p = nullptr, *q = nullptr;
        int64_t got = 0;
        rc = vol2pcd_range(in, c, planes_at_hand(b - a, ny, nz, (int)a, (int)(c0 - a), (int)(c1 - a)), &p, &q, &got);
        ps.push_back(p); ns.push_back(q); cs.push_back(got);
        total += got;
    }
    if (rc == SC_OK && total > 0) {
        double *P = static_cast<double *>(malloc((size_t)total * 24)), *N = static_cast<double *>(malloc((size_t)total * 24));
        if (!P || !N) {
            free(P); free(N);
            rc = g_err.fail(SC_ERR_NOMEM, "host allocation failed");
        } else {
            int64_t at = 0;
            for (size_t k = 0; k < cs.size(); ++k) {
                if (cs[k] > 0) {
                    memcpy(P + 3 * at, ps[k], (size_t)cs[k] * 24);
                    memcpy(N + 3 * at, ns[k], (size_t)cs[k] * 24);
                    at += cs[k];
                }
            }
            *points_out = P;
            *normals_out = N;
            *count = total;
        }
    }
    for (size_t k = 0; k < ps.size(); ++k) { free(ps[k]); free(ns[k]); }
    return rc;
}

}  // namespace

extern "C" {

const char *sc_vol2pcd_last_error(void) { return g_err.msg; }

void sc_free_host(void *p) { free(p); }

void sc_vol2pcd_set_scratch_limit(int64_t bytes) { g_scratch_limit = bytes < 0 ? 0 : bytes; }

int sc_vol2pcd(const void *volume, int on_device, int dtype, int64_t nx, int64_t ny, int64_t nz, const double origin[3],
               double voxel_size, double level_set_value, const double gauss_w[5], int device, double **points_out,
               double **normals_out, int64_t *count) {
    const Input in{Input::kDense, static_cast<const char *>(volume), on_device != 0, dtype};
    const Call c{origin, voxel_size, level_set_value, gauss_w, device};
    return vol2pcd_driver(in, nx, ny, nz, c, points_out, normals_out, count);
}

int sc_vol2pcd_packed(const void *recv_dev, int64_t rank_bytes, int world, int partition, int bits, int64_t nx,
                      int64_t ny, int64_t nz, const double origin[3], double voxel_size, double level_set_value,
                      const double gauss_w[5], int device, double **points_out, double **normals_out, int64_t *count) {
    if (!recv_dev) return g_err.fail(SC_ERR_INVALID, "null argument");
    if (bits != 1 && bits != 2) return g_err.fail(SC_ERR_INVALID, "bits must be 1 or 2");
    if (partition != 0 && partition != 1) return g_err.fail(SC_ERR_INVALID, "partition: 0 plane-cyclic, 1 slabs");
    if (world < 1 || nx < world || rank_bytes < 0 || (rank_bytes & 3)) return g_err.fail(SC_ERR_INVALID, "bad world / stride");
    const uint64_t pmax = (uint64_t)(nx + world - 1) / world;
    if ((uint64_t)rank_bytes * 8 < pmax * (uint64_t)ny * (uint64_t)nz * (uint64_t)bits)
        return g_err.fail(SC_ERR_INVALID, "rank stride too small for its planes");
    Input in{Input::kPacked};
    in.pk = PackedIn{static_cast<const uint32_t *>(recv_dev), (uint64_t)rank_bytes / 4, (uint32_t)world, (uint32_t)nx,
                     partition == 0 ? 1 : 0, bits};
    const Call c{origin, voxel_size, level_set_value, gauss_w, device};
    return vol2pcd_driver(in, nx, ny, nz, c, points_out, normals_out, count);
}

int sc_vol2pcd_class(const uint8_t *winner, int on_device, int cls, int64_t nx, int64_t ny, int64_t nz, const double origin[3],
                     double voxel_size, double level_set_value, const double gauss_w[5], int device, double **points_out,
                     double **normals_out, int64_t *count) {
    if (cls < 0 || cls > 255) return g_err.fail(SC_ERR_INVALID, "cls must be 0..255 (a byte of the winner volume)");
    const Input in{Input::kWinner, reinterpret_cast<const char *>(winner), on_device != 0, 3, (uint32_t)cls};
    const Call c{origin, voxel_size, level_set_value, gauss_w, device};
    return vol2pcd_driver(in, nx, ny, nz, c, points_out, normals_out, count);
}

void sc_vol2pcd_release(void) {
    std::lock_guard<std::mutex> lock(g_scratch_mu);
    on_each_device([](int d) {
        ScratchSlot &sl = g_scratch[d];
        if (sl.base && !sl.busy && hipSetDevice(d) == hipSuccess) sl.drop();
    });
}

}  // extern "C"
