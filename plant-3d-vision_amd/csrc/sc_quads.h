// sc_quads.h -- the quad walk of evaluate.hip (volumes) and class_select.hip: the typed loads of a quad, the geometry
// of a launch with each thread's place in it, and the host's planning around it (run plan, one-launch limit, slab
// size, chunk limit).  Internal linkage like sc_unit.h: every unit that includes it has its own copy.
// evaluate.hip plans with QuadGeom but hands its kernel the fields flat and derives the thread's place there (the
// same arithmetic as quad_at; its comment says why): a change to quad_at belongs there too.
//
// A thread owns one quad -- 4 consecutive voxels of one z-row -- of the (y, z) plane and walks a run of x-planes with
// it: lanes run along z, every value is read once, a quad whose 4 values lie inside the row and whose address is
// aligned is one wide load (16 bytes of float32, 2 x 16 of float64, 4 of uint8), any other quad up to 4 scalar loads.
// Nothing is read beyond the quad's own voxels: a row tail of nv < 4 voxels touches nv values.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdint>

#include "spacecarve.h"

namespace {

constexpr int kQuadThreads = 256;  // threads of a block = quads of a tile

// The 4 values of a whole, aligned quad as they lie in memory: loaded now, widened when they are used.
template <class T>
struct Quad;

template <>
struct Quad<float> {
    float4 r;
    static constexpr uintptr_t kAlign = 15;
    __device__ __forceinline__ void load(const float *p) { r = *reinterpret_cast<const float4 *>(p); }
    __device__ __forceinline__ void widen(double out[4]) const {
        out[0] = (double)r.x;
        out[1] = (double)r.y;
        out[2] = (double)r.z;
        out[3] = (double)r.w;
    }
};

template <>
struct Quad<double> {
    double2 a, b;
    static constexpr uintptr_t kAlign = 15;
    __device__ __forceinline__ void load(const double *p) {
        a = *reinterpret_cast<const double2 *>(p);
        b = *reinterpret_cast<const double2 *>(p + 2);
    }
    __device__ __forceinline__ void widen(double out[4]) const {
        out[0] = a.x;
        out[1] = a.y;
        out[2] = b.x;
        out[3] = b.y;
    }
};

template <>
struct Quad<uint8_t> {
    uint32_t r;
    static constexpr uintptr_t kAlign = 3;
    __device__ __forceinline__ void load(const uint8_t *p) { r = *reinterpret_cast<const uint32_t *>(p); }
    __device__ __forceinline__ void widen(double out[4]) const {
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = (double)((r >> (8 * j)) & 255u);
    }
};

// any quad: the wide load where it is whole and aligned, up to 4 scalar loads otherwise; out[j] = fill for j >= nv
template <class T>
__device__ __forceinline__ void load4(const T *p, int nv, double fill, double out[4]) {
    if (nv == 4 && (reinterpret_cast<uintptr_t>(p) & Quad<T>::kAlign) == 0) {
        Quad<T> q;
        q.load(p);
        q.widen(out);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) out[j] = j < nv ? (double)p[j] : fill;
    }
}

// What every quad kernel is told about its launch; class_select's argument struct embeds it.
struct QuadGeom {
    int L, background;
    int nx, ny, nz;  // of this launch
    int Q;           // quads per row
    int xc;          // x-planes per block
    uint32_t tiles;  // blocks per run of planes
};

// A thread's place: its quad (y, z0 .. z0 + nv) and its run of planes [x0, x1).  A thread beyond the plane has no
// voxel (live false, nv 0) and the address of quad 0.  x0 and x1 are block-uniform.
struct QuadAt {
    bool live;
    int y, z0, nv;
    int64_t x0, x1;
};

__device__ __forceinline__ QuadAt quad_at(const QuadGeom g) {  // by value: the kernel argument's words are loaded together
    const uint32_t tile = blockIdx.x % g.tiles, run = blockIdx.x / g.tiles;
    const int64_t q = (int64_t)tile * kQuadThreads + threadIdx.x, nq = (int64_t)g.ny * g.Q;
    const bool live = q < nq;
    const int y = live ? (int)(q / g.Q) : 0, z0 = live ? (int)(q % g.Q) * 4 : 0;
    const int64_t x0 = (int64_t)run * g.xc;
    return QuadAt{live, y, z0, live ? min(4, g.nz - z0) : 0, x0, min((int64_t)g.nx, x0 + g.xc)};
}

// ---- the host's planning --------------------------------------------------------------------------------------
size_t dtype_bytes(int code) { return code == SC_EVAL_F32 ? 4 : code == SC_EVAL_F64 ? 8 : code == SC_EVAL_U8 ? 1 : 0; }

constexpr int64_t kFillBlocks = 4096;    // blocks that fill the device
constexpr int kRunPlanesLog2 = 20;       // at most 2^20 planes per block: its 32-bit counters in LDS hold 1024 * 2^20 voxels

int64_t quad_tiles(int64_t ny, int64_t nz) { return (ny * ((nz + 3) / 4) + kQuadThreads - 1) / kQuadThreads; }
int64_t least_runs(int64_t planes) { return (planes + ((int64_t)1 << kRunPlanesLog2) - 1) >> kRunPlanesLog2; }

// What a call knows before it plans a launch; plan_quads sets the rest.  G: QuadGeom, or a struct with its fields.
template <class G>
void set_quads(G &g, int L, int background, int64_t ny, int64_t nz) {
    g.L = L;
    g.background = background;
    g.ny = (int)ny;
    g.nz = (int)nz;
    g.Q = (int)((nz + 3) / 4);
}

// The run plan of one launch over `planes` x-planes: enough blocks to fill the device, no
// block with more than 2^20 planes.  Sets g.nx, g.xc and g.tiles; returns the grid.
template <class G>
dim3 plan_quads(G &g, int64_t planes) {
    const int64_t tiles = quad_tiles(g.ny, g.nz);
    int64_t runs = std::min<int64_t>(planes, std::max<int64_t>((kFillBlocks + tiles - 1) / tiles, least_runs(planes)));
    const int64_t xc = (planes + runs - 1) / runs;
    runs = (planes + xc - 1) / xc;
    g.nx = (int)planes;
    g.xc = (int)xc;
    g.tiles = (uint32_t)tiles;
    return dim3((uint32_t)(tiles * runs));
}

// whether plan_quads' grid can be indexed for every launch of at most nx planes
bool one_launch_holds(int64_t nx, int64_t ny, int64_t nz) { return quad_tiles(ny, nz) * least_runs(nx) <= 0x7fffffffLL - 8192; }

// x-planes per slab of host volumes: what `limit` bytes leave room for behind the `laid` bytes already laid out and
// the `pad` bytes of alignment the slabs may cost; one plane at least, whatever the limit.
int64_t slab_planes(size_t limit, size_t laid, size_t per_plane, size_t pad) {
    const size_t room = limit > laid + pad ? limit - laid - pad : 0;
    return std::max<int64_t>(1, (int64_t)(room / per_plane));
}

// The bytes of work buffer a unit gives the inputs of one call that lie in host memory.
struct ChunkLimit {
    static constexpr int64_t kDefault = (int64_t)256 << 20;
    std::atomic<int64_t> bytes{kDefault};
    void set(int64_t b) { bytes.store(b > 0 ? b : kDefault); }  // not positive: the default again
    size_t get() const { return (size_t)bytes.load(); }
};

}  // namespace
