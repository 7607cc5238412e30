// sc_points.h -- what dbscan.hip and nearest.hip share about clouds of float64 points: the squared distance (rule 1
// of dbscan.hip, N1 of nearest.hip: ONE text, so the two units and the CPU rehearsal decide every pair alike) and the
// two judges of non-finite coordinates, the host's for host points and a kernel for device points.
// dist2 is host and device and needs no HIP; the rest is for the units only (behind __HIPCC__).
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>

#if defined(__HIPCC__)
#include "sc_unit.h"
#define SC_HD __host__ __device__ __forceinline__
#else
#define SC_HD inline
#endif

namespace {

// d2 = ((dx dx) + (dy dy)) + (dz dz) in IEEE binary64 without contraction (-ffp-contract=off), dx = ax - bx
SC_HD double dist2(double ax, double ay, double az, double bx, double by, double bz) {
    const double dx = ax - bx, dy = ay - by, dz = az - bz;
    return ((dx * dx) + (dy * dy)) + (dz * dz);
}

#if defined(__HIPCC__)
// host points: refuses the first of the n points p that has a NaN or an infinity, as "<what> <its number>"
int first_non_finite(UnitError &err, const double *p, int64_t n, const char *what) {
    for (int64_t k = 0; k < 3 * n; ++k)
        if (!std::isfinite(p[k])) {
            char msg[160];
            snprintf(msg, sizeof msg, "non-finite coordinate in %s %lld", what, (long long)(k / 3));
            return err.fail(SC_ERR_INVALID, msg);
        }
    return SC_OK;
}

// device points have no other judge.  flag: zeroed before the launch; one add per block that saw a NaN or an infinity
__global__ __launch_bounds__(256) void points_finite_kernel(const double *__restrict__ pts, int64_t n3, unsigned int *flag) {
    __shared__ int sbad;
    if (threadIdx.x == 0) sbad = 0;
    __syncthreads();
    int bad = 0;
    for (int64_t k = (int64_t)blockIdx.x * 256 + threadIdx.x; k < n3; k += (int64_t)gridDim.x * 256)
        if (!(fabs(pts[k]) <= DBL_MAX)) bad = 1;
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(&sbad, 1);
    __syncthreads();
    if (threadIdx.x == 0 && sbad) atomicAdd(flag, 1u);
}

// grid-stride over the 3 n coordinates of n >= 1 points
void launch_points_finite(hipStream_t stream, const double *pts, int64_t n, unsigned int *flag) {
    const uint32_t blocks = (uint32_t)std::min<int64_t>((n + 255) / 256, 1024);
    hipLaunchKernelGGL(points_finite_kernel, dim3(blocks), dim3(256), 0, stream, pts, 3 * n, flag);
}
#endif

}  // namespace
