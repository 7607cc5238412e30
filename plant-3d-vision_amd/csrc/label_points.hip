// label_points.hip -- SegmentedPointCloud's point back-projection on the GPU.
//
// Replaces the per-point Python loop of plant3dvision/tasks/proc3d.py:203-232 over
// plant3dvision/proc3d.py::backproject_points (:655-659): every point is projected into every
// view in float64 (x = R p + t; x = K x; x /= x_z), the pixel is int(x + 0.5) -- truncation toward
// zero, a DIFFERENT rounding from the carve kernel's -- and, if it is inside the picture, the
// label image's value is added to scores[label][point]; the point's label is the arg-max.
// The reference multiplies with BLAS (`rot @ points.T`), whose summation order is the machine's;
// here each dot product is evaluated left to right without FMA.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "sc_unit.h"

namespace {

constexpr int kB = 256;
thread_local UnitError g_err;

__global__ __launch_bounds__(kB) void label_points_kernel(const double *__restrict__ pts, int64_t P,
                                                          int L, int V, const double *__restrict__ K,
                                                          const double *__restrict__ R,
                                                          const double *__restrict__ t,
                                                          const uint8_t *__restrict__ masks, int H, int W,
                                                          double *__restrict__ scores,
                                                          int32_t *__restrict__ labels) {
    int64_t i = (int64_t)blockIdx.x * kB + threadIdx.x;
    if (i >= P) return;
    const double px = pts[3 * i], py = pts[3 * i + 1], pz = pts[3 * i + 2];
    for (int l = 0; l < L; ++l) scores[(int64_t)l * P + i] = 0.0;
    for (int v = 0; v < V; ++v) {
        const double *r = R + 9 * v, *k = K + 4 * v, *tv = t + 3 * v;
        // rot @ p + tvec (proc3d.py:656)
        double x0 = ((r[0] * px + r[1] * py) + r[2] * pz) + tv[0];
        double x1 = ((r[3] * px + r[4] * py) + r[5] * pz) + tv[1];
        double x2 = ((r[6] * px + r[7] * py) + r[8] * pz) + tv[2];
        // K @ x with K = [[fx,0,cx],[0,fy,cy],[0,0,1]] (tasks/proc3d.py:221-222, proc3d.py:657)
        double u = ((k[0] * x0 + 0.0 * x1) + k[2] * x2) / x2;  // :658
        double w = ((0.0 * x0 + k[1] * x1) + k[3] * x2) / x2;
        double uf = u + 0.5, wf = w + 0.5;  // tasks/proc3d.py:224
        if (!(fabs(uf) < 9.0e15) || !(fabs(wf) < 9.0e15)) continue;  // NaN/inf: int() is out of range -> outside
        int64_t pu = (int64_t)uf, pv = (int64_t)wf;  // astype(int): toward zero
        if (pu >= 0 && pu < W && pv >= 0 && pv < H) {  // is_in_pict, :185-186
            for (int l = 0; l < L; ++l)
                scores[(int64_t)l * P + i] += (double)masks[(((int64_t)l * V + v) * H + pv) * W + pu];  // :229-230
        }
    }
    int best = 0;  // np.argmax: first maximum (:232)
    double bs = scores[i];
    for (int l = 1; l < L; ++l) {
        double s = scores[(int64_t)l * P + i];
        if (s > bs) { bs = s; best = l; }
    }
    labels[i] = best;
}

}  // namespace

extern "C" {

const char *sc_label_points_last_error(void) { return g_err.msg; }

int sc_label_points(const double *points, int64_t P, int L, int V, const double *K, const double *R,
                    const double *t, const void *masks, int masks_on_device, int H, int W, int device,
                    double *scores_out, int32_t *labels_out) {
    if (!points || !K || !R || !t || !masks || !scores_out || !labels_out)
        return g_err.fail(SC_ERR_INVALID, "null argument");
    if (P < 0 || L <= 0 || V < 0 || H <= 0 || W <= 0) return g_err.fail(SC_ERR_INVALID, "bad sizes");
    if (P == 0) return SC_OK;
    int rc = SC_OK;
    CallerDevice caller(device);  // put back when the call ends
    const size_t mbytes = (size_t)L * V * H * W, views = (size_t)(V ? V : 1);
    Layout lay;  // one allocation: points | K | R | t | scores | labels | the masks, where they come from the host
    const size_t pts_at = lay.take((size_t)P * 24), K_at = lay.take(views * 32), R_at = lay.take(views * 72),
                 t_at = lay.take(views * 24), sc_at = lay.take((size_t)L * P * 8), lab_at = lay.take((size_t)P * 4),
                 m_at = masks_on_device ? 0 : lay.take(mbytes ? mbytes : 1);
    char *base = nullptr;
    double *pts_d = nullptr, *K_d = nullptr, *R_d = nullptr, *t_d = nullptr, *sc_d = nullptr;
    int32_t *lab_d = nullptr;
    const void *m_d = masks;
    UNIT_TRY(hipSetDevice(device));
    UNIT_TRY(hipMalloc(reinterpret_cast<void **>(&base), lay.total));
    pts_d = reinterpret_cast<double *>(base + pts_at);
    K_d = reinterpret_cast<double *>(base + K_at);
    R_d = reinterpret_cast<double *>(base + R_at);
    t_d = reinterpret_cast<double *>(base + t_at);
    sc_d = reinterpret_cast<double *>(base + sc_at);
    lab_d = reinterpret_cast<int32_t *>(base + lab_at);
    UNIT_TRY(hipMemcpy(pts_d, points, (size_t)P * 24, hipMemcpyHostToDevice));
    if (V) {
        UNIT_TRY(hipMemcpy(K_d, K, (size_t)V * 32, hipMemcpyHostToDevice));
        UNIT_TRY(hipMemcpy(R_d, R, (size_t)V * 72, hipMemcpyHostToDevice));
        UNIT_TRY(hipMemcpy(t_d, t, (size_t)V * 24, hipMemcpyHostToDevice));
    }
    if (!masks_on_device) {
        m_d = base + m_at;
        if (mbytes) UNIT_TRY(hipMemcpy(base + m_at, masks, mbytes, hipMemcpyHostToDevice));
    }
    hipLaunchKernelGGL(label_points_kernel, dim3((uint32_t)((P + kB - 1) / kB)), dim3(kB), 0, nullptr, pts_d, P,
                       L, V, K_d, R_d, t_d, static_cast<const uint8_t *>(m_d), H, W, sc_d, lab_d);
    UNIT_TRY(hipGetLastError());
    UNIT_TRY(hipMemcpy(scores_out, sc_d, (size_t)L * P * 8, hipMemcpyDeviceToHost));
    UNIT_TRY(hipMemcpy(labels_out, lab_d, (size_t)P * 4, hipMemcpyDeviceToHost));
done:
    (void)hipDeviceSynchronize();
    if (base) (void)hipFree(base);
    return rc;
}

}  // extern "C"
