// loc_lib_amd/csrc/pose_interp.hpp — math::PoseInterp on the device (LocUtils/include/LocUtils/common/math_utils.h:470-517): the one copy
// of the slerp and of the matrix made of it, shared by the per-column deskew of the range-image ingest (range_ingest.hip,
// rd_pose_kernel), the per-point deskew of the point-record ingest (record_ingest.hip, rec_scatter_kernel) and the pass over a resident
// batch (resident_deskew.hip, rsd_move_kernel).
#pragma once
#include <hip/hip_runtime.h>

#include <cfloat>

#include "cloud_filters.hpp"
#include "device_math.hpp"

namespace locgpu {

constexpr int kMaxKnots = 256;
constexpr double kInterpTimeTh = 0.5;  // PoseInterp's time_th, math_utils.h:471

// math::PoseInterp (math_utils.h:470-517) on the K knots staged in LDS, t[K] and p[K][7] (quaternion xyzw, translation): the pose at
// time q. The times increase strictly, so the first interval with t[j] < q <= t[j+1] is found by bisection. Everything but acos and
// sin is one IEEE double operation per line of the header's definition (the build compiles with contraction off).
__device__ __forceinline__ void rd_pose_at(const double* t, const double* p, int K, double q, double (&out)[7]) {
    if (q > t[K - 1]) {  // :478-483, the caller has refused anything later than time_th behind the last knot
#pragma unroll
        for (int i = 0; i < 7; ++i) out[i] = p[7 * (K - 1) + i];
        return;
    }
    int lo = 0, hi = K;  // the number of knots with t < q
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (t[mid] < q) lo = mid + 1; else hi = mid;
    }
    const int j = lo > 0 ? lo - 1 : 0;  // q <= t[K-1]: lo <= K - 1, so j + 1 <= K - 1
    const double* a = p + 7 * j;
    const double* b = a + 7;
    const double dt = t[j + 1] - t[j];
    if (fabs(dt) < 1e-6) {  // :505-508
#pragma unroll
        for (int i = 0; i < 7; ++i) out[i] = a[i];
        return;
    }
    const double s = (q - t[j]) / dt;
    // Eigen's QuaternionBase::slerp (:513)
    const double d = ((a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]) + a[3] * b[3];
    const double ad = fabs(d);
    double s0, s1;
    if (ad >= 1.0 - DBL_EPSILON) {
        s0 = 1.0 - s;
        s1 = s;
    } else {
        const double th = acos(ad), st = sin(th);
        s0 = sin((1.0 - s) * th) / st;
        s1 = sin(s * th) / st;
    }
    if (d < 0.0) s1 = -s1;
#pragma unroll
    for (int i = 0; i < 4; ++i) out[i] = s0 * a[i] + s1 * b[i];
    const double u = 1.0 - s;
#pragma unroll
    for (int i = 4; i < 7; ++i) out[i] = a[i] * u + b[i] * s;  // :514
}

// The reference-time pose of a scan as the matrix rule reads it: ref[0..8] = R_r (Eigen's toRotationMatrix), ref[9..11] = t_r.
__device__ __forceinline__ void rd_ref_pose(const double* t, const double* p, int K, double ref_time, double* ref) {
    double pr[7];
    rd_pose_at(t, p, K, ref_time, pr);
    quat_to_R(pr, ref);
    ref[9] = pr[4];
    ref[10] = pr[5];
    ref[11] = pr[6];
}

// M = [ R_rᵀ·R_q | R_rᵀ·(t_q − t_r) ] of the pose pq against the reference pose `ref` (rd_ref_pose), row-major 3×4, every dot product
// summed left to right.
__device__ __forceinline__ void rd_matrix(const double* ref, const double (&pq)[7], double* m) {
    double Rq[9];
    quat_to_R(pq, Rq);
    const double d0 = pq[4] - ref[9], d1 = pq[5] - ref[10], d2 = pq[6] - ref[11];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const double a0 = ref[r], a1 = ref[3 + r], a2 = ref[6 + r];  // column r of R_r = row r of R_rᵀ
        m[4 * r + 0] = (a0 * Rq[0] + a1 * Rq[3]) + a2 * Rq[6];
        m[4 * r + 1] = (a0 * Rq[1] + a1 * Rq[4]) + a2 * Rq[7];
        m[4 * r + 2] = (a0 * Rq[2] + a1 * Rq[5]) + a2 * Rq[8];
        m[4 * r + 3] = (a0 * d0 + a1 * d1) + a2 * d2;
    }
}

// One survivor of a scan moved into the reference frame at its OWN time tp: the pose at tp on the knots staged in LDS, its matrix m
// against the scan's reference pose `ref` (rd_ref_pose), and the point as locgpu_cloud_transform's arithmetic gives it (every
// survivor is finite). The one copy of the per-point deskew: the store loop of the point-record ingest (record_ingest.hip,
// rec_scatter_kernel<true>) and the pass over a resident batch (resident_deskew.hip, rsd_move_kernel) both call it.
__device__ __forceinline__ float4 rd_move_point(const double* t, const double* p, int K, const double* ref, double tp, const float4& pt, double (&m)[12]) {
    double pq[7];
    rd_pose_at(t, p, K, tp, pq);
    rd_matrix(ref, pq, m);
    return transform_point_f64(pt, m, true);
}

}  // namespace locgpu
