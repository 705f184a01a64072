// loc_lib_amd/csrc/ndt_ingest.hpp — the ingest front every NDT table is built from (ndt_kernels.hip: direct, ndt_pairs.hip: the
// voxel set, with a key of its own in front of the grouping half, ndt_inc.hip: incremental).
//
// point → key → stable radix sort → run heads → exclusive sum → run starts and the points in voxel order → per-voxel mean and scatter
// summed sequentially in input order. That sequence is why both tables carry the reference's bits (its per-voxel index list holds a
// voxel's points in input order, ndt cpp:97-103, and math::ComputeMeanAndCov adds them one after the other, math_utils.h:55-72), and
// why two ingests of one cloud give the same bits. It is written here once: a change to the summation order, the key range or the
// counters is a change to this file.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_buffer.hpp"
#include "ndt_kernels.hpp"

namespace locgpu {

// The counter block (ints on the device). run() zeroes all of it and its kernels write the first three; the rest is the caller's,
// for the kernels it puts behind the front (direct: voxels kept; incremental: new voxels, live slots collected).
enum { kIngRuns = 0, kIngBadKey = 1, kIngLastEmpty = 2, kIngUser = 3, kIngCtrs = 8 };

// Per-call scratch of the front, by points (a call has at most n runs, so the per-run arrays are as long). Grow-only; a local
// instance (the direct build) allocates per call and frees on return.
struct NdtIngest {
    DevBuf<unsigned long long> pkey, skey;  // keys by point, sorted
    DevBuf<unsigned long long> ukey;        // key of run u (with_masks)
    DevBuf<uint32_t> pidx, sidx;            // point index, in sorted order
    DevBuf<uint32_t> ustart;                // first sorted position of run u; ustart[runs] = n
    DevBuf<int> head, uid;                  // 1 at a run's first point; the run of every sorted point
    DevBuf<float4> psorted;                 // the points in voxel order, a voxel's points in input order
    DevBuf<unsigned char> keep;             // the caller's mask for run(masked = true) (with_masks)
    DevBuf<unsigned char> temp;             // scratch of the device-wide primitives
    DevBuf<int> ctr;                        // kIngCtrs counters

    size_t cap() const { return cap_; }
    // room for clouds of up to cap − 1 points; with_masks: ukey and keep too
    hipError_t reserve(size_t cap, bool with_masks);
    hipError_t ensure_temp(size_t bytes) { return bytes <= temp.cap() ? hipSuccess : temp.alloc(bytes + 256); }
    // keys → group(), enqueued on `s` (no synchronisation, no read-back). A point outside the ±2^20-voxel key
    // range raises ctr[kIngBadKey]; it, and with `masked` a point whose keep[i] == 0, gets kNdtEmpty and sorts into the last run.
    hipError_t run(const float4* d_pts, size_t n, double inv_voxel, bool masked, hipStream_t s);
    // The grouping half: sort → heads → scan → runs over the n keys in pkey, pidx[i] = the index in d_pts of the point behind key i.
    // Writes ctr[kIngRuns] and ctr[kIngLastEmpty] and no other counter. For a caller with a key of its own (the voxel set, ndt_pairs.hip).
    hipError_t group(const float4* d_pts, size_t n, hipStream_t s);

  private:
    size_t cap_ = 0;
};

// math::ComputeMeanAndCov's sums (math_utils.h:55-72) over the run psorted[b, e): the mean is the sequential sum in input order,
// then one division each; c = the six scatter sums (00 01 02 11 12 22) of the products, product first, then sum — never fused: the
// callers are compiled without contraction and must stay so. Each caller does its own /(n−1) and its own inverse.
__device__ __forceinline__ void ndt_mean_scatter(const float4* __restrict__ psorted, uint32_t b, uint32_t e, double (&m)[3], double (&c)[6]) {
    const uint32_t len = e - b;
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (uint32_t j = b; j < e; ++j) { const float4 p = psorted[j]; sx = sx + (double)p.x; sy = sy + (double)p.y; sz = sz + (double)p.z; }
    m[0] = sx / (double)len; m[1] = sy / (double)len; m[2] = sz / (double)len;
    double c00 = 0.0, c01 = 0.0, c02 = 0.0, c11 = 0.0, c12 = 0.0, c22 = 0.0;
    for (uint32_t j = b; j < e; ++j) {
        const float4 p = psorted[j];
        const double dx = (double)p.x - m[0], dy = (double)p.y - m[1], dz = (double)p.z - m[2];
        c00 += dx * dx; c01 += dx * dy; c02 += dx * dz; c11 += dy * dy; c12 += dy * dz; c22 += dz * dz;
    }
    c[0] = c00; c[1] = c01; c[2] = c02; c[3] = c11; c[4] = c12; c[5] = c22;
}

// Claims the table slot of `key` and returns it (keys are distinct: a first probe that finds the slot taken walks on). The caller
// writes the slot's record index.
__device__ __forceinline__ size_t ndt_claim_slot(NdtSlot* slots, unsigned long long key, size_t cap_mask) {
    size_t h = ndt_hash32(key, cap_mask);
    for (;;) {
        const unsigned long long prev = atomicCAS(&slots[h].key, kNdtEmpty, key);
        if (prev == kNdtEmpty) return h;
        h = (h + 1) & cap_mask;
    }
}

// The numerical rank of a voxel's covariance: 1e-14 ≈ 90·2^-53 is above the rounding of a few dozen points' sums and a decade below
// the smallest λ2/λ0 the voxel tests treat as full rank (1e-13). The CPU checker's ClampedInfo carries the same constant.
constexpr double kNdtNoiseRatio = 1e-14;

// One kept voxel of a DIRECT table, the run psorted[b, e) under `key`: math::ComputeMeanAndCov's sums (ndt_mean_scatter), Σ/(n−1),
// one-sided Jacobi SVD, λ1,λ2 clamped to ≥ 1e-3·λ0, info = V diag(1/λ) Uᵀ (ndt cpp:111-130) — then claim() takes the voxel's table
// slot and returns the index of its record, which is written. The single-target build (ndt_kernels.hip) and the voxel-set build
// (ndt_pairs.hip) differ in claim() alone, so a voxel has the same bits in both.
template <class Claim>
__device__ __forceinline__ void ndt_voxel_record(unsigned long long key, const float4* psorted, uint32_t b, uint32_t e, NdtRecord* rec, Claim claim) {
    const uint32_t len = e - b;
    double mu[3], c[6];
    ndt_mean_scatter(psorted, b, e, mu, c);
    const double mx = mu[0], my = mu[1], mz = mu[2];
    const double len1 = (double)(len - 1);
    const double sxx = c[0] / len1, sxy = c[1] / len1, sxz = c[2] / len1, syy = c[3] / len1, syz = c[4] / len1, szz = c[5] / len1;
    double a[3][3] = {{sxx, sxy, sxz}, {sxy, syy, syz}, {sxz, syz, szz}};  // columns of the symmetric Σ
    double vv[3][3];
    jacobi_svd_onesided<3, 3>(a, vv);
    double sv[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) sv[k] = sqrt(a[k][0] * a[k][0] + a[k][1] * a[k][1] + a[k][2] * a[k][2]);
    // order by descending singular value (stable, like std::sort on three keys with > comparator)
    int o0 = 0, o1 = 1, o2 = 2;
    if (sv[o1] > sv[o0]) { const int t = o0; o0 = o1; o1 = t; }
    if (sv[o2] > sv[o1]) { const int t = o1; o1 = o2; o2 = t; }
    if (sv[o1] > sv[o0]) { const int t = o0; o0 = o1; o1 = t; }
    const int ord[3] = {o0, o1, o2};
    // A singular value at or below kNdtNoiseRatio·λ0 is rounding noise of the sums and so is its column of a: it carries no
    // direction, and two such columns need not even be orthogonal to each other. There U takes V's column, which is exact to
    // rounding (Σ is symmetric PSD: U = V), as it always did for a column of exact zeros. Voxels with λ2 ≥ 1e-13·λ0 never get here.
    const double noise = kNdtNoiseRatio * sv[o0];
    double lam[3], U[3][3], V[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int cidx = ord[k];
        lam[k] = cidx == 0 ? sv[0] : (cidx == 1 ? sv[1] : sv[2]);
#pragma unroll
        for (int r = 0; r < 3; ++r) {
            const double vr = cidx == 0 ? vv[0][r] : (cidx == 1 ? vv[1][r] : vv[2][r]);
            const double ar = cidx == 0 ? a[0][r] : (cidx == 1 ? a[1][r] : a[2][r]);
            V[k][r] = vr;
            U[k][r] = lam[k] > noise ? ar / lam[k] : vr;
        }
    }
    if (lam[1] < lam[0] * 1e-3) lam[1] = lam[0] * 1e-3;
    if (lam[2] < lam[0] * 1e-3) lam[2] = lam[0] * 1e-3;
    const unsigned int vid = claim();
    NdtRecord& R = rec[vid];
    R.key = key;
    R.mu[0] = mx; R.mu[1] = my; R.mu[2] = mz;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int cc = 0; cc < 3; ++cc) {
            double s = 0.0;
#pragma unroll
            for (int k = 0; k < 3; ++k) s += V[k][r] * (1.0 / lam[k]) * U[k][cc];
            R.info[3 * r + cc] = s;
        }
}

// every slot of a table to its empty value
template <class T>
__global__ void ndt_fill_kernel(T* p, size_t n, T v) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

}  // namespace locgpu
