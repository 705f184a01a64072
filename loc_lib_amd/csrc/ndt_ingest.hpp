// loc_lib_amd/csrc/ndt_ingest.hpp — the ingest front both NDT tables are built from (ndt_kernels.hip: direct, ndt_inc.hip: incremental).
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
    // keys → sort → heads → scan → runs, enqueued on `s` (no synchronisation, no read-back). A point outside the ±2^20-voxel key
    // range raises ctr[kIngBadKey]; it, and with `masked` a point whose keep[i] == 0, gets kNdtEmpty and sorts into the last run.
    hipError_t run(const float4* d_pts, size_t n, double inv_voxel, bool masked, hipStream_t s);

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

// every slot of a table to its empty value
template <class T>
__global__ void ndt_fill_kernel(T* p, size_t n, T v) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) p[i] = v;
}

}  // namespace locgpu
