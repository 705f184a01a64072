// loc_lib_amd/csrc/ndt_ingest.hip — kernels and host sequencing of the NDT ingest front (ndt_ingest.hpp).
#include "ndt_ingest.hpp"

#include <algorithm>

#include "device_prims.hpp"
#include "icp_kernels.hpp"

namespace locgpu {

// key of every point ((pt * inv_voxel_size_).cast<int>(), ndt cpp:100,154: truncation toward zero); kNdtEmpty for a point outside the
// ±2^20-voxel range (reported) or masked out (keep[i] == 0)
__global__ __launch_bounds__(kBlock) void ndt_key_kernel(const float4* __restrict__ pts, size_t n, double inv, const unsigned char* __restrict__ keep,
                                                         unsigned long long* __restrict__ pkey, uint32_t* __restrict__ pidx, int* __restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 p = pts[i];
    int kx, ky, kz;
    ndt_key_of(D3{(double)p.x, (double)p.y, (double)p.z}, inv, kx, ky, kz);
    unsigned long long key = kNdtEmpty;
    if (!ndt_key_in_range(kx, ky, kz)) ctr[kIngBadKey] = 1;
    else if (!keep || keep[i]) key = ndt_pack(kx, ky, kz);
    pkey[i] = key;
    pidx[i] = (uint32_t)i;
}

// sorted keys → 1 at the first point of every run
__global__ __launch_bounds__(kBlock) void ndt_head_kernel(const unsigned long long* __restrict__ skey, size_t n, int* __restrict__ head) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || skey[i] != skey[i - 1]) ? 1 : 0;
}

// run u: first sorted position and (ukey != nullptr) key; ustart[runs] = n; the number of runs; whether the last run is the kNdtEmpty
// run; the points in voxel order
__global__ __launch_bounds__(kBlock) void ndt_runs_kernel(const unsigned long long* __restrict__ skey, const uint32_t* __restrict__ sidx, const int* __restrict__ head,
                                                          const int* __restrict__ uid, size_t n, const float4* __restrict__ pts,
                                                          unsigned long long* __restrict__ ukey, uint32_t* __restrict__ ustart, float4* __restrict__ psorted,
                                                          int* __restrict__ ctr) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    psorted[i] = pts[sidx[i]];
    if (head[i]) {
        if (ukey) ukey[uid[i]] = skey[i];
        ustart[uid[i]] = (uint32_t)i;
    }
    if (i == n - 1) {
        const int runs = uid[i] + head[i];
        ustart[runs] = (uint32_t)n;
        ctr[kIngRuns] = runs;
        ctr[kIngLastEmpty] = skey[i] == kNdtEmpty ? 1 : 0;
    }
}

hipError_t NdtIngest::reserve(size_t cap, bool with_masks) {
    LOCGPU_TRY(ctr.reserve(kIngCtrs));
    if (cap > cap_) {
        cap_ = 0;
        LOCGPU_TRY(pkey.alloc(cap)); LOCGPU_TRY(skey.alloc(cap));
        LOCGPU_TRY(pidx.alloc(cap)); LOCGPU_TRY(sidx.alloc(cap)); LOCGPU_TRY(ustart.alloc(cap));
        LOCGPU_TRY(head.alloc(cap)); LOCGPU_TRY(uid.alloc(cap));
        LOCGPU_TRY(psorted.alloc(cap));
        size_t b1 = 0, b2 = 0;
        LOCGPU_TRY(prim::sort_pairs(nullptr, b1, pkey.get(), skey.get(), pidx.get(), sidx.get(), cap, 0, 64, nullptr));
        LOCGPU_TRY(prim::exclusive_sum(nullptr, b2, head.get(), uid.get(), cap, nullptr));
        LOCGPU_TRY(ensure_temp(std::max(b1, b2)));
        cap_ = cap;
    }
    if (with_masks) { LOCGPU_TRY(ukey.reserve(cap_)); LOCGPU_TRY(keep.reserve(cap_)); }  // also when an earlier call reserved without them
    return hipSuccess;
}

hipError_t NdtIngest::run(const float4* d_pts, size_t n, double inv_voxel, bool masked, hipStream_t s) {
    if (n + 1 > cap_ || (masked && keep.cap() < n)) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
    LOCGPU_TRY(hipMemsetAsync(ctr, 0, kIngCtrs * sizeof(int), s));
    hipLaunchKernelGGL(ndt_key_kernel, dim3(grid), dim3(kBlock), 0, s, d_pts, n, inv_voxel, masked ? keep.get() : nullptr, pkey, pidx, ctr);
    return group(d_pts, n, s);
}

hipError_t NdtIngest::group(const float4* d_pts, size_t n, hipStream_t s) {
    if (n + 1 > cap_) return hipErrorInvalidValue;
    const unsigned grid = (unsigned)((n + kBlock - 1) / kBlock);
    size_t tb = temp.cap();
    LOCGPU_TRY(prim::sort_pairs(temp, tb, pkey.get(), skey.get(), pidx.get(), sidx.get(), n, 0, 64, s));  // stable: a voxel's points keep their input order
    hipLaunchKernelGGL(ndt_head_kernel, dim3(grid), dim3(kBlock), 0, s, skey, n, head);
    tb = temp.cap();
    LOCGPU_TRY(prim::exclusive_sum(temp, tb, head.get(), uid.get(), n, s));
    hipLaunchKernelGGL(ndt_runs_kernel, dim3(grid), dim3(kBlock), 0, s, skey, sidx, head, uid, n, d_pts, ukey, ustart, psorted, ctr);
    return hipSuccess;
}

}  // namespace locgpu
