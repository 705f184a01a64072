// loc_lib_amd/csrc/loam_stream.hip — the output cloud of LoamRegistration::ScanMatch on resident clouds
// (locgpu_loam_scan_match_cloud, loam_align.hip): written where a locgpu_cloud holds its points, never staged on the host.
#include "icp_kernels.hpp"
#include "launch.hpp"

namespace locgpu {

// *cloud += *edge; *cloud += *surf; pcl::transformPointCloud(*cloud, *result, pose.matrix().cast<float>()) (loam_registration.cpp:93-96)
// in one pass: output point i is edge point i for i < n_edge, surface point i − n_edge after that; x, y, z as transform_cloud_kernel
// (icp_fit.hip) rounds them — ((m0·x + m1·y) + m2·z) + m3 per row, what locgpu_loam_scan_match's host output holds — and the w lane
// (the intensity) carried through. One 16-byte load and one 16-byte store per thread; `out` overlaps neither input.
__global__ __launch_bounds__(kBlock) void loam_join_transform_kernel(const float4* __restrict__ edge, uint32_t n_edge, const float4* __restrict__ surf,
                                                                     uint32_t n_surf, M12f m, float4* __restrict__ out) {
    const uint32_t i = blockIdx.x * (uint32_t)kBlock + threadIdx.x;
    if (i >= n_edge + n_surf) return;
    const float4 p = i < n_edge ? edge[i] : surf[i - n_edge];
    const float* m12 = m.v;
    float4 q;
    q.x = ((m12[0] * p.x + m12[1] * p.y) + m12[2] * p.z) + m12[3];
    q.y = ((m12[4] * p.x + m12[5] * p.y) + m12[6] * p.z) + m12[7];
    q.z = ((m12[8] * p.x + m12[9] * p.y) + m12[10] * p.z) + m12[11];
    q.w = p.w;
    out[i] = q;
}

// n_edge + n_surf <= 0x7FFFFF00 (a cloud's limit): the index fits 32 bits and the grid 2^23 blocks.
void launch_loam_join_transform(const float4* edge, size_t n_edge, const float4* surf, size_t n_surf, const M12f& m12, float4* out, hipStream_t s) {
    const size_t n = n_edge + n_surf;
    if (n == 0) return;
    hipLaunchKernelGGL(loam_join_transform_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, edge, (uint32_t)n_edge, surf, (uint32_t)n_surf, m12, out);
}

}  // namespace locgpu
