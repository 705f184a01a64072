// loc_lib_amd/csrc/map_planes.hip — the per-map-point plane table of LOCGPU_P2PLANE_MAP: one math::FitPlane
// (math_utils.h:112-136) per KD-tree leaf at ingest instead of one per query and iteration (icp_registration.cpp:161-213).
//
// Shape of the ingest: the leaves are taken in chunks, in the tree's preorder (spatially coherent). Per chunk
//   map_plane_queries_kernel   the leaves' own float32 coordinates become the source points of a one-scan search batch;
//   launch_icp_search          the existing search stage, k = 5, alpha_eff = 1 (the exact walk with its deep pass and tie redo — no
//                              new instantiation of the walk) under the identity pose, which leaves the coordinates as they are;
//   map_plane_fit_kernel       one thread per leaf: the five neighbours in FP64, plane_null_vector_secular with its fall-back and
//                              the 1e-2 validity rule, exactly as icp_plane_accum_kernel applies them; one 32-byte row per leaf.
// Table layout: a leaf occupies two consecutive tree slots, so slot >> 1 is unique per leaf; row slot >> 1 = the FP64 4-vector n4
// (not normalised beyond what the SVD gives: the reference's normal is not unit either). A row that is no leaf's, or whose plane is
// invalid, holds four NaNs: the accumulate kernel needs one dependent 32-byte gather and no leaf load.
#include "icp_kernels.hpp"
#include "launch.hpp"

namespace locgpu {

// The chunk's queries: src[i] = coordinates of leaf first + i; counts[0] = n (the search batch has one scan).
__global__ __launch_bounds__(kBlock) void map_plane_queries_kernel(const uint2* __restrict__ tree, const uint32_t* __restrict__ leaf_slots, size_t first, int n,
                                                                   float4* __restrict__ src, int* __restrict__ counts) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i == 0) counts[0] = n;
    if (i >= n) return;
    uint4 w;
    __builtin_memcpy(&w, tree + leaf_slots[first + i], 16);
    src[i] = float4{as_f32(w.x), as_f32(w.z), as_f32(w.w), 0.f};
}

// nn: the search stage's lists of the chunk, [5][nn_pitch] leaf slots in ascending distance. n_valid: number of valid planes (an
// integer count, one atomic per wave; the rows themselves are written without atomics).
__global__ __launch_bounds__(kBlock) void map_plane_fit_kernel(const uint2* __restrict__ tree, const uint32_t* __restrict__ leaf_slots, size_t first, int n,
                                                               const uint32_t* __restrict__ nn, size_t nn_pitch, double4* __restrict__ planes,
                                                               unsigned long long* __restrict__ n_valid) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    bool valid = false;
    if (i < n) {
        uint32_t slot[5];
#pragma unroll
        for (int j = 0; j < 5; ++j) slot[j] = __builtin_nontemporal_load(&nn[(size_t)j * nn_pitch + i]);
        const double nan = __builtin_nan("");
        double4 row{nan, nan, nan, nan};
        if (slot[4] != kInvalidSlot) {  // k = 5 yields 5 or (k > size_) none
            D3 nb[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) nb[j] = leaf_point(tree, slot[j]);
            double n4[4];
            if (!plane_null_vector_secular(nb, n4)) plane_null_vector(nb, n4);
            const D3 n3{n4[0], n4[1], n4[2]};
            bool fit = true;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const double err = dot3(n3, nb[j]) + n4[3];
                if (err * err > 1e-2) fit = false;
            }
            // NaN is the table's "no plane" mark: a plane with a non-finite coefficient (non-finite map coordinates) is none
            valid = fit && isfinite(n4[0]) && isfinite(n4[1]) && isfinite(n4[2]) && isfinite(n4[3]);
            if (valid) row = double4{n4[0], n4[1], n4[2], n4[3]};
        }
        planes[leaf_slots[first + i] >> 1] = row;
    }
    const unsigned long long m = __ballot(valid);
    if (m && (threadIdx.x & 63) == 0) atomicAdd(n_valid, (unsigned long long)__popcll(m));
}

// Debug / test read-back: rows by ORIGINAL point index. out_n4 and out_valid are zeroed by the caller (a point that is no leaf stays invalid).
__global__ __launch_bounds__(kBlock) void map_plane_dump_kernel(const uint2* __restrict__ tree, const uint32_t* __restrict__ leaf_slots, size_t n_leaves,
                                                                const double4* __restrict__ planes, size_t n_points, double* __restrict__ out_n4,
                                                                unsigned char* __restrict__ out_valid) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n_leaves) return;
    const uint32_t slot = leaf_slots[i];
    const size_t orig = tree[slot].y & 0x3FFFFFFFu;
    if (orig >= n_points) return;
    const double4 r = planes[slot >> 1];
    if (r.x == r.x) {
        out_n4[4 * orig + 0] = r.x; out_n4[4 * orig + 1] = r.y; out_n4[4 * orig + 2] = r.z; out_n4[4 * orig + 3] = r.w;
        out_valid[orig] = 1;
    }
}

void launch_map_plane_queries(const uint2* tree, const uint32_t* leaf_slots, size_t first, int n, float4* src, int* counts, hipStream_t s) {
    hipLaunchKernelGGL(map_plane_queries_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, tree, leaf_slots, first, n, src, counts);
}

void launch_map_plane_fit(const uint2* tree, const uint32_t* leaf_slots, size_t first, int n, const uint32_t* nn, size_t nn_pitch, double* planes,
                          unsigned long long* n_valid, hipStream_t s) {
    hipLaunchKernelGGL(map_plane_fit_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, tree, leaf_slots, first, n, nn, nn_pitch,
                       reinterpret_cast<double4*>(planes), n_valid);
}

void launch_map_plane_dump(const uint2* tree, const uint32_t* leaf_slots, size_t n_leaves, const double* planes, size_t n_points, double* out_n4,
                           unsigned char* out_valid, hipStream_t s) {
    hipLaunchKernelGGL(map_plane_dump_kernel, dim3((unsigned)((n_leaves + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, tree, leaf_slots, n_leaves,
                       reinterpret_cast<const double4*>(planes), n_points, out_n4, out_valid);
}

}  // namespace locgpu
