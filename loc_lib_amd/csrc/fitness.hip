// loc_lib_amd/csrc/fitness.hip — the fitness score of an alignment (MatchingInterface::GetFitnessScore, matching_interface.h:53; the
// quantity pcl::Registration::getFitnessScore reports): mean squared distance from the transformed source points to their EXACT
// nearest target points, over the points within max_range.
//
// Shape: the existing search stage (launch_icp_search, k = 1, alpha_eff = 1: the exact walk of search_walk.hpp, with its deep pass and
// its tie redo — no new instantiation of the walk) leaves one leaf slot per point in the batch's neighbour list; the accumulate kernel
// below re-forms the float32 query and the float32 squared distance exactly as the walk evaluates it, and reduces {Σd², inliers,
// finite points} in FP64 per block — the accumulators' scheme, spelled out in the kernel (it says why); a last small kernel
// adds the block rows of a scan in a fixed order (fixed_order_row_sum below, also the joint LOAM score's). No atomics on the sums,
// two runs give the same bits. A fused
// walk + reduce kernel was not built: the walk retires lanes to the deep pass and the redo kernel, so a fused reduction would have
// to live in three kernels; the separate pass costs one 4-byte load per point.
//
// The split of the sums is FIXED (kFitPts points per thread, rows added in the order of fixed_order_row_sum) and does not depend on
// the batch: a scan scores the same bits alone, in a batch of any size and in any chunk of a candidate search.
#include "icp_kernels.hpp"
#include "launch.hpp"

namespace locgpu {

constexpr int kFitPts = 4;  // points per thread of the accumulate kernel: a block covers 1024 consecutive points of its scan

__global__ __launch_bounds__(kBlock) void icp_fitness_accum_kernel(const uint2* __restrict__ tree, const float4* __restrict__ src,
                                                                   const int* __restrict__ counts, const PoseState* __restrict__ st,
                                                                   const uint32_t* __restrict__ nn, int max_n, float gate2,
                                                                   double* __restrict__ partials, const int* __restrict__ src_of) {
    __shared__ double s_part[kBlock / 64][kFitW];
    const int scan = blockIdx.y;
    const int n = counts[scan];
    const size_t region = (size_t)(src_of ? src_of[scan] : scan) * max_n;
    double sum = 0.0, inl = 0.0, fin = 0.0;
#pragma unroll
    for (int pp = 0; pp < kFitPts; ++pp) {
        const int i = (blockIdx.x * kFitPts + pp) * kBlock + threadIdx.x;
        if (i < n) {
            const float4 p = src[region + i];
            const uint32_t s0 = __builtin_nontemporal_load(&nn[(size_t)scan * max_n + i]);
            // a point with a non-finite coordinate is not a query (the search left it the empty list) and is not counted
            if (isfinite(p.x) && isfinite(p.y) && isfinite(p.z) && s0 != kInvalidSlot) {
                const D3 qs = se3_apply(st[scan].q, st[scan].t, D3{(double)p.x, (double)p.y, (double)p.z});
                const float qx = (float)qs.x, qy = (float)qs.y, qz = (float)qs.z;  // the query of the alignment (icp_registration.cpp:169-170)
                uint4 w;
                __builtin_memcpy(&w, tree + s0, 16);
                const float dx = qx - as_f32(w.x), dy = qy - as_f32(w.z), dz = qz - as_f32(w.w);
                const float d2 = dx * dx + (dy * dy + dz * dz);  // as the walk evaluates it (search_walk.hpp; no contraction: -ffp-contract=off)
                fin += 1.0;
                if (d2 <= gate2) { sum += (double)d2; inl += 1.0; }
            }
        }
    }
    // block_reduce_store's scheme (icp_kernels.hpp) with the three butterflies side by side and one guarded store: through the shared
    // function, which finishes and stores one value before the next, the score call measured 0.7 % slower (profiles/ndt_shared_front.md)
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    sum = wave_sum(sum); inl = wave_sum(inl); fin = wave_sum(fin);
    if (lane == 0) { s_part[wave][0] = sum; s_part[wave][1] = inl; s_part[wave][2] = fin; }
    __syncthreads();
    if (threadIdx.x < 3) {
        double t = s_part[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kBlock / 64; ++w) t += s_part[w][threadIdx.x];
        partials[((size_t)scan * gridDim.x + blockIdx.x) * kFitW + threadIdx.x] = t;
    }
}

// The fixed-order sum of the block rows p[rows][kFitW] by one wave: lane l adds rows l, l + 64, … in order, then lane c < 3 adds the 64
// lane sums of column c in order and returns the total (other lanes: 0). Rows that do not exist count as zeros, so the result does not
// depend on how many rows the batch's longest scan needs. Every lane of the wave must call it (barrier inside); a second call needs a
// barrier in front of it: s_lane is still being read.
__device__ __forceinline__ double fixed_order_row_sum(const double* __restrict__ p, int rows, int lane, double (&s_lane)[3][64]) {
    double a = 0.0, b = 0.0, c = 0.0;
    for (int r = lane; r < rows; r += 64) {
        a += p[(size_t)r * kFitW + 0];
        b += p[(size_t)r * kFitW + 1];
        c += p[(size_t)r * kFitW + 2];
    }
    s_lane[0][lane] = a; s_lane[1][lane] = b; s_lane[2][lane] = c;
    __syncthreads();
    double t = 0.0;
    if (lane < 3) {
        t = s_lane[lane][0];
        for (int l = 1; l < 64; ++l) t += s_lane[lane][l];
    }
    return t;
}

// One wave per scan: out[scan] = {Σd², inliers, finite points, 0}, the block rows added by fixed_order_row_sum.
// list_counts: the search stage's work-list counters, consumed by now — zeroed for the next search (as gn_solve_kernel does).
__global__ __launch_bounds__(64) void icp_fitness_sum_kernel(const double* __restrict__ partials, int rows, double* __restrict__ out,
                                                             unsigned int* __restrict__ list_counts) {
    __shared__ double s_lane[3][64];
    const int scan = blockIdx.x, lane = threadIdx.x;
    if (list_counts && blockIdx.x == 0 && lane < 4) list_counts[lane] = 0u;
    const double t = fixed_order_row_sum(partials + (size_t)scan * rows * kFitW, rows, lane, s_lane);
    if (lane < 4) out[(size_t)scan * kFitW + lane] = t;  // lane 3: 0
}

// The joint score of the LOAM matcher (loam_align.hip): one wave per candidate adds the surface batch's rows, then the edge batch's —
// each class with fixed_order_row_sum, the sum icp_fitness_sum_kernel is, with its own rows per scan — so out[cand][1 + c] holds the
// bits locgpu_icp_fitness gives for class c, and out[cand][0] = surface + edge formed from those UN-ROUNDED class sums (surface first),
// not from two means. partials[c] == nullptr: the class is switched off and adds zeros. out[cand][3][kFitW] = {Σd², inliers, finite
// points, 0} of joint, surface, edge. list_counts[c]: the class batch's search work-list counters, consumed by now — zeroed for the
// next search (as loam_solve_kernel does). No atomics.
__global__ __launch_bounds__(64) void loam_fitness_sum_kernel(const double* __restrict__ part_surf, int rows_surf, const double* __restrict__ part_edge,
                                                              int rows_edge, double* __restrict__ out, unsigned int* __restrict__ counts_surf,
                                                              unsigned int* __restrict__ counts_edge) {
    __shared__ double s_lane[3][64];
    const int cand = blockIdx.x, lane = threadIdx.x;
    if (blockIdx.x == 0 && lane < 4) {
        if (counts_surf) counts_surf[lane] = 0u;
        if (counts_edge) counts_edge[lane] = 0u;
    }
    double* o = out + (size_t)cand * 3 * kFitW;
    double joint = 0.0;  // lanes 0..2: Σ, inliers, finite points of both classes
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const double* part = c == 0 ? part_surf : part_edge;
        const int rows = part ? (c == 0 ? rows_surf : rows_edge) : 0;
        if (c == 1) __syncthreads();  // the surface class's lane sums have been read
        const double t = fixed_order_row_sum(part + (size_t)cand * rows * kFitW, rows, lane, s_lane);  // part is not read when rows == 0
        if (lane < 4) o[(1 + c) * kFitW + lane] = t;
        joint += t;
    }
    if (lane < 4) o[lane] = joint;
}

int icp_fitness_rows(int max_n) { return (max_n + kFitPts * kBlock - 1) / (kFitPts * kBlock); }

void launch_fitness_sum(const double* partials, int rows, int n_scans, double* out, unsigned int* list_counts, hipStream_t s) {
    hipLaunchKernelGGL(icp_fitness_sum_kernel, dim3(n_scans), dim3(64), 0, s, partials, rows, out, list_counts);
}

int launch_icp_fitness_accum(const FitnessArgs& a, hipStream_t s) {
    const int rows = icp_fitness_rows(a.max_n);
    hipLaunchKernelGGL(icp_fitness_accum_kernel, dim3(rows, a.n_scans), dim3(kBlock), 0, s, a.tree, a.src, a.counts, a.st, a.nn, a.max_n, a.gate2, a.partials,
                       a.src_of);
    return rows;
}

void launch_icp_fitness(const FitnessArgs& a, hipStream_t s) {
    const int rows = launch_icp_fitness_accum(a, s);
    launch_fitness_sum(a.partials, rows, a.n_scans, a.out, a.list_counts, s);
}

void launch_loam_fitness_sum(const double* const partials[2], const int rows[2], int n_cands, double* out, unsigned int* const list_counts[2], hipStream_t s) {
    hipLaunchKernelGGL(loam_fitness_sum_kernel, dim3(n_cands), dim3(64), 0, s, partials[0], rows[0], partials[1], rows[1], out, list_counts[0], list_counts[1]);
}

}  // namespace locgpu
