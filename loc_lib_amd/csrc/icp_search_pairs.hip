// loc_lib_amd/csrc/icp_search_pairs.hip — the search stage over a forest target (locgpu_icp_set_target_forest): every scan of the batch
// is searched in a tree of its own. The trees lie behind one another in one array (kdtree_build.hpp, PackedForest), each with local
// slot indices and its root at local slot 0, so a scan's walk is the ordinary one on `tree + base` and only the slots it reports are
// rebased — the fit, accumulate and solve kernels read absolute slots of the one array and do not change.
//
// This is the one-thread-per-query exact traversal (icp_search_kernel<K, D, false>'s shape), not the walk / deep / redo passes of
// icp_search.hip: those share a descent across a wave, i.e. assume one root per wave and one buffer resource per launch.
#include "icp_kernels.hpp"
#include "launch.hpp"
#include "search_dispatch.hpp"

namespace locgpu {

// Grid (ceil(max_n/256), n_scans or n_active). scan_base[scan]: first slot of the scan's tree (even; a scan that is `done` from the
// start — no target — never reads its entry).
template <int KMAX, int D>
__global__ __launch_bounds__(kBlock) void icp_search_pairs_kernel(const uint2* __restrict__ tree, const uint32_t* __restrict__ scan_base,
                                                                  const float4* __restrict__ src, const int* __restrict__ counts,
                                                                  const PoseState* __restrict__ st, uint32_t* __restrict__ nn, size_t nn_pitch, int max_n,
                                                                  int k, float alpha_eff, int skip_nonfinite, const int* __restrict__ active,
                                                                  const int* __restrict__ src_of) {
    __shared__ uint32_t s_far[D][kBlock];
    __shared__ float s_d2[D][kBlock];
    const int scan = active ? active[blockIdx.y] : (int)blockIdx.y;
    if (st[scan].done) return;
    const int tid = threadIdx.x;
    const int i = blockIdx.x * kBlock + tid;
    if (i >= counts[scan]) return;
    const size_t gi = (size_t)scan * max_n + i;
    const float4 p = src[src_index(src_of, scan, max_n, i)];
    const uint32_t base = scan_base[scan];  // uniform over the block
    uint32_t out[KMAX];
    int cnt = 0;
    uint32_t nvis = 0, lvis = 0;
    const bool finite = !skip_nonfinite || (isfinite(p.x) && isfinite(p.y) && isfinite(p.z));  // pcl::isFinite, icp cpp:64 (P2P only)
    if (finite) {
        const D3 qs = se3_apply(st[scan].q, st[scan].t, D3{(double)p.x, (double)p.y, (double)p.z});
        KnnHeap<KMAX> heap;
        tree_knn_flat<KMAX, D, false>(tree + base, (float)qs.x, (float)qs.y, (float)qs.z, k, alpha_eff, s_far, s_d2, tid, heap, nvis, lvis);
        heap_to_sorted<KMAX>(heap, out, cnt);
    } else {
#pragma unroll
        for (int j = 0; j < KMAX; ++j) out[j] = kInvalidSlot;
    }
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < k) nn[(size_t)j * nn_pitch + gi] = out[j] == kInvalidSlot ? kInvalidSlot : out[j] + base;  // local → absolute
}

bool launch_icp_search_pairs(const SearchArgs& a, hipStream_t s) {
    return with_k<false>(a.k, [&](auto Kc) {
        return with_depth(a.depth, [&](auto Dc) {
            dim3 grid((a.max_n + kBlock - 1) / kBlock, a.active ? a.n_active : a.n_scans);
            hipLaunchKernelGGL((icp_search_pairs_kernel<decltype(Kc)::value, decltype(Dc)::value>), grid, dim3(kBlock), 0, s, a.tree, a.scan_tree_base, a.src,
                               a.counts, a.st, a.nn, a.nn_pitch, a.max_n, a.k, a.alpha_eff, a.skip_nonfinite, a.active, a.src_of);
        });
    });
}

}  // namespace locgpu
