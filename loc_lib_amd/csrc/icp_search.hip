// loc_lib_amd/csrc/icp_search.hip — K1, the search stage of the ICP hot path: kernels + launchers (see icp_kernels.hpp, search_walk.hpp).
#include "env.hpp"
#include "icp_kernels.hpp"
#include "launch.hpp"
#include "search_dispatch.hpp"
#include "search_walk.hpp"

#include <algorithm>
#include <iterator>
#include <type_traits>
#include <utility>

namespace locgpu {

// ---------------------------------------------------------------------------------------------
// K1, instrumented / unbounded-tree form: one thread per source point, the exact one-pass traversal with the libstdc++ heap.
// Grid (ceil(max_n/256), n_scans). Runs only for visit counting (bench.py's algorithmic bytes) and for trees with non-finite or huge
// coordinates; the hot kernel is icp_search_walk_kernel below.
template <int KMAX, int D, bool COUNT>
__global__ __launch_bounds__(kBlock) void icp_search_kernel(const uint2* __restrict__ tree, const float4* __restrict__ src,
                                                            const int* __restrict__ counts, const PoseState* __restrict__ st,
                                                            uint32_t* __restrict__ nn, size_t nn_pitch, int max_n, int k, float alpha_eff,
                                                            int skip_nonfinite, unsigned long long* __restrict__ visit_totals, uint32_t* __restrict__ touched,
                                                            const int* __restrict__ active, const int* __restrict__ src_of) {
    __shared__ uint32_t s_far[D][kBlock];
    __shared__ float s_d2[D][kBlock];
    const int scan = active ? active[blockIdx.y] : (int)blockIdx.y;
    if (st[scan].done) return;
    const int tid = threadIdx.x;
    const int i = blockIdx.x * kBlock + tid;
    if (i >= counts[scan]) return;
    const size_t gi = (size_t)scan * max_n + i;
    const float4 p = src[src_index(src_of, scan, max_n, i)];
    uint32_t out[KMAX];
    int cnt = 0;
    uint32_t nvis = 0, lvis = 0;
    const bool finite = !skip_nonfinite || (isfinite(p.x) && isfinite(p.y) && isfinite(p.z));  // pcl::isFinite, icp cpp:64 (P2P only)
    if (finite) {
        const D3 qs = se3_apply(st[scan].q, st[scan].t, D3{(double)p.x, (double)p.y, (double)p.z});
        KnnHeap<KMAX> heap;
        tree_knn_flat<KMAX, D, COUNT>(tree, (float)qs.x, (float)qs.y, (float)qs.z, k, alpha_eff, s_far, s_d2, tid, heap, nvis, lvis, touched);
        heap_to_sorted<KMAX>(heap, out, cnt);
    } else {
#pragma unroll
        for (int j = 0; j < KMAX; ++j) out[j] = kInvalidSlot;
    }
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < k) nn[(size_t)j * nn_pitch + gi] = out[j];
    if (COUNT) {
        atomicAdd(&visit_totals[0], (unsigned long long)nvis);
        atomicAdd(&visit_totals[1], (unsigned long long)lvis);
        atomicAdd(&visit_totals[2], 1ull);
    }
}

// Streaming accesses (elements touched once per launch) are marked non-temporal so that they do not evict tree nodes from L2 —
// measured one by one on the bench workload (search ms per 256-scan step): the search kernel's neighbour-list stores and source loads
// 25.0 -> 24.3; the fit kernel's neighbour-list loads -> 24.0. NOT the fit kernel's source loads (-> 24.7: the next search wants them cached).
typedef float f32x4_nt __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 load_once(const float4* __restrict__ p) {
    const f32x4_nt v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_nt*>(p));
    return float4{v.x, v.y, v.z, v.w};
}

// Source point of work-list entry gi = scan * max_n + i (the deep and redo lists), and its scan. T: the width the caller holds gi in.
template <class T>
__device__ __forceinline__ float4 list_point(const float4* __restrict__ src, const int* __restrict__ src_of, int max_n, T gi, int& scan) {
    scan = (int)(gi / (T)max_n);
    return src_of ? src[(size_t)src_of[scan] * max_n + (gi - (T)scan * (T)max_n)] : src[gi];
}

// K1: the traversal of search_walk.hpp. One-wave workgroups; dynamic LDS = DF rows x LANES x 8 B (the stack is the ONLY LDS of the
// kernel: a row below its bottom must lie outside the allocation). `dummy` = slot of the sentinel leaf.
// Every lane of the wave must call walk_query (wave-wide ballots inside); a lane without a query passes valid = false.
template <int K, int ROWB, bool STAMP = false, int WIN = 0>
__device__ __forceinline__ void walk_query(__amdgpu_buffer_rsrc_t rsrc, const uint2* __restrict__ tree, Walk<K>& w, bool valid, float alpha_eff, int T, uint32_t dummy,
                                           uint32_t col_addr, int cap) {
#pragma unroll
    for (int j = 0; j < K; ++j) { w.d[j] = __builtin_inff(); w.id[j] = kInvalidSlot; }
    w.slow = 0;
    // finite-arithmetic precondition of the traversal (the tree is `bounded`): anything else goes to the exact kernel
    const bool sane = fabsf(w.qx) < 1e18f && fabsf(w.qy) < 1e18f && fabsf(w.qz) < 1e18f;
    const uint32_t dummy_ref = node_ref(dummy);  // the traversal names nodes by reference (search_walk.hpp); scalar work
    if (valid && sane) {
        walk_descend<K, ROWB, WIN>(rsrc, tree, w, T, col_addr);
    } else {
        w.cur = dummy_ref; w.avail = 0; w.c3n = 0; w.slow = valid ? 1u : 0u;
    }
#ifndef LOCGPU_K1_C
#define LOCGPU_K1_C 2  // internal steps per round (A/B builds: -DLOCGPU_K1_C=1|3)
#endif
    walk_rounds_capped<K, ROWB, LOCGPU_K1_C, STAMP>(rsrc, w, alpha_eff, dummy_ref, col_addr, cap);
#pragma unroll
    for (int j = 0; j < K; ++j) w.id[j] = node_slot(w.id[j]);  // back to slots once per query, behind the loop
#pragma unroll
    for (int j = 0; j + 1 < K; ++j) w.slow |= w.d[j] == w.d[j + 1] ? 1u : 0u;  // equal distances in the final set: heap pop order is layout-dependent
}

// One or two queries of the wave that need the exact traversal (ties): answered here, the wave's LDS (its stacks are dead now)
// serving as their two stack columns. Returns false when there are more (the caller appends them to the redo list).
template <int K>
__device__ __forceinline__ bool walk_exact_in_wave(const uint2* __restrict__ tree, bool slow, float qx, float qy, float qz, float alpha_eff, uint2* lds,
                                                   uint32_t* __restrict__ nn, size_t nn_pitch, size_t gi, unsigned long long* __restrict__ search_stats) {
    const unsigned long long slow_mask = __ballot(slow);
    if (slow_mask == 0ull || __popcll(slow_mask) > 2) return slow_mask == 0ull;
    if (slow) {
        uint32_t(*s_far)[2] = reinterpret_cast<uint32_t(*)[2]>(lds);
        float(*s_d2)[2] = reinterpret_cast<float(*)[2]>(reinterpret_cast<char*>(lds) + 64 * 2 * sizeof(uint32_t));
        const int col = __popcll(slow_mask & ((1ull << (threadIdx.x & 63)) - 1ull));
        KnnHeap<K> heap;
        uint32_t nvis = 0, lvis = 0, out[K];
        int cnt;
        tree_knn_flat<K, 64, false, 2>(tree, qx, qy, qz, K, alpha_eff, s_far, s_d2, col, heap, nvis, lvis);
        heap_to_sorted<K>(heap, out, cnt);
#pragma unroll
        for (int j = 0; j < K; ++j) nn[(size_t)j * nn_pitch + gi] = out[j];
        if (search_stats) atomicAdd(&search_stats[1], 1ull);
    }
    return true;
}

// LANES = active lanes per wave = stack columns (64; 16 for launches that cannot fill the chip anyway: a wave's time is its
// longest traversal, and with 128-byte rows every level fits in LDS — T = 0 — so that no query needs the deep pass).
// WIN > 0: of the levels ≥ T only the deepest WIN = DF − 2 of each query's first descent are stored (search_walk.hpp, walk_descend).
template <int K, int DF, int LANES = 64, bool STAMP = false, int WIN = 0>
__global__ __launch_bounds__(64) void icp_search_walk_kernel(const uint2* __restrict__ tree, const float4* __restrict__ src,
                                                             const int* __restrict__ counts, const PoseState* __restrict__ st,
                                                             uint32_t* __restrict__ nn, size_t nn_pitch, int max_n, float alpha_eff, int T,
                                                             unsigned int tree_bytes, uint32_t dummy, int skip_nonfinite, uint32_t* __restrict__ redo_list,
                                                             unsigned int* __restrict__ redo_count, uint32_t* __restrict__ deep_list,
                                                             unsigned int* __restrict__ deep_count, unsigned long long* __restrict__ search_stats,
                                                             const int* __restrict__ active, const int* __restrict__ src_of,
                                                             unsigned long long* __restrict__ run_flags) {
    extern __shared__ uint2 s_dyn[];
    constexpr int ROWB = LANES * 8;
    static_assert(DF * ROWB >= 64 * 2 * 8, "exact stack columns do not fit");
    // The traversal reads rows BELOW the stack's bottom (they must lie outside the workgroup's LDS allocation and read as 0): the
    // stack has to start at LDS address 0, i.e. the kernel must own no other LDS. The launcher checks the code object
    // (search_kernels_lds_ok); this is the last line of defence — wrong neighbours or an endless loop otherwise.
    if ((uint32_t)(size_t)s_dyn != 0u) __builtin_trap();
    const int scan = active ? active[blockIdx.y] : (int)blockIdx.y;  // later chunks of an alignment launch only the scans still open
    const int tid = threadIdx.x;
    if (st[scan].done) return;
    const int i = blockIdx.x * LANES + tid;
    if (tid >= LANES || i >= counts[scan]) return;
    const size_t gi = (size_t)scan * max_n + i;
    const float4 p = load_once(&src[src_index(src_of, scan, max_n, i)]);
    // pcl::isFinite, icp cpp:64 (P2P only): such a point has no neighbours; its lane stays in the wave with nothing to do (the list
    // it stores at the end is the empty one)
    const bool finite = !skip_nonfinite || (isfinite(p.x) && isfinite(p.y) && isfinite(p.z));
    if (search_stats && finite) atomicAdd(&search_stats[0], 1ull);
    const D3 qs = se3_apply(st[scan].q, st[scan].t, D3{(double)p.x, (double)p.y, (double)p.z});
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)tree, 0, (int)tree_bytes, 0x00020000);
    Walk<K> w;
    w.qx = (float)qs.x; w.qy = (float)qs.y; w.qz = (float)qs.z;
    static_assert(WIN <= DF - 2, "the window lies in the rows above the two candidate rows");
    walk_query<K, ROWB, STAMP, WIN>(rsrc, tree, w, finite, alpha_eff, T, dummy, (uint32_t)(size_t)(&s_dyn[tid]), DF);  // DF rows: a stack that outgrows them → deep pass
    if (STAMP && search_stats) {
        // diagnostic build (LOCGPU_STAMP=1): rounds each lane needed against the rounds its wave ran — the kernel's lane
        // efficiency — and the per-query round counts behind the neighbour-list area of redo_list (2 x pitch entries in this build)
        atomicAdd(&search_stats[4], (unsigned long long)w.rounds);
        if ((tid & 63) == 0) { atomicAdd(&search_stats[9], (unsigned long long)w.wave_rounds); atomicAdd(&search_stats[12], 1ull); }
        atomicAdd(&search_stats[13], (unsigned long long)w.wave_rounds);  // rounds paid by this lane's wave, summed over lanes
        redo_list[nn_pitch + gi] = w.rounds;
    }
    const bool deep = w.c3n == 1u;
    const bool slow = !deep && w.slow != 0u;
    if (!deep && !slow) {
#pragma unroll
        for (int j = 0; j < K; ++j) __builtin_nontemporal_store(w.id[j], &nn[(size_t)j * nn_pitch + gi]);
    }
    if constexpr (K == 5 && LANES == 64) {
        // Run flags for the plane fit (icp_fit.hip, plane_accum_flagged): bit `lane` of the wave's word says that this query's
        // neighbour SET is not known to be the previous lane's — a leader; 0 = a follower, whose plane is its leader's. The wave is the
        // aligned group of 64 points a wave of the fit kernel takes, the five ids are in registers and the main loop's registers are
        // free. A lane whose list is written later (deep pass, in-wave exact walk, redo kernel) is a leader and so is the lane behind
        // it: its ids here mean nothing. Lanes past the scan's count have left and contribute 0; a wave wholly past it writes no word.
        if (run_flags) {  // uniform; every surviving lane of the wave is here
            uint32_t set5[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) set5[j] = w.id[j];
            sort5(set5);
            bool lead = w.id[4] == kInvalidSlot;  // fewer than five found: no list
#pragma unroll
            for (int j = 0; j < 5; ++j) lead |= (uint32_t)__shfl_up((int)set5[j], 1, 64) != set5[j];
            const unsigned long long unknown = __ballot(deep || slow);
            const unsigned long long word = (__ballot(lead) | unknown | (unknown << 1) | 1ull) & __ballot(true);
            if (tid == 0) run_flags[(size_t)scan * gridDim.x + blockIdx.x] = word;
        }
    }
    wave_append(deep_list, deep_count, deep, (uint32_t)gi);
    if (LANES == 16) {
        // the one-scan launch: every tied query is answered here, two at a time on the wave's dead stacks, so that the latency path
        // has no redo launch behind it (a wave holds 16 queries; more than two ties in one is a lattice map)
        bool pending = slow;
        for (;;) {
            const unsigned long long m = __ballot(pending);
            if (m == 0ull) break;
            const bool mine = pending && __popcll(m & ((1ull << (threadIdx.x & 63)) - 1ull)) < 2;
            (void)walk_exact_in_wave<K>(tree, mine, w.qx, w.qy, w.qz, alpha_eff, s_dyn, nn, nn_pitch, gi, search_stats);
            pending = pending && !mine;
        }
    } else if (!walk_exact_in_wave<K>(tree, slow, w.qx, w.qy, w.qz, alpha_eff, s_dyn, nn, nn_pitch, gi, search_stats)) {
        wave_append(redo_list, redo_count, slow, (uint32_t)gi);
    }
}

// The deep pass: the same traversal with EVERY level stored (T = 0, D + 2 rows) over the list of queries whose un-stored top
// levels could not be resolved from two candidates (≈1e-3 of them at 15 rows). One-wave workgroups, grid-stride over the list
// whose length lives on the device.
template <int K, int D, int LANES = 64>
__global__ __launch_bounds__(64) void icp_search_walk_list_kernel(const uint2* __restrict__ tree, const float4* __restrict__ src,
                                                                  const PoseState* __restrict__ st, uint32_t* __restrict__ nn, size_t nn_pitch, int max_n,
                                                                  float alpha_eff, unsigned int tree_bytes, uint32_t dummy, const uint32_t* __restrict__ list,
                                                                  const unsigned int* __restrict__ n_list, uint32_t* __restrict__ redo_list,
                                                                  unsigned int* __restrict__ redo_count, unsigned long long* __restrict__ search_stats,
                                                                  const int* __restrict__ src_of) {
    extern __shared__ uint2 s_dyn[];
    constexpr int ROWB = LANES * 8;
    static_assert((D + 2) * ROWB >= 64 * 2 * 8, "exact stack columns do not fit");
    if ((uint32_t)(size_t)s_dyn != 0u) __builtin_trap();  // see icp_search_walk_kernel
    const unsigned int n = *n_list;
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0 && search_stats) atomicAdd(&search_stats[2], (unsigned long long)n);
    if (tid >= LANES) return;  // LANES stack columns per wave (see icp_search_walk_kernel)
    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc((void*)tree, 0, (int)tree_bytes, 0x00020000);
    // a short list is spread thin: these are the long traversals, and a wave's time is the longest among its lanes
    const unsigned int per_wave = min((unsigned int)LANES, max(1u, (n + gridDim.x - 1) / gridDim.x));
    for (unsigned int r0 = blockIdx.x * per_wave; r0 < n; r0 += gridDim.x * per_wave) {
        const unsigned int r = r0 + (unsigned int)tid;
        const bool valid = (unsigned int)tid < per_wave && r < n;
        const uint32_t gi = valid ? list[r] : 0u;
        Walk<K> w;
        w.qx = w.qy = w.qz = 0.f;
        if (valid) {
            int scan;
            const float4 p = list_point(src, src_of, max_n, gi, scan);
            const D3 qs = se3_apply(st[scan].q, st[scan].t, D3{(double)p.x, (double)p.y, (double)p.z});
            w.qx = (float)qs.x; w.qy = (float)qs.y; w.qz = (float)qs.z;
        }
        walk_query<K, ROWB>(rsrc, tree, w, valid, alpha_eff, 0, dummy, (uint32_t)(size_t)(&s_dyn[tid]), 0x7fffffff);  // D + 2 rows ≥ depth: cannot overflow
        const bool slow = valid && w.slow != 0u;
        if (valid && !slow) {
#pragma unroll
            for (int j = 0; j < K; ++j) nn[(size_t)j * nn_pitch + gi] = w.id[j];
        }
        if (!walk_exact_in_wave<K>(tree, slow, w.qx, w.qy, w.qz, alpha_eff, s_dyn, nn, nn_pitch, gi, search_stats))
            wave_append(redo_list, redo_count, slow, gi);
    }
}

// Exact recomputation of the queries the fast kernel could not finish (≈1e-6 of them on real maps: ≈30 per 256-scan launch).
// One-wave workgroups over the list. A short list is dealt one query per WAVE (lane 0): 30 queries sharing a wave would each
// pay the others' heap-emulation branches and the longest traversal; alone in its wave a query costs its own ≈40 dependent loads.
// A long list (a lattice map: every distance ties) fills all 64 lanes of every wave.
constexpr int kRedoWaves = 2048;
// The deep pass: full waves, 2048 of them (16 lanes to a wave on 8192 waves — a wave's time is the longest traversal among its lanes,
// and these are the long ones — was measured: search 17.25 → 17.47 ms per 256-scan step; the pass is issue-bound like the walk kernel)
constexpr int kDeepLanes = 64, kDeepWaves = 2048;
template <int KMAX, int D>
__global__ __launch_bounds__(64) void icp_search_redo_kernel(const uint2* __restrict__ tree, const float4* __restrict__ src,
                                                             const PoseState* __restrict__ st, uint32_t* __restrict__ nn, size_t nn_pitch,
                                                             int max_n, int k, float alpha_eff, const uint32_t* __restrict__ redo_list,
                                                             const unsigned int* __restrict__ redo_count, unsigned long long* __restrict__ search_stats,
                                                             const int* __restrict__ src_of) {
    __shared__ uint32_t s_far[D][64];
    __shared__ float s_d2[D][64];
    const unsigned int n = *redo_count;
    const int tid = threadIdx.x;
    if (blockIdx.x == 0 && tid == 0 && search_stats) atomicAdd(&search_stats[1], (unsigned long long)n);
    const unsigned int per_wave = min(64u, (n + gridDim.x - 1) / gridDim.x);  // queries a wave takes per round
    if ((unsigned)tid >= per_wave) return;
    for (unsigned int r = blockIdx.x * per_wave + tid; r < n; r += gridDim.x * per_wave) {
        const size_t gi = redo_list[r];
        int scan;
        const float4 p = list_point(src, src_of, max_n, gi, scan);
        const D3 qs = se3_apply(st[scan].q, st[scan].t, D3{(double)p.x, (double)p.y, (double)p.z});
        KnnHeap<KMAX> heap;
        uint32_t nvis = 0, lvis = 0, out[KMAX];
        int cnt;
        tree_knn_flat<KMAX, D, false, 64>(tree, (float)qs.x, (float)qs.y, (float)qs.z, k, alpha_eff, s_far, s_d2, tid, heap, nvis, lvis);
        heap_to_sorted<KMAX>(heap, out, cnt);
#pragma unroll
        for (int j = 0; j < KMAX; ++j)
            if (j < k) nn[(size_t)j * nn_pitch + gi] = out[j];
    }
}

// Plain k-NN over given queries (SearchPointInterface::FindNearstPoints). 1-D grid.
template <int KMAX, int D>
__global__ __launch_bounds__(kBlock) void knn_query_kernel(const uint2* __restrict__ tree, const float* __restrict__ queries, size_t nq,
                                                           int k, float alpha_eff, int32_t* __restrict__ out_idx,
                                                           uint32_t* __restrict__ visits) {
    __shared__ uint32_t s_far[D][kBlock];
    __shared__ float s_d2[D][kBlock];
    const int tid = threadIdx.x;
    const size_t i = (size_t)blockIdx.x * kBlock + tid;
    if (i >= nq) return;
    KnnHeap<KMAX> heap;
    uint32_t nvis = 0, lvis = 0;
    tree_knn<KMAX, D, true>(tree, queries[3 * i], queries[3 * i + 1], queries[3 * i + 2], k, alpha_eff, s_far, s_d2, tid, heap, nvis, lvis);
    uint32_t out[KMAX];
    int cnt;
    heap_to_sorted<KMAX>(heap, out, cnt);
#pragma unroll
    for (int j = 0; j < KMAX; ++j)
        if (j < k) out_idx[i * k + j] = (out[j] == kInvalidSlot) ? -1 : (int32_t)(tree[out[j]].y & 0x3FFFFFFFu);  // original point index
    if (visits) { visits[2 * i] = nvis; visits[2 * i + 1] = lvis; }
}

// Instrumented pass: number of tree slots a search launch read at all (bitmap of tree_knn_flat), added to totals[3]; the bitmap is cleared.
__global__ __launch_bounds__(kBlock) void count_touched_kernel(uint32_t* __restrict__ touched, size_t n_words, unsigned long long* __restrict__ totals) {
    unsigned long long c = 0;
    for (size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x; i < n_words; i += (size_t)gridDim.x * kBlock) {
        c += (unsigned long long)__popc(touched[i]);
        touched[i] = 0u;
    }
    for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
    if ((threadIdx.x & 63) == 0 && c) atomicAdd(&totals[3], c);
}

// Test hook: the search stage's slot lists as original point indices (what knn_query_kernel reports), out[(gi * k) + j].
// No search kernel writes the rows past a scan's count, and the batch's list buffer is not cleared when it is allocated: those rows
// hold whatever the memory held, so they are reported as -1 without being read as slots (a ragged batch made this kernel read
// tree[garbage]: an illegal memory access). A slot beyond the tree is reported as -1 as well instead of being followed.
__global__ __launch_bounds__(kBlock) void nn_to_index_kernel(const uint2* __restrict__ tree, uint32_t tree_slots, const uint32_t* __restrict__ nn, size_t nn_pitch,
                                                             const int* __restrict__ counts, int max_n, size_t n_queries, int k, int32_t* __restrict__ out) {
    const size_t gi = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (gi >= n_queries) return;
    const bool live = (int)(gi % (size_t)max_n) < counts[gi / (size_t)max_n];
    for (int j = 0; j < k; ++j) {
        const uint32_t slot = live ? nn[(size_t)j * nn_pitch + gi] : kInvalidSlot;
        out[gi * k + j] = (slot == kInvalidSlot || slot >= tree_slots) ? -1 : (int32_t)(tree[slot].y & 0x3FFFFFFFu);
    }
}

// ---------------------------------------------------------------------------------------------
// Launchers (declared in launch.hpp).

// with_depth / with_k: search_dispatch.hpp

bool stamp_build() {
    static const bool on = env_int("LOCGPU_STAMP", 0) != 0;
    return on;
}

void launch_nn_to_index(const uint2* tree, size_t tree_slots, const uint32_t* nn, size_t nn_pitch, const int* counts, int max_n, size_t n_queries, int k,
                        int32_t* out, hipStream_t s) {
    if (n_queries == 0 || max_n <= 0) return;
    hipLaunchKernelGGL(nn_to_index_kernel, dim3((unsigned)((n_queries + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, tree, (uint32_t)tree_slots, nn, nn_pitch, counts, max_n,
                       n_queries, k, out);
}

void launch_count_touched(uint32_t* touched, size_t n_words, unsigned long long* totals, hipStream_t s) {
    hipLaunchKernelGGL(count_touched_kernel, dim3(1024), dim3(kBlock), 0, s, touched, n_words, totals);
}

template <int KMAX, int D, bool COUNT>
static void launch_exact(const SearchArgs& a, hipStream_t s) {
    dim3 grid((a.max_n + kBlock - 1) / kBlock, a.active ? a.n_active : a.n_scans);
    hipLaunchKernelGGL((icp_search_kernel<KMAX, D, COUNT>), grid, dim3(kBlock), 0, s, a.tree, a.src, a.counts, a.st, a.nn, a.nn_pitch, a.max_n,
                       a.k, a.alpha_eff, a.skip_nonfinite, a.visit_totals, COUNT ? a.touched : nullptr, a.active, a.src_of);
}

// The 64-lane walk kernel's shapes: DF stored LDS stack rows per lane (8 B each; the levels above them are kept as candidates,
// search_walk.hpp) and the sliding window WIN over them (0 = none). One-wave workgroups (waves retire independently), so the rows set
// the waves a CU holds: 10 → 5 120 B → 32 waves per CU (profiles/r06_k1_occupancy.md), 15 → 7.5 KB → 21. The balance is between
// occupancy and the queries that go to the deep pass — measured on the bench workload (search ms per 256-scan step, round 2, no window):
// 12 → 30.0, 13 → 28.2, 14 → 26.2, 15 → 25.5, 16 → 27.2, 20 → 29.0, 24 → 35.9.
// [0] is the default; LOCGPU_FAST_STACK=12|15|24 selects the others: the parity tests run the deep-pass hand-over at stack depths
// where it is common (15: round 2-5's shape). This list is all a launch can select and all search_kernels_lds_ok checks.
struct WalkShape { int df, win; };
constexpr WalkShape kWalkShapes[] = {{10, 8}, {12, 0}, {15, 0}, {24, 0}};
// f(integral_constant DF, integral_constant WIN) for every shape in turn, as long as f returns true; whether all did
template <class F, size_t... I>
static bool all_walk_shapes(F&& f, std::index_sequence<I...>) {
    return (f(std::integral_constant<int, kWalkShapes[I].df>{}, std::integral_constant<int, kWalkShapes[I].win>{}) && ...);
}
template <class F>
static bool all_walk_shapes(F&& f) { return all_walk_shapes(f, std::make_index_sequence<std::size(kWalkShapes)>{}); }

static int fast_stack_depth() {
    static const int v = [] {
        const int e = env_int("LOCGPU_FAST_STACK", kWalkShapes[0].df);
        for (const WalkShape& w : kWalkShapes)
            if (w.df == e) return e;
        return kWalkShapes[0].df;
    }();
    return v;
}
// The window shape leaves the levels above T = depth − 13 un-stored, as 15 plain rows would: the un-stored top levels are sized by
// what a TYPICAL descent can store, the window takes care of the deeper ones.
constexpr int kWindowStored = 13;

// The walk kernels' LDS stack must start at LDS address 0 (search_walk.hpp: rows below the bottom are read and must fall outside
// the allocation). That holds exactly when the kernel has no static LDS of its own — checked on the code object for every
// instantiation the launchers below can select, once per process, when the first context is created (not at launch time: a launch
// may happen under stream capture).
template <auto Kernel>
static bool no_static_lds() {
    hipFuncAttributes attr{};
    return hipFuncGetAttributes(&attr, reinterpret_cast<const void*>(Kernel)) == hipSuccess && attr.sharedSizeBytes == 0;
}
template <int K>
static bool walk_kernels_ok() {
    bool ok = all_walk_shapes([](auto DF, auto WIN) {
        return no_static_lds<icp_search_walk_kernel<K, DF(), 64, false, WIN()>>() && no_static_lds<icp_search_walk_kernel<K, DF(), 64, true, WIN()>>();
    });
    for (int depth : {32, 40, 64})  // one tree depth per rung of with_depth
        with_depth(depth, [&](auto D) { ok = ok && no_static_lds<icp_search_walk_kernel<K, D() + 2, 16>>() && no_static_lds<icp_search_walk_list_kernel<K, D(), kDeepLanes>>(); });
    return ok;
}
bool search_kernels_lds_ok() {
    static const bool ok = walk_kernels_ok<1>() && walk_kernels_ok<5>();
    return ok;
}

template <int K, int D>
static void launch_redo(const SearchArgs& a, hipStream_t s) {
    hipLaunchKernelGGL((icp_search_redo_kernel<K, D>), dim3(kRedoWaves), dim3(64), 0, s, a.tree, a.src, a.st, a.nn, a.nn_pitch, a.max_n, a.k,
                       a.alpha_eff, a.redo_list, a.redo_count, a.search_stats, a.src_of);
}
// 2048 one-wave blocks of 17 KB LDS are all resident at once (nine fit a CU): the first iteration's ≈140 k deep queries take one
// traversal per wave instead of two or three in sequence (search 18.07 → 17.80 ms per 256-scan step; 4608: 17.96)
template <int K, int D>
static void launch_walk_list(const SearchArgs& a, const uint32_t* list, const unsigned int* n_list, hipStream_t s) {
    hipLaunchKernelGGL((icp_search_walk_list_kernel<K, D, kDeepLanes>), dim3(kDeepWaves), dim3(64), (D + 2) * kDeepLanes * 8, s, a.tree, a.src, a.st, a.nn, a.nn_pitch, a.max_n,
                       a.alpha_eff, (unsigned int)a.tree_bytes + 16u, (uint32_t)(a.tree_bytes / 8), list, n_list, a.redo_list, a.redo_count, a.search_stats, a.src_of);
}

// The search stage of one Gauss–Newton iteration: walk kernel → deep pass → exact redo (the last two over device-side lists that are
// almost always short). a.redo_count / a.redo_count2 are zero here: the caller clears them before an alignment's first iteration,
// gn_solve_kernel after every search. Returns whether the walk kernel wrote a.run_flags: the 64-lane route with k = 5 alone does.
template <int K, int D, int DF, int WIN>
static bool launch_walk(const SearchArgs& a, hipStream_t s) {
    const bool stamp = stamp_build();
    const uint32_t dummy = (uint32_t)(a.tree_bytes / 8);  // the sentinel leaf behind the tree
    const unsigned int rsrc_bytes = (unsigned int)a.tree_bytes + 16u;
    const int n_launch = a.active ? a.n_active : a.n_scans;  // grid.y: the scans still open (a.active) or all of them
    if (!stamp && (size_t)((a.max_n + 63) / 64) * n_launch <= 2048) {
        // fewer than 2048 full waves (one or two scans): quarter-filled waves with every level stored — no deep pass, and the
        // 16-lane kernel answers its ties itself: no redo launch on the latency path
        dim3 g1((a.max_n + 15) / 16, n_launch);
        hipLaunchKernelGGL((icp_search_walk_kernel<K, D + 2, 16>), g1, dim3(64), (D + 2) * 16 * 8, s, a.tree, a.src, a.counts, a.st, a.nn, a.nn_pitch, a.max_n,
                           a.alpha_eff, 0, rsrc_bytes, dummy, a.skip_nonfinite, a.redo_list, a.redo_count, a.redo_list2, a.redo_count2, a.search_stats, a.active, a.src_of, nullptr);
        return false;
    }
    // rows 0/1 of the DF stored rows hold the candidates of the un-stored levels, the other DF-2 rows one level each. Queries whose
    // un-stored levels need more than two candidates, or whose candidate descent outgrows the rows, go through a.redo_list2 to the
    // deep pass (every level stored), ties to the exact redo kernel.
    const int stored = WIN ? kWindowStored : DF - 2;
    const int Tw = a.depth > stored ? a.depth - stored : 0;
    dim3 g2((a.max_n + 63) / 64, n_launch);
    // LOCGPU_K1_LDS_BYTES (measurement only, profiles/r06_k1_occupancy.md): a larger dynamic LDS allocation than the DF rows need, i.e.
    // fewer waves per CU. The extra bytes sit ABOVE the stack (a push beyond row DF lands in them instead of off the allocation:
    // harmless, `cap` sends such a query to the deep pass either way).
    static const bool lds_knob = env_flag("LOCGPU_K1_LDS_BYTES");  // present at the first launch: re-read at every launch (tools/k1_occupancy.py sweeps it in one process)
    unsigned lds_bytes = DF * 64 * 8;
    if (lds_knob) lds_bytes = (unsigned)std::max(env_int("LOCGPU_K1_LDS_BYTES", 0), DF * 64 * 8);
    if (stamp)  // diagnostic build: counts rounds per lane and per wave (search_stats[4], [9], [12], [13]; per query at redo_list[pitch + gi]); timing meaningless
        hipLaunchKernelGGL((icp_search_walk_kernel<K, DF, 64, true, WIN>), g2, dim3(64), DF * 64 * 8, s, a.tree, a.src, a.counts, a.st, a.nn, a.nn_pitch, a.max_n,
                           a.alpha_eff, Tw, rsrc_bytes, dummy, a.skip_nonfinite, a.redo_list, a.redo_count, a.redo_list2, a.redo_count2, a.search_stats, a.active, a.src_of, a.run_flags);
    else
        hipLaunchKernelGGL((icp_search_walk_kernel<K, DF, 64, false, WIN>), g2, dim3(64), lds_bytes, s, a.tree, a.src, a.counts, a.st, a.nn, a.nn_pitch, a.max_n,
                           a.alpha_eff, Tw, rsrc_bytes, dummy, a.skip_nonfinite, a.redo_list, a.redo_count, a.redo_list2, a.redo_count2, a.search_stats, a.active, a.src_of, a.run_flags);
    launch_walk_list<K, D>(a, a.redo_list2, a.redo_count2, s);
    launch_redo<K, D>(a, s);
    return K == 5 && a.run_flags != nullptr;
}

bool launch_icp_search(const SearchArgs& a, hipStream_t s, bool* wrote_run_flags) {
    if (wrote_run_flags) *wrote_run_flags = false;
    if (a.scan_tree_base) return launch_icp_search_pairs(a, s);  // a forest target: every scan walks a tree of its own (icp_search_pairs.hip)
    // Instrumented (visit-counting) runs and trees with non-finite / huge coordinates (no redo list) use the exact one-pass kernel.
    const bool exact_only = a.visit_totals != nullptr || !a.redo_list || !a.redo_list2;
    return with_k<false>(a.k, [&](auto Kc) {
        return with_depth(a.depth, [&](auto Dc) {
            constexpr int K = decltype(Kc)::value, D = decltype(Dc)::value;
            if (exact_only) return a.visit_totals ? launch_exact<K, D, true>(a, s) : launch_exact<K, D, false>(a, s);
            all_walk_shapes([&](auto DF, auto WIN) {  // stops at the selected one
                if (DF() != fast_stack_depth()) return true;
                const bool wrote = launch_walk<K, D, DF(), WIN()>(a, s);
                if (wrote_run_flags) *wrote_run_flags = wrote;
                return false;
            });
        });
    });
}

bool launch_icp_search_redo(const SearchArgs& a, hipStream_t s) {
    return with_k<false>(a.k, [&](auto Kc) {
        return with_depth(a.depth, [&](auto Dc) { launch_redo<decltype(Kc)::value, decltype(Dc)::value>(a, s); });
    });
}

// The walk traversal with every level stored over `list` (length *n_list on the device) — what the grid search could not settle,
// with a.alpha_eff = 1 — then the exact redo kernel for its ties. a.redo_count must have been zeroed on the stream.
bool launch_icp_search_list(const SearchArgs& a, const uint32_t* list, const unsigned int* n_list, hipStream_t s) {
    return with_k<false>(a.k, [&](auto Kc) {
        return with_depth(a.depth, [&](auto Dc) {
            constexpr int K = decltype(Kc)::value, D = decltype(Dc)::value;
            launch_walk_list<K, D>(a, list, n_list, s);
            launch_redo<K, D>(a, s);
        });
    });
}

bool launch_knn_query(const uint2* tree, int depth, const float* q, size_t nq, int k, float alpha_eff, int32_t* out, uint32_t* visits,
                      hipStream_t s) {
    return with_k<true>(k, [&](auto Kc) {
        return with_depth(depth, [&](auto Dc) {
            hipLaunchKernelGGL((knn_query_kernel<decltype(Kc)::value, decltype(Dc)::value>), dim3((unsigned)((nq + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, tree, q, nq, k,
                               alpha_eff, out, visits);
        });
    });
}

}  // namespace locgpu
