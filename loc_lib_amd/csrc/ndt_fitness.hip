// loc_lib_amd/csrc/ndt_fitness.hip — the fitness score of an alignment against the DIRECT NDT target (include/locgpu.h,
// locgpu_ndt_fitness): the mean over the inlier points of the smallest accepted χ² residual eᵀ·info·e among the voxels AlignNdt probes
// for the point (ndt_registration.cpp:399-433). AlignNdt forms that residual for its gate (:416-421) and drops it; here it is kept.
//
// Shape: one kernel probes the voxel table with ndt_accum_kernel's look-up (ndt_kernels.hip, where it says why this is a copy and not a
// shared function; like that kernel it is a template over the key rule, so a voxel set is scored by the same text) and
// reduces {Σ min res, inliers, finite points} in FP64 per block — the accumulators' scheme, spelled out in the kernel (it says
// why); the row format is the ICP score's (fitness.hip), so its last small kernel adds the block rows of a scan in its
// fixed order. No atomics on the sums.
//
// The split of the sums is FIXED (kFitPts points per thread, a block covers 1024 consecutive points of its scan) and does not depend
// on the batch: a scan scores the same bits alone, in a batch of any size, from a shared-source batch and in any chunk of a search.
#include "icp_kernels.hpp"
#include "launch.hpp"
#include "ndt_kernels.hpp"

namespace locgpu {

constexpr int kNdtFitPts = 4;  // = kFitPts of fitness.hip: launch_fitness_sum sums icp_fitness_rows(max_n) rows per scan

// A template over the key rule, as ndt_accum_kernel is: one target's table, or a voxel set with the scan's look-ups under its own target.
template <class Rule>
__global__ __launch_bounds__(kBlock) void ndt_fitness_accum_kernel(const NdtSlot* __restrict__ slots, const NdtRecord* __restrict__ rec, size_t cap_mask,
                                                                   double inv_voxel, double res_th, int n_nearby, const float4* __restrict__ src,
                                                                   const int* __restrict__ counts, const PoseState* __restrict__ st, int max_n,
                                                                   double* __restrict__ partials, const int* __restrict__ src_of, Rule rule) {
    __shared__ double s_part[kBlock / 64][kFitW];
    const int scan = blockIdx.y;
    const int n = counts[scan];
    unsigned long long tbits = 0;  // the set's rule: the key bits of this scan's target
    if constexpr (std::is_same_v<Rule, NdtVoxelSet>) tbits = ndt_set_target_bits(rule.pair_target[scan]);
    double sum = 0.0, inl = 0.0, fin = 0.0;
    // one point at a time (as the accumulate kernel): its seven look-ups are what is in flight together
#pragma unroll 1
    for (int pp = 0; pp < kNdtFitPts; ++pp) {
        const int i = (blockIdx.x * kNdtFitPts + pp) * kBlock + threadIdx.x;
        if (i >= n) continue;
        const float4 p = src[src_index(src_of, scan, max_n, i)];
        // a point with a non-finite coordinate is skipped and not counted (the ICP score's rule)
        if (!(isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) continue;
        const D3 qs = se3_apply(st[scan].q, st[scan].t, D3{(double)p.x, (double)p.y, (double)p.z});
        int kx, ky, kz;
        ndt_key_of(qs, inv_voxel, kx, ky, kz);
        // nearby_grids_ order (ndt cpp:57-58): (0,0,0) (-1,0,0) (1,0,0) (0,1,0) (0,-1,0) (0,0,-1) (0,0,1)
        const int ox[7] = {0, -1, 1, 0, 0, 0, 0}, oy[7] = {0, 0, 0, 1, -1, 0, 0}, oz[7] = {0, 0, 0, 0, 0, -1, 1};
        unsigned long long key[7], kk[7];
        unsigned int vx[7];
        size_t hs[7];
        bool found[7];
        // keys and probe validity per rule, as in ndt_accum_kernel (ndt_kernels.hip, where each rule is explained)
        if constexpr (std::is_same_v<Rule, NdtOneTarget>) {
            const bool centre_ok = ndt_key_in_range(kx, ky, kz);
            const unsigned long long key0 = ndt_pack(centre_ok ? kx : 0, centre_ok ? ky : 0, centre_ok ? kz : 0);
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const int moved = ox[j] != 0 ? kx + ox[j] : (oy[j] != 0 ? ky + oy[j] : kz + oz[j]);  // j = 0: kz, in range with the centre
                found[j] = j < n_nearby && centre_ok && moved > -kNdtBias && moved < kNdtBias;
                const long long delta = (long long)ox[j] * (1ll << 42) + (long long)oy[j] * (1ll << 21) + (long long)oz[j];  // a constant after unrolling
                key[j] = found[j] ? key0 + (unsigned long long)delta : key0;
                hs[j] = ndt_hash32(key[j], cap_mask);
            }
        } else {
            const bool centre_ok = ndt_key_in_range(kx, ky, kz);
            const bool okx = ndt_set_coord_ok(kx), oky = ndt_set_coord_ok(ky), okz = ndt_set_coord_ok(kz);
            const unsigned long long key0 = ndt_set_pack(tbits, centre_ok ? kx : 0, centre_ok ? ky : 0, centre_ok ? kz : 0);
#pragma unroll
            for (int j = 0; j < 7; ++j) {
                const int moved = ox[j] != 0 ? kx + ox[j] : (oy[j] != 0 ? ky + oy[j] : kz + oz[j]);  // j = 0: kz
                const bool rest_ok = ox[j] != 0 ? (oky && okz) : (oy[j] != 0 ? (okx && okz) : (okx && oky));
                found[j] = j < n_nearby && centre_ok && rest_ok && ndt_set_coord_ok(moved);
                const unsigned long long delta = ndt_set_delta(ox[j], oy[j], oz[j]);  // a constant after unrolling
                key[j] = found[j] ? key0 + delta : key0;
                hs[j] = ndt_hash32(key[j], cap_mask);
            }
        }
#pragma unroll
        for (int j = 0; j < 7; ++j) { const NdtSlot sl = slots[hs[j]]; kk[j] = sl.key; vx[j] = sl.vid; }
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            if (found[j] && kk[j] != key[j] && kk[j] != kNdtEmpty) {  // collision on the first probe: walk on (load factor ≤ 0.5: an empty slot ends it)
                size_t h = (hs[j] + 1) & cap_mask;
                for (;;) {
                    const NdtSlot sl = slots[h];
                    if (sl.key == key[j]) { kk[j] = sl.key; vx[j] = sl.vid; break; }
                    if (sl.key == kNdtEmpty) { kk[j] = sl.key; break; }
                    h = (h + 1) & cap_mask;
                }
            }
            found[j] = found[j] && kk[j] == key[j];
        }
        double best = HUGE_VAL;
        bool any = false;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const NdtRecord& R = rec[found[j] ? vx[j] : 0u];  // a voxel that is not there reads record 0 and is not accepted
            const double* m = R.mu;
            const double* I = R.info;
            const D3 e{qs.x - m[0], qs.y - m[1], qs.z - m[2]};
            // e.transpose() * v.info_ * e (ndt cpp:416) with the association of ndt_accum_kernel: the row vector eᵀ·info, then its dot product with e
            const double t0 = (e.x * I[0] + e.y * I[3]) + e.z * I[6];
            const double t1 = (e.x * I[1] + e.y * I[4]) + e.z * I[7];
            const double t2 = (e.x * I[2] + e.y * I[5]) + e.z * I[8];
            const double res = (t0 * e.x + t1 * e.y) + t2 * e.z;
            const bool accept = found[j] && !(isnan(res) || res > res_th);  // AlignNdt's gate (ndt cpp:417-421)
            best = accept ? fmin(best, res) : best;  // the minimum: the best explanation, whatever the probe order
            any = any || accept;
        }
        fin += 1.0;
        sum = any ? sum + best : sum;
        inl = any ? inl + 1.0 : inl;
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

void launch_ndt_fitness(const NdtTable* t, const float4* src, const int* counts, const PoseState* st, int max_n, int n_scans, double* partials,
                        double* out, hipStream_t s, const int* src_of, const uint32_t* pair_target) {
    static_assert(kNdtFitPts * kBlock == 1024, "the rows launch_fitness_sum adds");
    const int rows = icp_fitness_rows(max_n);
    if (pair_target)
        hipLaunchKernelGGL(ndt_fitness_accum_kernel<NdtVoxelSet>, dim3(rows, n_scans), dim3(kBlock), 0, s, t->d_slots, t->d_rec, t->cap - 1, t->inv_voxel, t->res_outlier_th,
                           t->n_nearby, src, counts, st, max_n, partials, src_of, NdtVoxelSet{pair_target});
    else
        hipLaunchKernelGGL(ndt_fitness_accum_kernel<NdtOneTarget>, dim3(rows, n_scans), dim3(kBlock), 0, s, t->d_slots, t->d_rec, t->cap - 1, t->inv_voxel, t->res_outlier_th,
                           t->n_nearby, src, counts, st, max_n, partials, src_of, NdtOneTarget{});
    launch_fitness_sum(partials, rows, n_scans, out, nullptr, s);
}

}  // namespace locgpu
