// loc_lib_amd/csrc/ndt_kernels.hip — direct NDT on gfx950: voxel-table build (K4) and per-iteration accumulation (K5).
//
// K4 follows NdtRegistration::SetDirectNdtTargetCloud (ndt_registration.cpp:87-148): key = trunc-toward-zero of
// pt/voxel (`(pt * inv_voxel_size_).cast<int>()`, :100), per voxel with more than min_pts_in_voxel points the mean and
// the (n−1)-normalised covariance (math_utils.h:55-72), SVD, λ1,λ2 clamped to ≥ 1e-3·λ0, info = V·diag(1/λ)·Uᵀ (:118-130).
// The sums are the REFERENCE's sums — the shared ingest front (ndt_ingest.hpp) puts a voxel's points side by side in input order and one
// thread per voxel adds them sequentially, products not fused — so μ and Σ equal the reference's bit for bit and two ingests of one
// map give the same bits (rounds 1-4 summed with FP64 atomics: 1e-10 / 1e-7 from the oracle, different last bits run to run).
// The table is open addressing over 16-byte {key, voxel index} slots plus a dense array of 128-byte records {μ, info}
// (ndt_kernels.hpp): two dependent gathers per voxel instead of three. Voxels the reference drops (:136-142) are simply not inserted.
// K5 follows AlignNdt's inner loop (:399-433): 7 probes in the reference's offset order (:57-58), χ² gate with info,
// sums NOT weighted by info, effective_num once per source point.
#include <algorithm>
#include <vector>

#include "icp_kernels.hpp"
#include "ndt_ingest.hpp"
#include "ndt_kernels.hpp"

#ifndef LOCGPU_NDT_WAVES
#define LOCGPU_NDT_WAVES 4
#endif
namespace locgpu {

// One thread per voxel (run of the sorted keys) with more than min_pts points: math::ComputeMeanAndCov's sums (ndt_mean_scatter),
// Σ/(n−1), one-sided Jacobi SVD, clamp, info = V diag(1/λ) Uᵀ (ndt cpp:111-130; ndt_voxel_record, ndt_ingest.hpp) — then the record goes
// into the table.
__global__ __launch_bounds__(kBlock) void ndt_voxel_kernel(const unsigned long long* __restrict__ skey, const float4* __restrict__ psorted, const uint32_t* __restrict__ ustart,
                                                           const int* __restrict__ n_runs, int min_pts, NdtSlot* __restrict__ slots, NdtRecord* __restrict__ rec, size_t cap_mask,
                                                           int* __restrict__ n_vox) {
    const int u = blockIdx.x * kBlock + threadIdx.x;
    if (u >= *n_runs) return;
    const uint32_t b = ustart[u], e = ustart[u + 1];
    const uint32_t len = e - b;
    const unsigned long long key = skey[b];
    if (key == kNdtEmpty || (int)len <= min_pts) return;  // count > min_pts_in_voxel_ (ndt cpp:111,137)
    ndt_voxel_record(key, psorted, b, e, rec, [&]() -> unsigned int {
        const size_t h = ndt_claim_slot(slots, key, cap_mask);
        const unsigned int vid = (unsigned int)atomicAdd(n_vox, 1);  // which record a voxel gets varies from run to run; what is in it does not
        slots[h].vid = vid;
        return vid;
    });
}

// Read-back for tests: the records as dense arrays, the key unpacked by the table's rule (a set's key without its target).
template <class Rule>
__global__ __launch_bounds__(kBlock) void ndt_dump_kernel(const NdtRecord* __restrict__ rec, size_t n, int* __restrict__ keys, double* __restrict__ mu, double* __restrict__ info) {
    const size_t o = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (o >= n) return;
    const NdtRecord& R = rec[o];
    if constexpr (std::is_same_v<Rule, NdtVoxelSet>) {
        int t, x, y, z;
        ndt_set_unpack(R.key, t, x, y, z);
        keys[3 * o + 0] = x; keys[3 * o + 1] = y; keys[3 * o + 2] = z;
    } else {
        keys[3 * o + 0] = (int)((R.key >> 42) & 0x1FFFFF) - kNdtBias;
        keys[3 * o + 1] = (int)((R.key >> 21) & 0x1FFFFF) - kNdtBias;
        keys[3 * o + 2] = (int)(R.key & 0x1FFFFF) - kNdtBias;
    }
    for (int k = 0; k < 3; ++k) mu[3 * o + k] = R.mu[k];
    for (int k = 0; k < 9; ++k) info[9 * o + k] = R.info[k];
}

hipError_t ndt_table_alloc(NdtTable& t, size_t runs, size_t n_rec, hipStream_t s) {
    // A SPARSE table: at load 0.03 nearly every look-up — hit or miss — ends at its first probe, and a collision walk is what costs
    // (a wave walks as long as its unluckiest lane, seven times per point); the lines a launch touches are as many as the voxels it
    // looks up, whatever the table's size (measured: load <= 0.5, 15.7 ms per 256-scan step; load <= 0.03, see profiles/experiments.md).
    size_t cap = 1024;
    while (cap < 32 * runs && cap < ((size_t)1 << 26)) cap <<= 1;  // at most 1 GB of slots ...
    while (cap < 2 * runs) cap <<= 1;                              // ... but never above load 0.5
    LOCGPU_TRY(t.d_slots.alloc(cap));
    LOCGPU_TRY(t.d_rec.alloc(n_rec));
    t.cap = cap;
    hipLaunchKernelGGL(ndt_fill_kernel<NdtSlot>, dim3((unsigned)((cap + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, t.d_slots.get(), cap, NdtSlot{kNdtEmpty, 0u, 0u});
    return hipMemsetAsync(t.d_rec, 0, n_rec * sizeof(NdtRecord), s);  // record 0 is read for voxels that are not there: finite numbers, never accepted
}

hipError_t ndt_build(NdtTable& t, const float4* d_pts, size_t n, double voxel_size, int min_pts_in_voxel, hipStream_t s, bool* bad_key) {
    t = NdtTable();
    *bad_key = false;
    t.inv_voxel = 1.0 / voxel_size;  // the reference's constructors recompute it (ndt cpp:15,25)
    if (n > 0xFFFFFFF0ull) return hipErrorInvalidValue;
    NdtIngest ing;  // local: allocated per build, freed on return
    LOCGPU_TRY(ing.reserve(n + 1, false));
    LOCGPU_TRY(ing.run(d_pts, n, t.inv_voxel, false, s));
    int* const d_n_vox = ing.ctr.get() + kIngUser;  // voxels kept
    int h_ctr[kIngCtrs] = {};
    LOCGPU_TRY(hipMemcpyAsync(h_ctr, ing.ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, s));
    LOCGPU_TRY(hipStreamSynchronize(s));
    *bad_key = h_ctr[kIngBadKey] != 0;
    const size_t runs = (size_t)h_ctr[kIngRuns];
    LOCGPU_TRY(ndt_table_alloc(t, runs, std::max<size_t>(runs, 1), s));  // room for every run; the kept voxels fill a prefix
    if (runs > 0 && !*bad_key)
        hipLaunchKernelGGL(ndt_voxel_kernel, dim3((unsigned)((runs + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ing.skey, ing.psorted, ing.ustart, ing.ctr, min_pts_in_voxel,
                           t.d_slots, t.d_rec, t.cap - 1, d_n_vox);
    LOCGPU_TRY(hipGetLastError());
    LOCGPU_TRY(hipMemcpyAsync(h_ctr, ing.ctr, sizeof(h_ctr), hipMemcpyDeviceToHost, s));
    LOCGPU_TRY(hipStreamSynchronize(s));
    t.n_vox = (size_t)h_ctr[kIngUser];
    return hipSuccess;
}

hipError_t ndt_dump_range(const NdtTable& t, size_t first, size_t n, bool set_keys, int* keys, double* mu, double* info, hipStream_t s) {
    if (!t.d_rec || n == 0) return hipSuccess;
    if (first + n > t.n_vox) return hipErrorInvalidValue;
    DevBuf<int> d_keys;
    DevBuf<double> d_mu, d_info;
    LOCGPU_TRY(d_keys.alloc(n * 3));
    LOCGPU_TRY(d_mu.alloc(n * 3));
    LOCGPU_TRY(d_info.alloc(n * 9));
    const dim3 grid((unsigned)((n + kBlock - 1) / kBlock));
    if (set_keys) hipLaunchKernelGGL(ndt_dump_kernel<NdtVoxelSet>, grid, dim3(kBlock), 0, s, t.d_rec.get() + first, n, d_keys, d_mu, d_info);
    else hipLaunchKernelGGL(ndt_dump_kernel<NdtOneTarget>, grid, dim3(kBlock), 0, s, t.d_rec.get() + first, n, d_keys, d_mu, d_info);
    if (keys) LOCGPU_TRY(hipMemcpyAsync(keys, d_keys, n * 3 * sizeof(int), hipMemcpyDeviceToHost, s));
    if (mu) LOCGPU_TRY(hipMemcpyAsync(mu, d_mu, n * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (info) LOCGPU_TRY(hipMemcpyAsync(info, d_info, n * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
    LOCGPU_TRY(hipStreamSynchronize(s));
    return hipSuccess;
}

hipError_t ndt_dump(const NdtTable& t, int* keys, double* mu, double* info, size_t out_cap, hipStream_t s) {
    return ndt_dump_range(t, 0, std::min(out_cap, t.n_vox), false, keys, mu, info, s);
}

hipError_t ndt_slots_read(const NdtTable& t, uint64_t* keys, int32_t* vid, size_t out_cap, hipStream_t s) {
    const size_t n = std::min(out_cap, t.cap);
    if (!t.d_slots || n == 0 || (!keys && !vid)) return hipSuccess;
    std::vector<NdtSlot> h(n);
    LOCGPU_TRY(hipMemcpyAsync(h.data(), t.d_slots, n * sizeof(NdtSlot), hipMemcpyDeviceToHost, s));
    LOCGPU_TRY(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; ++i) {
        if (keys) keys[i] = (uint64_t)h[i].key;
        if (vid) vid[i] = h[i].key == kNdtEmpty ? -1 : (int32_t)h[i].vid;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------
// K5. Grid (ceil(max_n/256), n_scans).
// The seven-voxel look-up below is written out in the kernel, and again in ndt_fitness_accum_kernel (ndt_fitness.hip: the same table
// and hash). It is not a shared FUNCTION on purpose: this kernel sits at 126 VGPRs under the 128 that amdgpu_waves_per_eu(4,4)
// allows, with no scratch, and every shape of a shared __forceinline__ look-up that was tried (arrays by reference, a returned
// struct, a visitor, the slot look-up alone without the residual, an always_inline lambda around the unchanged text) put 240-440
// bytes per lane of scratch into it. What IS shared is the kernel's text: the single-target look-up and the voxel set's (pairwise batch
// NDT) are this one template over the key rule (ndt_kernels.hpp), and they differ in the block that forms the seven keys and nowhere
// else — probe order, collision walk, record 0 for absent voxels, gate, sums and partial layout are written once, and each
// instantiation compiles to the registers and instructions of a kernel written out for its rule (profiles/ndt_one_kernel_text.md).
// A scan of a set reads the word of its target (pair_target[scan], uniform over the block) and forms its keys under that target's
// bits; its range rule is given at the block.
// inc_accum_kernel (ndt_inc.hip) stays a kernel of its own: another table layout, another hash, contracted arithmetic.
template <class Rule>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(LOCGPU_NDT_WAVES, LOCGPU_NDT_WAVES))) void ndt_accum_kernel(const NdtSlot* __restrict__ slots, const NdtRecord* __restrict__ rec, size_t cap_mask,
                                                           double inv_voxel, double res_th, int n_nearby, const float4* __restrict__ src,
                                                           const int* __restrict__ counts, const PoseState* __restrict__ st, int max_n,
                                                           double* __restrict__ partials, int pts, const int* __restrict__ active,
                                                           const int* __restrict__ src_of, Rule rule) {
    const int scan = active ? active[blockIdx.y] : (int)blockIdx.y;
    if (st[scan].done) return;
    unsigned long long tbits = 0;  // the set's rule: the key bits of this scan's target
    if constexpr (std::is_same_v<Rule, NdtVoxelSet>) tbits = ndt_set_target_bits(rule.pair_target[scan]);
    double acc[28];
#pragma unroll
    for (int v = 0; v < 28; ++v) acc[v] = 0.0;
#pragma unroll 1
    for (int pp = 0; pp < pts; ++pp) {  // several points per thread before the 28-value block reduction (≈ as costly as a point)
    const int i = (blockIdx.x * pts + pp) * kBlock + threadIdx.x;
    if (i < counts[scan]) {
        const float4 p = src[src_index(src_of, scan, max_n, i)];
        const D3 q{(double)p.x, (double)p.y, (double)p.z};
        const D3 qs = se3_apply(st[scan].q, st[scan].t, q);
        int kx, ky, kz;
        ndt_key_of(qs, inv_voxel, kx, ky, kz);
        // nearby_grids_ order (ndt cpp:57-58): (0,0,0) (-1,0,0) (1,0,0) (0,1,0) (0,-1,0) (0,0,-1) (0,0,1)
        const int ox[7] = {0, -1, 1, 0, 0, 0, 0}, oy[7] = {0, 0, 0, 1, -1, 0, 0}, oz[7] = {0, 0, 0, 0, 0, -1, 1};
        double n_acc = 0.0;
        D3 esum{0.0, 0.0, 0.0};
        // The seven voxels of a point are independent look-ups. Written as a loop with `continue`, they ran one after the other. Here
        // the first probe of the open-addressing table is issued for all seven (one 16-byte load returns key and voxel index), then
        // the few collisions one by one (four slots to a cache line: the walk rarely leaves the line), then the seven records (one
        // 128-byte line each); the acceptance test is a select and the sums are formed in the reference's order j = 0..6 from the
        // same numbers.
        unsigned long long key[7], kk[7];
        unsigned int vx[7];
        size_t hs[7];
        bool found[7];
        if constexpr (std::is_same_v<Rule, NdtOneTarget>) {
            // the packed key is linear in the coordinates (ndt_pack): a face neighbour's key is the centre's ± one constant, and it is in
            // range when the centre is and the one coordinate that moved still is
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
            // the set's key is linear in the coordinates and formed in signed arithmetic (ndt_set_pack): key0 + delta is the probed voxel's
            // key whenever THAT voxel is in the set's range, wherever the centre lies within the ordinary range. So a probe is valid iff
            // its OWN three coordinates are in the set's ±2^15 range and the centre is within the ordinary ±2^20 (the rule above). A
            // voxel outside the set's range is in no target of the set, so a table of that target alone does not hold it either — but a
            // query just outside whose face neighbour is inside must still probe that neighbour, as it does there.
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
            if (found[j] && kk[j] != key[j] && kk[j] != kNdtEmpty) {  // collision on the first probe: walk on (load factor ≤ 0.5)
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
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const NdtRecord& R = rec[found[j] ? vx[j] : 0u];  // a voxel that is not there (never seen, or dropped for having too few points, ndt cpp:136-142) reads record 0 and is not accepted
            const double* m = R.mu;
            const double* I = R.info;
            const D3 e{qs.x - m[0], qs.y - m[1], qs.z - m[2]};
            // e.transpose() * v.info_ * e (ndt cpp:416) = (eᵀ·info)·e: the row vector first, then its dot product with e — 12 + 8 FP64
            // operations in three short chains (a sum over the nine e_r·info_rc·e_c terms is 27 in one long chain)
            const double t0 = (e.x * I[0] + e.y * I[3]) + e.z * I[6];
            const double t1 = (e.x * I[1] + e.y * I[4]) + e.z * I[7];
            const double t2 = (e.x * I[2] + e.y * I[5]) + e.z * I[8];
            const double res = (t0 * e.x + t1 * e.y) + t2 * e.z;
            const bool accept = found[j] && !(isnan(res) || res > res_th);
            n_acc = accept ? n_acc + 1.0 : n_acc;
            esum.x = accept ? esum.x + e.x : esum.x;
            esum.y = accept ? esum.y + e.y : esum.y;
            esum.z = accept ? esum.z + e.z : esum.z;
        }
        acc[27] += 1.0;  // effective_num++ once per source point (ndt cpp:432)
        if (n_acc > 0.0) {
            double Rh[3][3];  // R·hat(q); the zeros of hat() drop out exactly
            const double* R = st[scan].R;
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                Rh[r][0] = R[3 * r + 1] * q.z - R[3 * r + 2] * q.y;
                Rh[r][1] = R[3 * r + 2] * q.x - R[3 * r + 0] * q.z;
                Rh[r][2] = R[3 * r + 0] * q.y - R[3 * r + 1] * q.x;
            }
            // J = [A | I3] with A = −R·hat(q) (ndt cpp:413-416). The reference forms JᵀJ and Jᵀe entry by entry; with the identity block
            // written out, ((J0a·J0b) + J1a·J1b) + J2a·J2b is A's column product for a, b < 3, the element A[b−3][a] for a < 3 ≤ b (the
            // two products with 0.0 add nothing), 1 on the rest of the diagonal and 0 elsewhere — the same sums bit for bit (up to the
            // sign of a zero), a third of the FP64 instructions: x·0.0 is not something the compiler may drop on its own.
            double A[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) A[r][c] = -Rh[r][c];
            const double ev[3] = {esum.x, esum.y, esum.z};
            int o = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b) {
                    if (a < 3 && b < 3) {
                        double s = A[0][a] * A[0][b];
                        s += A[1][a] * A[1][b];
                        s += A[2][a] * A[2][b];
                        acc[o] += n_acc * s;  // the same J for every accepted voxel of this point
                    } else if (a < 3) {
                        acc[o] += n_acc * A[b - 3][a];
                    } else if (a == b) {
                        acc[o] += n_acc;
                    }
                    ++o;
                }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                double s = -A[0][a] * ev[0];
                s += -A[1][a] * ev[1];
                s += -A[2][a] * ev[2];
                acc[21 + a] += s;
            }
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[24 + c] += -ev[c];
        }
    }
    }
    block_reduce_store<28, kAccW>(acc, partials + ((size_t)scan * gridDim.x + blockIdx.x) * kAccW);
}

int launch_ndt_accum(const NdtTable* t, const float4* src, const int* counts, const PoseState* st, int max_n, int n_scans, double* partials,
                     hipStream_t s, const int* active, int n_active, int split_scans, const int* src_of, const uint32_t* pair_target) {
    const int blocks = (max_n + kBlock - 1) / kBlock;
    const long total_blocks = (long)blocks * (split_scans > 0 ? split_scans : n_scans);  // the split — the order of the sums — never depends on `active`
    const int pts = total_blocks >= 8192 ? 8 : (total_blocks >= 4096 ? 4 : (total_blocks >= 2048 ? 2 : 1));
    dim3 grid((blocks + pts - 1) / pts, active ? n_active : n_scans);
    if (pair_target)
        hipLaunchKernelGGL(ndt_accum_kernel<NdtVoxelSet>, grid, dim3(kBlock), 0, s, t->d_slots, t->d_rec, t->cap - 1, t->inv_voxel, t->res_outlier_th,
                           t->n_nearby, src, counts, st, max_n, partials, pts, active, src_of, NdtVoxelSet{pair_target});
    else
        hipLaunchKernelGGL(ndt_accum_kernel<NdtOneTarget>, grid, dim3(kBlock), 0, s, t->d_slots, t->d_rec, t->cap - 1, t->inv_voxel, t->res_outlier_th,
                           t->n_nearby, src, counts, st, max_n, partials, pts, active, src_of, NdtOneTarget{});
    return (int)grid.x;  // partial blocks per scan
}

}  // namespace locgpu
