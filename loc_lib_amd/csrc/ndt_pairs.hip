// loc_lib_amd/csrc/ndt_pairs.hip — pairwise batch NDT on gfx950 (ndt_pairs.hpp): the voxel-set build and the accumulate and fitness
// kernels that look every scan up in a grid of its own.
//
// The reference's scan-to-scan NDT odometry (slam_demo/src/apps/test_node.cpp:317-374) runs SetInputTarget(last_cloud) — that is
// SetDirectNdtTargetCloud, ndt_registration.cpp:65-85, 87-148 — and ScanMatch from the identity (AlignNdt, :374-464) per scan. Here the
// n grids are built in ONE pass of the ordinary build's sequence (ndt_ingest.hpp): key (target above voxel) → one stable sort → heads →
// exclusive sum → runs → kept-voxel flags → exclusive sum → records. The sort is stable, so a voxel's points stay in input order and
// ndt_mean_scatter / ndt_voxel_record give every voxel the bits of its target's single build; records are numbered by the second
// sum, so they are dense, deterministic and in (target, key) order. The only atomic is the slot claim's atomicCAS.
#include <algorithm>

#include "device_prims.hpp"
#include "icp_kernels.hpp"
#include "launch.hpp"
#include "ndt_ingest.hpp"
#include "ndt_pairs.hpp"

#ifndef LOCGPU_NDT_WAVES
#define LOCGPU_NDT_WAVES 4
#endif
namespace locgpu {

// Key of point i of target blockIdx.y under that target's bits; kNdtEmpty, and bad[target] raised, for a point outside the set's
// ±2^15-voxel range. Points are written behind one another (off[t] + i) whatever the source's layout; pidx keeps the source index.
__global__ __launch_bounds__(kBlock) void ndt_set_key_kernel(const float4* __restrict__ pts, size_t scan_stride, const uint32_t* __restrict__ off, double inv,
                                                             unsigned long long* __restrict__ pkey, uint32_t* __restrict__ pidx, int* __restrict__ bad) {
    const uint32_t t = blockIdx.y;
    const uint32_t o = off[t], cnt = off[t + 1] - o;
    const uint32_t i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= cnt) return;
    const size_t si = scan_stride ? (size_t)t * scan_stride + i : (size_t)o + i;
    const float4 p = pts[si];
    int kx, ky, kz;
    ndt_key_of(D3{(double)p.x, (double)p.y, (double)p.z}, inv, kx, ky, kz);
    unsigned long long key = kNdtEmpty;
    if (!ndt_set_key_in_range(kx, ky, kz)) bad[t] = 1;
    else key = ndt_set_pack(ndt_set_target_bits(t), kx, ky, kz);
    pkey[o + i] = key;
    pidx[o + i] = (uint32_t)si;
}

// sorted keys → 1 at the first point of every run
__global__ __launch_bounds__(kBlock) void ndt_set_head_kernel(const unsigned long long* __restrict__ skey, size_t n, int* __restrict__ head) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    head[i] = (i == 0 || skey[i] != skey[i - 1]) ? 1 : 0;
}

// run u: first sorted position; ustart[runs] = n; the points in voxel order; first_run[t] = the first run of target t (the sort puts a
// target's runs side by side), first_run[n_targets] = the number of runs
__global__ __launch_bounds__(kBlock) void ndt_set_runs_kernel(const unsigned long long* __restrict__ skey, const uint32_t* __restrict__ sidx, const int* __restrict__ head,
                                                              const int* __restrict__ uid, size_t n, const float4* __restrict__ pts, uint32_t* __restrict__ ustart,
                                                              float4* __restrict__ psorted, unsigned n_targets, int* __restrict__ first_run) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    psorted[i] = pts[sidx[i]];
    if (head[i]) {
        ustart[uid[i]] = (uint32_t)i;
        const unsigned t = (unsigned)(skey[i] >> 48);
        if (t < n_targets && (i == 0 || (unsigned)(skey[i - 1] >> 48) != t)) first_run[t] = uid[i];
    }
    if (i == n - 1) {
        const int runs = uid[i] + head[i];
        ustart[runs] = (uint32_t)n;
        first_run[n_targets] = runs;
    }
}

// kept[u] = run u becomes a record (count > min_pts_in_voxel_, ndt cpp:111,137), for all n + 1 entries the sum behind it reads
__global__ __launch_bounds__(kBlock) void ndt_set_kept_kernel(const unsigned long long* __restrict__ skey, const uint32_t* __restrict__ ustart, const int* __restrict__ first_run,
                                                              unsigned n_targets, size_t n, int min_pts, int* __restrict__ kept) {
    const size_t u = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (u > n) return;
    int k = 0;
    if (u < (size_t)first_run[n_targets]) {
        const uint32_t b = ustart[u], e = ustart[u + 1];
        k = (skey[b] != kNdtEmpty && (int)(e - b) > min_pts) ? 1 : 0;
    }
    kept[u] = k;
}

// the read-back: per target {points, runs, records, bad-key flag}; entry n_targets holds the totals
__global__ __launch_bounds__(kBlock) void ndt_set_info_kernel(const uint32_t* __restrict__ off, const int* __restrict__ first_run, const int* __restrict__ vid,
                                                              const int* __restrict__ bad, unsigned n_targets, NdtSetTarget* __restrict__ info) {
    const unsigned t = blockIdx.x * kBlock + threadIdx.x;
    if (t > n_targets) return;
    const int r0 = t < n_targets ? first_run[t] : 0, r1 = t < n_targets ? first_run[t + 1] : first_run[n_targets];
    NdtSetTarget o;
    o.points = t < n_targets ? (int)(off[t + 1] - off[t]) : (int)off[n_targets];
    o.runs = r1 - r0;
    o.voxels = vid[r1] - vid[r0];
    o.bad_key = t < n_targets ? bad[t] : 0;
    info[t] = o;
}

// One thread per run that becomes a record: ndt_voxel_kernel's arithmetic (ndt_voxel_record), the record at the index the sum gave it.
__global__ __launch_bounds__(kBlock) void ndt_set_voxel_kernel(const unsigned long long* __restrict__ skey, const float4* __restrict__ psorted, const uint32_t* __restrict__ ustart,
                                                               int n_runs, int min_pts, const int* __restrict__ vid, NdtSlot* __restrict__ slots, NdtRecord* __restrict__ rec,
                                                               size_t cap_mask) {
    const int u = blockIdx.x * kBlock + threadIdx.x;
    if (u >= n_runs) return;
    const uint32_t b = ustart[u], e = ustart[u + 1];
    const uint32_t len = e - b;
    const unsigned long long key = skey[b];
    if (key == kNdtEmpty || (int)len <= min_pts) return;  // count > min_pts_in_voxel_ (ndt cpp:111,137)
    ndt_voxel_record(key, psorted, b, e, rec, [&]() -> unsigned int {
        // claim a table slot (keys are distinct: a first probe that finds the slot taken walks on)
        size_t h = ndt_hash32(key, cap_mask);
        for (;;) {
            const unsigned long long prev = atomicCAS(&slots[h].key, kNdtEmpty, key);
            if (prev == kNdtEmpty) break;
            h = (h + 1) & cap_mask;
        }
        const unsigned int v = (unsigned int)vid[u];
        slots[h].vid = v;
        return v;
    });
}

// Read-back for tests: records [first, first + n) as dense arrays, the key without its target.
__global__ __launch_bounds__(kBlock) void ndt_set_dump_kernel(const NdtRecord* __restrict__ rec, size_t n, int* __restrict__ keys, double* __restrict__ mu, double* __restrict__ info) {
    const size_t o = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (o >= n) return;
    const NdtRecord& R = rec[o];
    int t, x, y, z;
    ndt_set_unpack(R.key, t, x, y, z);
    keys[3 * o + 0] = x; keys[3 * o + 1] = y; keys[3 * o + 2] = z;
    for (int k = 0; k < 3; ++k) mu[3 * o + k] = R.mu[k];
    for (int k = 0; k < 9; ++k) info[9 * o + k] = R.info[k];
}

hipError_t ndt_set_build(NdtTable& t, const float4* d_pts, size_t scan_stride, const int* counts, int n_targets, double voxel_size, int min_pts_in_voxel, hipStream_t s,
                         std::vector<NdtSetTarget>& info, int* bad_target) {
    *bad_target = -1;
    if (n_targets < 1 || n_targets > kNdtSetMaxTargets) return hipErrorInvalidValue;
    const unsigned nt = (unsigned)n_targets;
    std::vector<uint32_t> off((size_t)nt + 1, 0u);
    size_t total = 0, max_cnt = 0;
    for (unsigned j = 0; j < nt; ++j) {
        if (counts[j] < 1 || (scan_stride && (size_t)counts[j] > scan_stride)) return hipErrorInvalidValue;
        off[j] = (uint32_t)total;
        total += (size_t)counts[j];
        max_cnt = std::max(max_cnt, (size_t)counts[j]);
        if (total > kNdtSetMaxPoints) return hipErrorInvalidValue;
    }
    off[nt] = (uint32_t)total;
    if (scan_stride && (size_t)nt * scan_stride > 0xFFFFFFF0ull) return hipErrorInvalidValue;  // pidx holds source indices in 32 bits
    const double inv_voxel = 1.0 / voxel_size;  // the reference's constructors recompute it (ndt cpp:15,25)
    NdtIngest ing;  // local: allocated per build, freed on return
    LOCGPU_TRY(ing.reserve(total + 1, false));
    DevBuf<uint32_t> d_off;
    DevBuf<int> d_first_run, d_bad;
    DevBuf<NdtSetTarget> d_info;
    LOCGPU_TRY(d_off.alloc((size_t)nt + 1));
    LOCGPU_TRY(d_first_run.alloc((size_t)nt + 1));
    LOCGPU_TRY(d_bad.alloc(nt));
    LOCGPU_TRY(d_info.alloc((size_t)nt + 1));
    LOCGPU_TRY(hipMemcpyAsync(d_off, off.data(), ((size_t)nt + 1) * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    LOCGPU_TRY(hipMemsetAsync(d_first_run, 0, ((size_t)nt + 1) * sizeof(int), s));
    LOCGPU_TRY(hipMemsetAsync(d_bad, 0, (size_t)nt * sizeof(int), s));
    const unsigned grid = (unsigned)((total + kBlock - 1) / kBlock), grid1 = (unsigned)((total + 1 + kBlock - 1) / kBlock);
    hipLaunchKernelGGL(ndt_set_key_kernel, dim3((unsigned)((max_cnt + kBlock - 1) / kBlock), nt), dim3(kBlock), 0, s, d_pts, scan_stride, d_off, inv_voxel, ing.pkey, ing.pidx,
                       d_bad);
    size_t tb = ing.temp.cap();
    LOCGPU_TRY(prim::sort_pairs(ing.temp, tb, ing.pkey.get(), ing.skey.get(), ing.pidx.get(), ing.sidx.get(), total, 0, 64, s));  // stable: a voxel's points keep their input order
    hipLaunchKernelGGL(ndt_set_head_kernel, dim3(grid), dim3(kBlock), 0, s, ing.skey, total, ing.head);
    tb = ing.temp.cap();
    LOCGPU_TRY(prim::exclusive_sum(ing.temp, tb, ing.head.get(), ing.uid.get(), total, s));
    hipLaunchKernelGGL(ndt_set_runs_kernel, dim3(grid), dim3(kBlock), 0, s, ing.skey, ing.sidx, ing.head, ing.uid, total, d_pts, ing.ustart, ing.psorted, nt, d_first_run);
    // head and uid have done their work: they now hold the kept-voxel flag of every run and its exclusive sum, the record index
    int* const d_kept = ing.head.get();
    int* const d_vid = ing.uid.get();
    hipLaunchKernelGGL(ndt_set_kept_kernel, dim3(grid1), dim3(kBlock), 0, s, ing.skey, ing.ustart, d_first_run, nt, total, min_pts_in_voxel, d_kept);
    tb = ing.temp.cap();
    LOCGPU_TRY(prim::exclusive_sum(ing.temp, tb, d_kept, d_vid, total + 1, s));
    hipLaunchKernelGGL(ndt_set_info_kernel, dim3((nt + 1 + kBlock - 1) / kBlock), dim3(kBlock), 0, s, d_off, d_first_run, d_vid, d_bad, nt, d_info);
    LOCGPU_TRY(hipGetLastError());
    std::vector<NdtSetTarget> h_info((size_t)nt + 1);
    LOCGPU_TRY(hipMemcpyAsync(h_info.data(), d_info, ((size_t)nt + 1) * sizeof(NdtSetTarget), hipMemcpyDeviceToHost, s));
    LOCGPU_TRY(hipStreamSynchronize(s));  // the one read-back
    info.assign(h_info.begin(), h_info.begin() + nt);
    for (unsigned j = 0; j < nt; ++j)
        if (h_info[j].bad_key) { *bad_target = (int)j; return hipSuccess; }
    const size_t runs = (size_t)h_info[nt].runs, n_vox = (size_t)h_info[nt].voxels;
    // ndt_build's rule (ndt_kernels.hip, where it says why the table is sparse), applied to the runs of all targets together
    size_t cap = 1024;
    while (cap < 32 * runs && cap < ((size_t)1 << 26)) cap <<= 1;
    while (cap < 2 * runs) cap <<= 1;
    NdtTable nt_table;
    LOCGPU_TRY(nt_table.d_slots.alloc(cap));
    LOCGPU_TRY(nt_table.d_rec.alloc(std::max<size_t>(n_vox, 1)));
    nt_table.cap = cap;
    nt_table.n_vox = n_vox;
    nt_table.inv_voxel = inv_voxel;
    hipLaunchKernelGGL(ndt_fill_kernel<NdtSlot>, dim3((unsigned)((cap + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, nt_table.d_slots.get(), cap, NdtSlot{kNdtEmpty, 0u, 0u});
    LOCGPU_TRY(hipMemsetAsync(nt_table.d_rec, 0, std::max<size_t>(n_vox, 1) * sizeof(NdtRecord), s));  // record 0 is read for voxels that are not there: finite numbers, never accepted
    if (runs > 0)
        hipLaunchKernelGGL(ndt_set_voxel_kernel, dim3((unsigned)((runs + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ing.skey, ing.psorted, ing.ustart, (int)runs, min_pts_in_voxel,
                           d_vid, nt_table.d_slots, nt_table.d_rec, cap - 1);
    LOCGPU_TRY(hipGetLastError());
    LOCGPU_TRY(hipStreamSynchronize(s));
    t = std::move(nt_table);
    return hipSuccess;
}

hipError_t ndt_set_dump(const NdtTable& t, size_t first, size_t n, int* keys, double* mu, double* info, hipStream_t s) {
    if (!t.d_rec || n == 0) return hipSuccess;
    if (first + n > t.n_vox) return hipErrorInvalidValue;
    DevBuf<int> d_keys;
    DevBuf<double> d_mu, d_info;
    LOCGPU_TRY(d_keys.alloc(n * 3));
    LOCGPU_TRY(d_mu.alloc(n * 3));
    LOCGPU_TRY(d_info.alloc(n * 9));
    hipLaunchKernelGGL(ndt_set_dump_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, t.d_rec.get() + first, n, d_keys, d_mu, d_info);
    if (keys) LOCGPU_TRY(hipMemcpyAsync(keys, d_keys, n * 3 * sizeof(int), hipMemcpyDeviceToHost, s));
    if (mu) LOCGPU_TRY(hipMemcpyAsync(mu, d_mu, n * 3 * sizeof(double), hipMemcpyDeviceToHost, s));
    if (info) LOCGPU_TRY(hipMemcpyAsync(info, d_info, n * 9 * sizeof(double), hipMemcpyDeviceToHost, s));
    LOCGPU_TRY(hipStreamSynchronize(s));
    return hipSuccess;
}

// ---------------------------------------------------------------------------------------------
// K5 for pairs. Grid (ceil(max_n/256), n_scans). This is ndt_accum_kernel (ndt_kernels.hip, where it says why the look-up is a copy and
// not a shared function) with one difference: the scan reads the word of its target (pair_target[scan], uniform over the block) and
// forms its seven keys under that target's bits, in the set's key (ndt_set_key.hpp). Probe order, gate, record 0 for absent voxels,
// the point loop, active / n_active and the partial layout are the ordinary kernel's, so gn_solve_kernel sums the same numbers.
// Range: a probe is valid iff its OWN three coordinates are in the set's ±2^15 range and the centre is within the ordinary ±2^20 (the
// ordinary kernel's rule). A voxel outside the set's range is in no target of the set, so the ordinary path does not find it either —
// but a query just outside whose face neighbour is inside must still probe that neighbour, as it does there.
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(LOCGPU_NDT_WAVES, LOCGPU_NDT_WAVES))) void ndt_accum_pairs_kernel(
    const NdtSlot* __restrict__ slots, const NdtRecord* __restrict__ rec, size_t cap_mask, double inv_voxel, double res_th, int n_nearby, const float4* __restrict__ src,
    const int* __restrict__ counts, const PoseState* __restrict__ st, int max_n, double* __restrict__ partials, int pts, const int* __restrict__ active,
    const int* __restrict__ src_of, const uint32_t* __restrict__ pair_target) {
    const int scan = active ? active[blockIdx.y] : (int)blockIdx.y;
    if (st[scan].done) return;
    const unsigned long long tbits = ndt_set_target_bits(pair_target[scan]);
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
        unsigned long long key[7], kk[7];
        unsigned int vx[7];
        size_t hs[7];
        bool found[7];
        // the set's key is linear in the coordinates and formed in signed arithmetic (ndt_set_pack): key0 + delta is the probed voxel's
        // key whenever THAT voxel is in the set's range, wherever the centre lies within the ordinary range
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
            const NdtRecord& R = rec[found[j] ? vx[j] : 0u];  // a voxel that is not there reads record 0 and is not accepted
            const double* m = R.mu;
            const double* I = R.info;
            const D3 e{qs.x - m[0], qs.y - m[1], qs.z - m[2]};
            // e.transpose() * v.info_ * e (ndt cpp:416) with ndt_accum_kernel's association
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
            // J = [A | I3] with A = −R·hat(q) (ndt cpp:413-416), summed entry by entry as ndt_accum_kernel does
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

int launch_ndt_accum_pairs(const NdtTable* t, const uint32_t* pair_target, const float4* src, const int* counts, const PoseState* st, int max_n, int n_scans,
                           double* partials, hipStream_t s, const int* active, int n_active, int split_scans, const int* src_of) {
    // launch_ndt_accum's rule, word for word: the split — the order of the sums — is the ordinary batch's
    const int blocks = (max_n + kBlock - 1) / kBlock;
    const long total_blocks = (long)blocks * (split_scans > 0 ? split_scans : n_scans);
    const int pts = total_blocks >= 8192 ? 8 : (total_blocks >= 4096 ? 4 : (total_blocks >= 2048 ? 2 : 1));
    dim3 grid((blocks + pts - 1) / pts, active ? n_active : n_scans);
    hipLaunchKernelGGL(ndt_accum_pairs_kernel, grid, dim3(kBlock), 0, s, t->d_slots, t->d_rec, t->cap - 1, t->inv_voxel, t->res_outlier_th, t->n_nearby, src, counts, st, max_n,
                       partials, pts, active, src_of, pair_target);
    return (int)grid.x;  // partial blocks per scan
}

// ---------------------------------------------------------------------------------------------
// The score for pairs: ndt_fitness_accum_kernel (ndt_fitness.hip) with the scan's look-ups under its own target, as above.
constexpr int kNdtFitPts = 4;  // = kFitPts of fitness.hip: launch_fitness_sum sums icp_fitness_rows(max_n) rows per scan

__global__ __launch_bounds__(kBlock) void ndt_fitness_pairs_kernel(const NdtSlot* __restrict__ slots, const NdtRecord* __restrict__ rec, size_t cap_mask, double inv_voxel,
                                                                   double res_th, int n_nearby, const float4* __restrict__ src, const int* __restrict__ counts,
                                                                   const PoseState* __restrict__ st, int max_n, double* __restrict__ partials, const int* __restrict__ src_of,
                                                                   const uint32_t* __restrict__ pair_target) {
    __shared__ double s_part[kBlock / 64][kFitW];
    const int scan = blockIdx.y;
    const int n = counts[scan];
    const unsigned long long tbits = ndt_set_target_bits(pair_target[scan]);
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
        // keys and probe validity as in ndt_accum_pairs_kernel
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
            // e.transpose() * v.info_ * e (ndt cpp:416) with the association of ndt_accum_kernel
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
    // ndt_fitness_accum_kernel's reduction: the three butterflies side by side and one guarded store
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

void launch_ndt_fitness_pairs(const NdtTable* t, const uint32_t* pair_target, const float4* src, const int* counts, const PoseState* st, int max_n, int n_scans,
                              double* partials, double* out, hipStream_t s, const int* src_of) {
    static_assert(kNdtFitPts * kBlock == 1024, "the rows launch_fitness_sum adds");
    const int rows = icp_fitness_rows(max_n);
    hipLaunchKernelGGL(ndt_fitness_pairs_kernel, dim3(rows, n_scans), dim3(kBlock), 0, s, t->d_slots, t->d_rec, t->cap - 1, t->inv_voxel, t->res_outlier_th, t->n_nearby, src,
                       counts, st, max_n, partials, src_of, pair_target);
    launch_fitness_sum(partials, rows, n_scans, out, nullptr, s);
}

}  // namespace locgpu
