// loc_lib_amd/csrc/ndt_pairs.hip — pairwise batch NDT on gfx950 (ndt_pairs.hpp): the voxel-set build. The kernels that look every scan
// up in a grid of its own are the ordinary ones under the set's key rule (ndt_kernels.hip, ndt_fitness.hip).
//
// The reference's scan-to-scan NDT odometry (slam_demo/src/apps/test_node.cpp:317-374) runs SetInputTarget(last_cloud) — that is
// SetDirectNdtTargetCloud, ndt_registration.cpp:65-85, 87-148 — and ScanMatch from the identity (AlignNdt, :374-464) per scan. Here the
// n grids are built in ONE pass of the ordinary build's sequence: key (target above voxel, written here) → the front's grouping half
// (NdtIngest::group: one stable sort → heads → exclusive sum → runs) → kept-voxel flags → exclusive sum → records. The sort is stable,
// so a voxel's points stay in input order and ndt_mean_scatter / ndt_voxel_record give every voxel the bits of its target's single
// build; records are numbered by the second sum, so they are dense, deterministic and in (target, key) order. The only atomic is the
// slot claim's atomicCAS.
#include <algorithm>

#include "device_prims.hpp"
#include "icp_kernels.hpp"
#include "ndt_ingest.hpp"
#include "ndt_pairs.hpp"

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

// One thread per run of the grouped keys: first_run[t] = the first run of target t (the sort puts a target's runs side by side),
// first_run[n_targets] = the number of runs, from the front's counter
__global__ __launch_bounds__(kBlock) void ndt_set_runs_kernel(const unsigned long long* __restrict__ skey, const uint32_t* __restrict__ ustart, const int* __restrict__ ctr,
                                                              unsigned n_targets, int* __restrict__ first_run) {
    const size_t u = (size_t)blockIdx.x * kBlock + threadIdx.x;
    const int runs = ctr[kIngRuns];
    if (u == 0) first_run[n_targets] = runs;
    if (u >= (size_t)runs) return;
    const unsigned t = (unsigned)(skey[ustart[u]] >> 48);
    if (t < n_targets && (u == 0 || (unsigned)(skey[ustart[u - 1]] >> 48) != t)) first_run[t] = (int)u;
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
        const size_t h = ndt_claim_slot(slots, key, cap_mask);
        const unsigned int v = (unsigned int)vid[u];
        slots[h].vid = v;
        return v;
    });
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
    LOCGPU_TRY(ing.group(d_pts, total, s));  // the ordinary build's sort → heads → sum → runs, over the set's keys
    hipLaunchKernelGGL(ndt_set_runs_kernel, dim3(grid), dim3(kBlock), 0, s, ing.skey, ing.ustart, ing.ctr, nt, d_first_run);
    // head and uid have done their work: they now hold the kept-voxel flag of every run and its exclusive sum, the record index
    int* const d_kept = ing.head.get();
    int* const d_vid = ing.uid.get();
    hipLaunchKernelGGL(ndt_set_kept_kernel, dim3(grid1), dim3(kBlock), 0, s, ing.skey, ing.ustart, d_first_run, nt, total, min_pts_in_voxel, d_kept);
    size_t tb = ing.temp.cap();
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
    NdtTable nt_table;
    LOCGPU_TRY(ndt_table_alloc(nt_table, runs, std::max<size_t>(n_vox, 1), s));  // sized by the runs of all targets together
    nt_table.n_vox = n_vox;
    nt_table.inv_voxel = inv_voxel;
    if (runs > 0)
        hipLaunchKernelGGL(ndt_set_voxel_kernel, dim3((unsigned)((runs + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, ing.skey, ing.psorted, ing.ustart, (int)runs, min_pts_in_voxel,
                           d_vid, nt_table.d_slots, nt_table.d_rec, nt_table.cap - 1);
    LOCGPU_TRY(hipGetLastError());
    LOCGPU_TRY(hipStreamSynchronize(s));
    t = std::move(nt_table);
    return hipSuccess;
}

hipError_t ndt_set_dump(const NdtTable& t, size_t first, size_t n, int* keys, double* mu, double* info, hipStream_t s) {
    return ndt_dump_range(t, first, n, true, keys, mu, info, s);
}

}  // namespace locgpu
