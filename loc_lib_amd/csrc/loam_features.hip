// loc_lib_amd/csrc/loam_features.hip — LOAM edge / surface feature picker on the GPU.
//
// Replaces LoamFeatureExtract::Extract + ExtractFromSector
// (LocUtils/src/model/feature_extract/loam_feature_extract.cpp:19-91, :93-151), which Lio::AddCloud(FullCloudPtr) runs on every
// scan before the LOAM matcher (lio.cpp:323). Same results, quirks included:
//   * points are bucketed per ring in input order (:27-36); rings with fewer than 131 points are skipped (:40-43);
//   * curvature = squared norm of (sum of the 10 ring neighbours − 10·p), the sums in float32 left to right (:47-69);
//   * six sectors per ring, each WITHOUT its last element (end iterator = begin + sector_end, :73-85);
//   * per sector: sort by curvature, walk from the largest: stop at value ≤ 0.1, at most 20 edges, the 21st pick is marked
//     but emitted nowhere, ±5 ring neighbours are marked while consecutive gaps² ≤ 0.05 (:100-139); every unmarked point of
//     the sector becomes a surface point in ascending curvature (:143-149);
//   * outputs are appended ring by ring, sector by sector.
// The reference's std::sort leaves the order of EQUAL curvatures open; here ties are ordered by ascending ring index.
//
// Mapping: one 256-thread workgroup per (sector, ring): bitonic sort of the sector's (curvature, id) pairs in LDS, the
// inherently sequential pick loop on one lane (≤ 21 picks), ordered compaction of the surface points by ballot/popcount.
#include "device_prims.hpp"

#include <cstring>
#include <string>
#include <vector>

#include "cloud_filters.hpp"
#include "context.hpp"
#include "loam_sector.hpp"

namespace locgpu {

namespace {

using namespace loam;  // kLB, kMaxSector, kMaxEdges and the per-point / per-sector bodies (loam_sector.hpp)

struct LoamParams {
    uint32_t n_edge, n_surf;
    int32_t too_long;  // a sector exceeded kMaxSector
};

__global__ __launch_bounds__(kLB) void ring_key_kernel(const unsigned char* __restrict__ ring, size_t n, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const size_t i = (size_t)blockIdx.x * kLB + threadIdx.x;
    if (i >= n) return;
    keys[i] = ring[i];
    vals[i] = (uint32_t)i;
}

// start[r] = first sorted position with key ≥ r, r = 0..num_scan
__global__ void ring_start_kernel(const uint32_t* __restrict__ keys, uint32_t n, int num_scan, uint32_t* __restrict__ start) {
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r > num_scan) return;
    start[r] = key_lower_bound(keys, n, (uint32_t)r);
}

__global__ __launch_bounds__(kLB) void ring_gather_kernel(const float4* __restrict__ pts, const uint32_t* __restrict__ vals, size_t n, float4* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * kLB + threadIdx.x;
    if (i >= n) return;
    out[i] = pts[vals[i]];
}

// curvature of ring-local index j ∈ [5, size−5) (loam_feature_extract.cpp:47-69); L is the ring-ordered cloud.
__global__ __launch_bounds__(kLB) void curvature_kernel(const float4* __restrict__ L, const uint32_t* __restrict__ ring_start, int num_scan,
                                                        double* __restrict__ curv) {
    const int r = blockIdx.y;
    const uint32_t base = ring_start[r], size = ring_start[r + 1] - base;
    if (size < kMinRing) return;
    const uint32_t j = blockIdx.x * kLB + threadIdx.x + 5;
    if (j + 5 >= size) return;
    curv[base + j] = ring_curvature(L + base + j);
}

// One workgroup per (sector, ring): sector_body (loam_sector.hpp).
__global__ __launch_bounds__(kLB) void sector_kernel(const float4* __restrict__ L, const double* __restrict__ curv, const uint32_t* __restrict__ ring_start,
                                                     float4* __restrict__ edge_slot, float4* __restrict__ surf_slot, uint32_t* __restrict__ edge_cnt,
                                                     uint32_t* __restrict__ surf_cnt, LoamParams* P) {
    const int sec = blockIdx.x, r = blockIdx.y;
    const uint32_t base = ring_start[r], size = ring_start[r + 1] - base;
    sector_body(L, curv, base, size, sec, (size_t)(r * 6 + sec), edge_slot, surf_slot, edge_cnt, surf_cnt, &P->too_long);
}

// exclusive scan of the per-task counts (≤ 256·6 tasks) by one workgroup; totals into P
__global__ __launch_bounds__(kLB) void task_scan_kernel(const uint32_t* __restrict__ edge_cnt, const uint32_t* __restrict__ surf_cnt, int n_tasks,
                                                        uint32_t* __restrict__ edge_off, uint32_t* __restrict__ surf_off, LoamParams* P) {
    if (threadIdx.x != 0) return;
    uint32_t e = 0, s = 0;
    for (int t = 0; t < n_tasks; ++t) {
        edge_off[t] = e; surf_off[t] = s;
        e += edge_cnt[t]; s += surf_cnt[t];
    }
    P->n_edge = e;
    P->n_surf = s;
}

__global__ __launch_bounds__(kLB) void sector_scatter_kernel(const float4* __restrict__ edge_slot, const float4* __restrict__ surf_slot,
                                                             const uint32_t* __restrict__ ring_start, const uint32_t* __restrict__ edge_cnt,
                                                             const uint32_t* __restrict__ surf_cnt, const uint32_t* __restrict__ edge_off,
                                                             const uint32_t* __restrict__ surf_off, float4* __restrict__ edge_out, float4* __restrict__ surf_out) {
    const int sec = blockIdx.x, r = blockIdx.y, task = r * 6 + sec;
    const uint32_t ne = edge_cnt[task], ns = surf_cnt[task];
    if (ne == 0 && ns == 0) return;
    const uint32_t base = ring_start[r], size = ring_start[r + 1] - base;
    const uint32_t src = base + 5 + (uint32_t)sector_start(size, sec);
    for (uint32_t e = threadIdx.x; e < ne; e += kLB) edge_out[edge_off[task] + e] = edge_slot[(size_t)task * kMaxEdges + e];
    for (uint32_t s = threadIdx.x; s < ns; s += kLB) surf_out[surf_off[task] + s] = surf_slot[src + s];
}

}  // namespace

struct LoamScratch {
    size_t cap = 0;  // points the group {d_ring … curv, temp} has room for
    DevBuf<unsigned char> d_ring;
    DevBuf<uint32_t> keys[2], vals[2];
    DevBuf<float4> ring_pts, surf_slot;
    DevBuf<double> curv;
    DevBuf<unsigned char> temp;  // scratch of the sort at `cap` points
    // per (ring, sector) task; edge_slot, grown last, has the capacity of the group
    DevBuf<uint32_t> ring_start, edge_cnt, surf_cnt, edge_off, surf_off;
    DevBuf<float4> edge_slot;
    DevBuf<LoamParams> d_params;
    PinnedBuf<LoamParams> h_params;
};

namespace {

hipError_t ensure(locgpu_ctx* ctx, size_t n, int num_scan) {
    if (!ctx->loam) ctx->loam = new LoamScratch();
    LoamScratch* S = ctx->loam;
    LOCGPU_TRY(S->d_params.reserve(1));
    LOCGPU_TRY(S->h_params.reserve(1));
    const size_t tasks = (size_t)num_scan * 6;
    if (tasks * kMaxEdges > S->edge_slot.cap()) {
        LOCGPU_TRY(S->ring_start.alloc((size_t)num_scan + 1));
        LOCGPU_TRY(S->edge_cnt.alloc(tasks));
        LOCGPU_TRY(S->surf_cnt.alloc(tasks));
        LOCGPU_TRY(S->edge_off.alloc(tasks));
        LOCGPU_TRY(S->surf_off.alloc(tasks));
        LOCGPU_TRY(S->edge_slot.alloc(tasks * kMaxEdges));
    }
    if (n > S->cap) {
        S->cap = 0;
        const size_t cap = with_headroom(n);
        LOCGPU_TRY(S->d_ring.alloc(cap));
        for (int j = 0; j < 2; ++j) {
            LOCGPU_TRY(S->keys[j].alloc(cap));
            LOCGPU_TRY(S->vals[j].alloc(cap));
        }
        LOCGPU_TRY(S->ring_pts.alloc(cap));
        LOCGPU_TRY(S->surf_slot.alloc(cap));
        LOCGPU_TRY(S->curv.alloc(cap));
        size_t tb = 0;
        LOCGPU_TRY(prim::sort_pairs(nullptr, tb, S->keys[0].get(), S->keys[1].get(), S->vals[0].get(), S->vals[1].get(), (int)cap, 0, 8, ctx->stream));
        LOCGPU_TRY(S->temp.alloc(tb + 256));
        S->cap = cap;
    }
    return hipSuccess;
}

}  // namespace

void loam_free(locgpu_ctx* ctx) {
    delete ctx->loam;
    ctx->loam = nullptr;
    batch_loam_free(ctx);
}

// in: cloud resident in HBM; ring: host bytes, one per point. *too_long is set when a sector exceeds the LDS sort capacity.
hipError_t loam_extract_dev(locgpu_ctx* ctx, const locgpu_cloud* in, const unsigned char* ring, int num_scan, locgpu_cloud* edge, locgpu_cloud* surf,
                            bool* too_long) {
    const size_t n = in->n;
    *too_long = false;
    edge->n = 0; edge->is_dense = 1;
    surf->n = 0; surf->is_dense = 1;
    if (n == 0) return hipSuccess;
    LOCGPU_TRY(ensure(ctx, n, num_scan));
    LoamScratch* S = ctx->loam;
    hipStream_t s = ctx->stream;
    const unsigned nb = (unsigned)((n + kLB - 1) / kLB);
    LOCGPU_TRY(hipMemcpyAsync(S->d_ring, ring, n, hipMemcpyHostToDevice, s));
    LOCGPU_TRY(hipMemsetAsync(S->d_params, 0, sizeof(LoamParams), s));
    hipLaunchKernelGGL(ring_key_kernel, dim3(nb), dim3(kLB), 0, s, S->d_ring, n, S->keys[0], S->vals[0]);
    size_t tb = S->temp.cap();
    LOCGPU_TRY(prim::sort_pairs(S->temp, tb, S->keys[0].get(), S->keys[1].get(), S->vals[0].get(), S->vals[1].get(), (int)n, 0, 8, s));  // stable: input order per ring
    hipLaunchKernelGGL(ring_start_kernel, dim3((num_scan + 1 + 63) / 64), dim3(64), 0, s, S->keys[1], (uint32_t)n, num_scan, S->ring_start);
    hipLaunchKernelGGL(ring_gather_kernel, dim3(nb), dim3(kLB), 0, s, in->d, S->vals[1], n, S->ring_pts);
    hipLaunchKernelGGL(curvature_kernel, dim3(nb, num_scan), dim3(kLB), 0, s, S->ring_pts, S->ring_start, num_scan, S->curv);
    hipLaunchKernelGGL(sector_kernel, dim3(6, num_scan), dim3(kLB), 0, s, S->ring_pts, S->curv, S->ring_start, S->edge_slot, S->surf_slot, S->edge_cnt,
                       S->surf_cnt, S->d_params);
    hipLaunchKernelGGL(task_scan_kernel, dim3(1), dim3(kLB), 0, s, S->edge_cnt, S->surf_cnt, num_scan * 6, S->edge_off, S->surf_off, S->d_params);
    LOCGPU_TRY(hipGetLastError());
    LOCGPU_TRY(hipMemcpyAsync(S->h_params, S->d_params, sizeof(LoamParams), hipMemcpyDeviceToHost, s));
    LOCGPU_TRY(hipStreamSynchronize(s));
    if (S->h_params->too_long) { *too_long = true; return hipSuccess; }
    const uint32_t ne = S->h_params->n_edge, ns = S->h_params->n_surf;
    LOCGPU_TRY(cloud_reserve(edge, ne, false));
    LOCGPU_TRY(cloud_reserve(surf, ns, false));
    hipLaunchKernelGGL(sector_scatter_kernel, dim3(6, num_scan), dim3(kLB), 0, s, S->edge_slot, S->surf_slot, S->ring_start, S->edge_cnt, S->surf_cnt,
                       S->edge_off, S->surf_off, edge->d, surf->d);
    LOCGPU_TRY(hipGetLastError());
    LOCGPU_TRY(hipStreamSynchronize(s));
    edge->n = ne;
    surf->n = ns;
    return hipSuccess;
}

}  // namespace locgpu
