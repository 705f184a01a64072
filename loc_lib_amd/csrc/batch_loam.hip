// loc_lib_amd/csrc/batch_loam.hip — the LOAM feature picker on every scan of a batch at once (locgpu_batch_loam_extract).
//
// Lio::AddCloud(FullCloudPtr) runs LoamFeatureExtract::Extract on every scan (lio.cpp:323; loam_feature_extract.cpp:19-151) before
// AlignWithLocalMap filters the two feature clouds (lio.cpp:485-486) and matches them. loam_features.hip does that for ONE resident
// cloud in seven launches, a sort and two stream synchronisations; this is the same pass with a COMPOSITE ring — ring r of scan s is
// ring s · num_scan + r of the batch — in one set of launches and one read-back of n_scans {edge count, surface count, status}:
//
//   keys     slot (s, i) → s · num_scan + ring; padding slots and rings ≥ num_scan → the sentinel n_scans · num_scan   bl_key_kernel
//   sort     ONE stable LSD radix sort of (key, slot) over the [n_scans][max_n] slots, ceil(log2(sentinel + 1)) bits    rocPRIM
//   starts   ring_start[0 .. n_scans · num_scan]: first sorted position of every composite ring                         bl_ring_start_kernel
//   gather   the ring-ordered cloud L (the sentinel's slots are left out)                                               bl_gather_kernel
//   curv     one thread per point of L: ring_curvature (loam_sector.hpp)                                                bl_curvature_kernel
//   sectors  one workgroup per (sector, composite ring): sector_body (loam_sector.hpp) — the single-cloud pass's        bl_sector_kernel
//   offsets  one workgroup per scan: exclusive sums of its 6 · num_scan task counts, its totals and too-long flag       bl_scan_offsets_kernel
//   verdict  one workgroup: does every scan fit both destinations, is no ring too long                                  bl_verdict_kernel
//   scatter  one workgroup per task → dst + s · dst_max_n + offset, {x, y, z, +0}; the device counts                    bl_scatter_kernel
//
// Why the bytes are the single picker's: the sort is stable and a scan's slots are in input order, so a ring's points reach L in input
// order, as there; curvature, sector sort, pick loop and compaction are the SAME device functions on the same operands; the offsets are
// integer sums in ring-then-sector order. Nothing of a scan depends on another scan, on n_scans or on the run, and there are no atomics
// (the too-long flag of a scan is a plain store of 1 by whichever of its sectors find one).
//
// Scratch, grow-only on the context (freed by batch_loam_free): per SLOT ring byte 1 B (+ 1 B pinned), keys 2 × 4 B, values 2 × 4 B,
// L 16 B, surface staging 16 B, curvature 8 B = 57 B, + rocPRIM's sort workspace (≈ 8 B); per TASK (6 per composite ring) two counts and
// two offsets 16 B + 20 staged edges 320 B = 336 B; per composite ring 4 B; per scan 20 B.
#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "batch_upload.hpp"
#include "cloud_filters.hpp"
#include "context.hpp"
#include "device_prims.hpp"
#include "loam_sector.hpp"

namespace locgpu {

namespace {

using namespace loam;

constexpr int kMaxRings = 65535;  // n_scans · num_scan: the y extent of the per-ring grids

__global__ __launch_bounds__(kLB) void bl_key_kernel(const unsigned char* __restrict__ ring, const int* __restrict__ counts, uint32_t max_n, uint32_t num_scan,
                                                     uint32_t sentinel, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t s = blockIdx.y;
    const uint32_t i = blockIdx.x * kLB + threadIdx.x;
    if (i >= max_n) return;
    const size_t slot = (size_t)s * max_n + i;
    uint32_t key = sentinel;
    if (i < (uint32_t)counts[s]) {
        const uint32_t r = ring[slot];
        if (r < num_scan) key = s * num_scan + r;
    }
    keys[slot] = key;
    vals[slot] = (uint32_t)slot;
}

// start[r] = first sorted position with key ≥ r, r = 0..n_rings (start[n_rings] = the number of points in any ring)
__global__ __launch_bounds__(kLB) void bl_ring_start_kernel(const uint32_t* __restrict__ keys, uint32_t n, uint32_t n_rings, uint32_t* __restrict__ start) {
    const uint32_t r = blockIdx.x * kLB + threadIdx.x;
    if (r > n_rings) return;
    start[r] = key_lower_bound(keys, n, r);
}

__global__ __launch_bounds__(kLB) void bl_gather_kernel(const float4* __restrict__ src, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ ring_start,
                                                        uint32_t n_rings, float4* __restrict__ L) {
    const uint32_t j = blockIdx.x * kLB + threadIdx.x;
    if (j >= ring_start[n_rings]) return;
    L[j] = src[vals[j]];
}

// Point j of L, ring-local index j − base ∈ [5, size − 5) (loam_feature_extract.cpp:47-69).
__global__ __launch_bounds__(kLB) void bl_curvature_kernel(const float4* __restrict__ L, const uint32_t* __restrict__ keys, const uint32_t* __restrict__ ring_start,
                                                           uint32_t n_rings, double* __restrict__ curv) {
    const uint32_t j = blockIdx.x * kLB + threadIdx.x;
    if (j >= ring_start[n_rings]) return;
    const uint32_t r = keys[j];
    const uint32_t base = ring_start[r], size = ring_start[r + 1] - base;
    if (size < kMinRing) return;
    const uint32_t local = j - base;
    if (local < 5 || local + 5 >= size) return;
    curv[j] = ring_curvature(L + j);
}

__global__ __launch_bounds__(kLB) void bl_sector_kernel(const float4* __restrict__ L, const double* __restrict__ curv, const uint32_t* __restrict__ ring_start,
                                                        uint32_t num_scan, float4* __restrict__ edge_slot, float4* __restrict__ surf_slot,
                                                        uint32_t* __restrict__ edge_cnt, uint32_t* __restrict__ surf_cnt, int32_t* too_long) {
    const int sec = blockIdx.x;
    const uint32_t r = blockIdx.y;
    const uint32_t base = ring_start[r], size = ring_start[r + 1] - base;
    sector_body(L, curv, base, size, sec, (size_t)r * 6 + sec, edge_slot, surf_slot, edge_cnt, surf_cnt, too_long + r / num_scan);
}

// Scan blockIdx.x: thread t owns ring t's six tasks. Offsets are relative to the scan's first output point; res[s] = {edges,
// surface points, too long, 0}.
__global__ __launch_bounds__(kLB) void bl_scan_offsets_kernel(const uint32_t* __restrict__ edge_cnt, const uint32_t* __restrict__ surf_cnt,
                                                              const int32_t* __restrict__ too_long, uint32_t num_scan, uint32_t* __restrict__ edge_off,
                                                              uint32_t* __restrict__ surf_off, int4* __restrict__ res) {
    static_assert(kLB == 256, "one thread per ring: num_scan <= 256");
    __shared__ uint32_t s_e[kLB / 64], s_s[kLB / 64];
    const uint32_t s = blockIdx.x, t = threadIdx.x;
    const size_t task0 = ((size_t)s * num_scan + t) * 6;
    uint32_t ce[6], cs[6], e = 0, u = 0;
#pragma unroll
    for (int k = 0; k < 6; ++k) {
        ce[k] = t < num_scan ? edge_cnt[task0 + k] : 0u;
        cs[k] = t < num_scan ? surf_cnt[task0 + k] : 0u;
        e += ce[k];
        u += cs[k];
    }
    uint32_t ie = e, iu = u;  // inclusive sums over the wave
    const int lane = t & 63, wave = t >> 6;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t oe = __shfl_up(ie, off, 64), ou = __shfl_up(iu, off, 64);
        if (lane >= off) { ie += oe; iu += ou; }
    }
    if (lane == 63) { s_e[wave] = ie; s_s[wave] = iu; }
    __syncthreads();
    uint32_t be = 0, bu = 0, te = 0, tu = 0;
    for (int w = 0; w < kLB / 64; ++w) {
        be += w < wave ? s_e[w] : 0u;
        bu += w < wave ? s_s[w] : 0u;
        te += s_e[w];
        tu += s_s[w];
    }
    uint32_t xe = be + ie - e, xu = bu + iu - u;  // exclusive
    if (t < num_scan) {
#pragma unroll
        for (int k = 0; k < 6; ++k) {
            edge_off[task0 + k] = xe;
            surf_off[task0 + k] = xu;
            xe += ce[k];
            xu += cs[k];
        }
    }
    if (t == 0) res[s] = int4{(int)te, (int)tu, too_long[s] != 0 ? 1 : 0, 0};
}

// One workgroup: res[n_scans] = {1 when every scan fits both destinations and no ring is too long, else 0; 0, 0, 0}.
__global__ __launch_bounds__(kLB) void bl_verdict_kernel(int4* __restrict__ res, int n_scans, uint32_t edge_max_n, uint32_t surf_max_n) {
    __shared__ int s_bad;
    if (threadIdx.x == 0) s_bad = 0;
    __syncthreads();
    bool bad = false;
    for (int s = threadIdx.x; s < n_scans; s += kLB) {
        const int4 v = res[s];
        bad = bad || (uint32_t)v.x > edge_max_n || (uint32_t)v.y > surf_max_n || v.z != 0;
    }
    if (bad) s_bad = 1;
    __syncthreads();
    if (threadIdx.x == 0) res[n_scans] = int4{s_bad ? 0 : 1, 0, 0, 0};
}

// Task (sector, composite ring) → its scan's rows of the two destinations. Nothing is written when the verdict is 0: the call fails
// and leaves both destinations alone.
__global__ __launch_bounds__(kLB) void bl_scatter_kernel(const float4* __restrict__ edge_slot, const float4* __restrict__ surf_slot,
                                                         const uint32_t* __restrict__ ring_start, const uint32_t* __restrict__ edge_cnt,
                                                         const uint32_t* __restrict__ surf_cnt, const uint32_t* __restrict__ edge_off,
                                                         const uint32_t* __restrict__ surf_off, const int4* __restrict__ res, int n_scans, uint32_t num_scan,
                                                         uint32_t edge_max_n, uint32_t surf_max_n, float4* __restrict__ edge_out, float4* __restrict__ surf_out,
                                                         int* __restrict__ edge_counts, int* __restrict__ surf_counts) {
    if (res[n_scans].x == 0) return;
    const int sec = blockIdx.x;
    const uint32_t r = blockIdx.y, s = r / num_scan;
    const size_t task = (size_t)r * 6 + sec;
    if (sec == 0 && r == s * num_scan && threadIdx.x == 0) {
        edge_counts[s] = res[s].x;
        surf_counts[s] = res[s].y;
    }
    const uint32_t ne = edge_cnt[task], ns = surf_cnt[task];
    if (ne == 0 && ns == 0) return;
    const uint32_t base = ring_start[r], size = ring_start[r + 1] - base;
    const uint32_t from = base + 5 + (uint32_t)sector_start(size, sec);
    float4* __restrict__ eo = edge_out + (size_t)s * edge_max_n + edge_off[task];
    float4* __restrict__ so = surf_out + (size_t)s * surf_max_n + surf_off[task];
    for (uint32_t e = threadIdx.x; e < ne; e += kLB) {
        const float4 p = edge_slot[task * kMaxEdges + e];
        eo[e] = float4{p.x, p.y, p.z, 0.f};
    }
    for (uint32_t k = threadIdx.x; k < ns; k += kLB) {
        const float4 p = surf_slot[from + k];
        so[k] = float4{p.x, p.y, p.z, 0.f};
    }
}

}  // namespace

// Three groups that grow together: per slot {d_ring … curv}, per composite ring {ring_start … edge_slot} and per scan {too_long, res,
// h_res}. The buffer grown last (curv, edge_slot, h_res) has the capacity of its whole group.
struct BatchLoamScratch {
    DevBuf<unsigned char> d_ring;
    PinnedBuf<unsigned char> h_ring;
    DevBuf<uint32_t> keys[2], vals[2];
    DevBuf<float4> L, surf_slot;
    DevBuf<double> curv;
    DevBuf<unsigned char> temp;
    DevBuf<uint32_t> ring_start, edge_cnt, surf_cnt, edge_off, surf_off;
    DevBuf<float4> edge_slot;
    DevBuf<int32_t> too_long;
    DevBuf<int4> res;  // [scans + 1]
    PinnedBuf<int4> h_res;
};

namespace {

hipError_t ensure(locgpu_ctx* ctx, size_t n, size_t n_rings, int n_scans, unsigned end_bit) {
    if (!ctx->bloam) ctx->bloam = new BatchLoamScratch();
    BatchLoamScratch* S = ctx->bloam;
    if ((size_t)n_scans + 1 > S->h_res.cap()) {
        const size_t cap = (size_t)n_scans + 16;
        LOCGPU_TRY(S->too_long.alloc(cap));
        LOCGPU_TRY(S->res.alloc(cap + 1));
        LOCGPU_TRY(S->h_res.alloc(cap + 1));
    }
    if (n_rings * 6 * kMaxEdges > S->edge_slot.cap()) {
        const size_t cap = n_rings + n_rings / 4 + 64, tasks = cap * 6;
        LOCGPU_TRY(S->ring_start.alloc(cap + 1));
        LOCGPU_TRY(S->edge_cnt.alloc(tasks));
        LOCGPU_TRY(S->surf_cnt.alloc(tasks));
        LOCGPU_TRY(S->edge_off.alloc(tasks));
        LOCGPU_TRY(S->surf_off.alloc(tasks));
        LOCGPU_TRY(S->edge_slot.alloc(tasks * kMaxEdges));
    }
    if (n > S->curv.cap()) {
        const size_t cap = with_headroom(n);
        LOCGPU_TRY(S->d_ring.alloc(cap));
        LOCGPU_TRY(S->h_ring.alloc(cap));
        for (int j = 0; j < 2; ++j) {
            LOCGPU_TRY(S->keys[j].alloc(cap));
            LOCGPU_TRY(S->vals[j].alloc(cap));
        }
        LOCGPU_TRY(S->L.alloc(cap));
        LOCGPU_TRY(S->surf_slot.alloc(cap));
        LOCGPU_TRY(S->curv.alloc(cap));
    }
    size_t tb = 0;
    LOCGPU_TRY(prim::sort_pairs((void*)nullptr, tb, S->keys[0].get(), S->keys[1].get(), S->vals[0].get(), S->vals[1].get(), n, 0, end_bit, ctx->stream));
    const size_t need = tb + 256;
    if (need > S->temp.cap()) LOCGPU_TRY(S->temp.alloc(need + need / 4));
    return hipSuccess;
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + kLB - 1) / kLB); }

// The launches of one pass; the result rows are on their way to S->h_res when it returns. The ring bytes come from the host arrays
// `rings`, or — rings == nullptr — are the ones locgpu_batch_upload_ranges left in src->d_rings, in the same [n_scans][max_n] layout.
hipError_t extract_dev(locgpu_ctx* ctx, locgpu_batch* src, const uint8_t* const* rings, int num_scan, locgpu_batch* edge, locgpu_batch* surf) {
    hipStream_t s = ctx->stream;
    const int n_scans = src->n_scans;
    const uint32_t max_n = (uint32_t)src->max_n, edge_max_n = (uint32_t)edge->max_n, surf_max_n = (uint32_t)surf->max_n;
    const size_t n = src->pitch;
    const uint32_t n_rings = (uint32_t)n_scans * (uint32_t)num_scan;  // also the sentinel key
    unsigned end_bit = 1;
    while ((1u << end_bit) <= n_rings) ++end_bit;
    LOCGPU_TRY(ensure(ctx, n, n_rings, n_scans, end_bit));
    BatchLoamScratch* S = ctx->bloam;
    const unsigned char* d_ring = src->d_rings;
    if (rings) {
        for (int i = 0; i < n_scans; ++i)
            if (src->counts[i] > 0) std::memcpy(S->h_ring + (size_t)i * max_n, rings[i], (size_t)src->counts[i]);
        LOCGPU_TRY(hipMemcpyAsync(S->d_ring, S->h_ring, n, hipMemcpyHostToDevice, s));
        d_ring = S->d_ring;
    }
    LOCGPU_TRY(hipMemsetAsync(S->too_long, 0, (size_t)n_scans * sizeof(int32_t), s));
    hipLaunchKernelGGL(bl_key_kernel, dim3(blocks_for(max_n), n_scans), dim3(kLB), 0, s, d_ring, src->d_counts, max_n, (uint32_t)num_scan, n_rings, S->keys[0],
                       S->vals[0]);
    LOCGPU_TRY(hipGetLastError());
    size_t tb = S->temp.cap();
    LOCGPU_TRY(prim::sort_pairs(S->temp, tb, S->keys[0].get(), S->keys[1].get(), S->vals[0].get(), S->vals[1].get(), n, 0, end_bit, s));  // stable: input order per ring
    hipLaunchKernelGGL(bl_ring_start_kernel, dim3(blocks_for((size_t)n_rings + 1)), dim3(kLB), 0, s, S->keys[1], (uint32_t)n, n_rings, S->ring_start);
    hipLaunchKernelGGL(bl_gather_kernel, dim3(blocks_for(n)), dim3(kLB), 0, s, src->d_src, S->vals[1], S->ring_start, n_rings, S->L);
    hipLaunchKernelGGL(bl_curvature_kernel, dim3(blocks_for(n)), dim3(kLB), 0, s, S->L, S->keys[1], S->ring_start, n_rings, S->curv);
    hipLaunchKernelGGL(bl_sector_kernel, dim3(6, n_rings), dim3(kLB), 0, s, S->L, S->curv, S->ring_start, (uint32_t)num_scan, S->edge_slot, S->surf_slot, S->edge_cnt,
                       S->surf_cnt, S->too_long);
    hipLaunchKernelGGL(bl_scan_offsets_kernel, dim3(n_scans), dim3(kLB), 0, s, S->edge_cnt, S->surf_cnt, S->too_long, (uint32_t)num_scan, S->edge_off, S->surf_off,
                       S->res);
    hipLaunchKernelGGL(bl_verdict_kernel, dim3(1), dim3(kLB), 0, s, S->res, n_scans, edge_max_n, surf_max_n);
    hipLaunchKernelGGL(bl_scatter_kernel, dim3(6, n_rings), dim3(kLB), 0, s, S->edge_slot, S->surf_slot, S->ring_start, S->edge_cnt, S->surf_cnt, S->edge_off,
                       S->surf_off, S->res, n_scans, (uint32_t)num_scan, edge_max_n, surf_max_n, edge->d_src, surf->d_src, edge->d_counts, surf->d_counts);
    LOCGPU_TRY(hipGetLastError());
    return hipMemcpyAsync(S->h_res, S->res, ((size_t)n_scans + 1) * sizeof(int4), hipMemcpyDeviceToHost, s);
}

int hip_fail(locgpu_ctx* ctx, hipError_t e, const char* what) {
    hip_ok(ctx, e, what);
    return e == hipErrorOutOfMemory ? LOCGPU_ERR_OOM : LOCGPU_ERR_NO_DEVICE;
}

}  // namespace

void batch_loam_free(locgpu_ctx* ctx) {
    delete ctx->bloam;
    ctx->bloam = nullptr;
}

}  // namespace locgpu

using namespace locgpu;

// The one body of locgpu_batch_loam_extract (host ring arrays) and locgpu_batch_loam_extract_resident (resident = true: the ring bytes
// that locgpu_batch_upload_ranges left in src).
static int batch_loam_extract(locgpu_batch* src, const uint8_t* const* rings, bool resident, int num_scan, locgpu_batch* edge, locgpu_batch* surf,
                              int32_t* out_edge_counts, int32_t* out_surf_counts, int32_t* out_status) {
    if (!src || !edge || !surf) {
        locgpu_batch* any = src ? src : (edge ? edge : surf);
        return fail(any ? any->ctx : nullptr, LOCGPU_ERR_INVALID, "batch_loam_extract: NULL batch");
    }
    locgpu_ctx* ctx = src->ctx;
    if (resident) {
        rings = nullptr;
        if (!src->rings_valid) return fail(ctx, LOCGPU_ERR_INVALID, "batch_loam_extract_resident: src holds no resident rings (they are left by locgpu_batch_upload_ranges and dropped by every later upload or preprocess into the batch)");
    } else if (!rings) return fail(ctx, LOCGPU_ERR_INVALID, "batch_loam_extract: rings is NULL");
    if (num_scan < 1 || num_scan > 256) return fail(ctx, LOCGPU_ERR_INVALID, "batch_loam_extract: num_scan must be in 1..256");
    if (src == edge || src == surf || edge == surf) return fail(ctx, LOCGPU_ERR_INVALID, "batch_loam_extract: src, edge and surf must be three distinct batches");
    if (edge->ctx != ctx || surf->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, "batch_loam_extract: the batches belong to different contexts");
    if (src->sharded || edge->sharded || surf->sharded) return fail(ctx, LOCGPU_ERR_INVALID, "batch_loam_extract: sharded batches are not supported");
    if (src->shared_src || edge->shared_src || surf->shared_src) return fail(ctx, LOCGPU_ERR_INVALID, "batch_loam_extract: shared-source batches are not supported");
    if (src->pending.active || edge->pending.active || surf->pending.active)
        return fail(ctx, LOCGPU_ERR_INVALID, "batch_loam_extract: an alignment of a batch has been begun and not finished");
    if (src->n_scans != edge->n_scans || src->n_scans != surf->n_scans) return fail(ctx, LOCGPU_ERR_INVALID, "batch_loam_extract: the batches hold different numbers of scans");
    const int n_scans = src->n_scans;
    if ((long long)n_scans * num_scan > kMaxRings)
        return fail(ctx, LOCGPU_ERR_INVALID, "batch_loam_extract: n_scans * num_scan = " + std::to_string((long long)n_scans * num_scan) + " exceeds the limit of 65535");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    int rc = order_behind_batch(ctx, src, "batch_loam_extract: ordering behind src");
    if (rc == LOCGPU_OK) rc = order_behind_batch(ctx, edge, "batch_loam_extract: ordering behind edge");
    if (rc == LOCGPU_OK) rc = order_behind_batch(ctx, surf, "batch_loam_extract: ordering behind surf");
    if (rc != LOCGPU_OK) return rc;
    for (int s = 0; s < n_scans; ++s)
        if (rings && src->counts[s] > 0 && !rings[s]) return fail(ctx, LOCGPU_ERR_INVALID, "batch_loam_extract: rings[" + std::to_string(s) + "] is NULL for a scan with points");
    if (n_scans == 0) return LOCGPU_OK;
    hipError_t e = extract_dev(ctx, src, rings, num_scan, edge, surf);
    // the one read-back: when it is there the whole pass has run, and whatever uses edge / surf next — on any stream — finds them complete
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return hip_fail(ctx, e, "batch_loam_extract"); }
    src->paced_tail = edge->paced_tail = surf->paced_tail = false;
    const int4* res = ctx->bloam->h_res;
    std::vector<int> ne(n_scans), ns(n_scans);
    int first_long = -1, first_big = -1;
    for (int s = 0; s < n_scans; ++s) {
        ne[s] = res[s].x;
        ns[s] = res[s].y;
        if (out_edge_counts) out_edge_counts[s] = res[s].x;
        if (out_surf_counts) out_surf_counts[s] = res[s].y;
        if (out_status) out_status[s] = res[s].z;
        if (res[s].z && first_long < 0) first_long = s;
        if ((res[s].x > edge->max_n || res[s].y > surf->max_n) && first_big < 0) first_big = s;
    }
    if (first_long >= 0)
        return fail(ctx, LOCGPU_ERR_INVALID, "batch_loam_extract: scan " + std::to_string(first_long) + " has a ring of more than 6 x 2048 points (edge and surf are unchanged)");
    if (first_big >= 0)
        return fail(ctx, LOCGPU_ERR_INVALID, "batch_loam_extract: scan " + std::to_string(first_big) + " yields " + std::to_string(ne[first_big]) + " edge and " +
                                                 std::to_string(ns[first_big]) + " surface points, edge / surf were created for " + std::to_string(edge->max_n) + " / " +
                                                 std::to_string(surf->max_n) + " per scan (both are unchanged)");
    set_host_counts(edge, ne.data());
    set_host_counts(surf, ns.data());
    edge->rings_valid = surf->rings_valid = edge->times_valid = surf->times_valid = false;  // features are written in picking order: whatever rings the destinations held are gone
    return LOCGPU_OK;
}

extern "C" {

int locgpu_batch_loam_extract(locgpu_batch* src, const uint8_t* const* rings, int num_scan, locgpu_batch* edge, locgpu_batch* surf, int32_t* out_edge_counts,
                              int32_t* out_surf_counts, int32_t* out_status) {
    return batch_loam_extract(src, rings, false, num_scan, edge, surf, out_edge_counts, out_surf_counts, out_status);
}

int locgpu_batch_loam_extract_resident(locgpu_batch* src, int num_scan, locgpu_batch* edge, locgpu_batch* surf, int32_t* out_edge_counts, int32_t* out_surf_counts,
                                       int32_t* out_status) {
    return batch_loam_extract(src, nullptr, true, num_scan, edge, surf, out_edge_counts, out_surf_counts, out_status);
}

}  // extern "C"
