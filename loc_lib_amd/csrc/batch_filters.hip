// loc_lib_amd/csrc/batch_filters.hip — the reference's front-end on every scan of a batch at once, and the two small calls that go
// with it (locgpu_batch_upload_clouds, locgpu_batch_download_scan).
//
// Every scan the reference matches goes through RemoveNanPoint → VoxelFilter::Filter → ScanMatch (loc.cpp:217-229, lio.cpp:236,257;
// voxel_filter.cpp:19-25 → pcl::VoxelGrid, point_cloud_utils.h:13-20 → pcl::removeNaNFromPointCloud). cloud_filters.hip does that for
// ONE resident cloud in 8 launches, a sort, a scan and a stream synchronisation — latency-bound at scan size. locgpu_batch_preprocess
// does it for all n_scans scans of a batch with one set of launches and one read-back of n_scans {count, status} pairs:
//
//   box      per (scan, block) partial bounding boxes of the finite points                 bp_box_kernel
//   set-up   one wave per scan: fold the boxes, PCL's overflow test, min_b / div_b         bp_setup_kernel   → VoxelParams[n_scans]
//   keys     64-bit key = scan << 32 | voxel index, value = slot of the point              bp_key_kernel
//   sort     ONE stable LSD radix sort of all slots on bits [0, 32 + ceil(log2 n_scans))   rocPRIM
//   heads    first point of every voxel run (every point, in a pass-through scan)          bp_head_kernel, exclusive sum → ranks
//   starts   start[rank] of every run; per scan: first rank, end rank, end of valid points bp_starts_kernel
//   counts   per scan {count, status}, largest count                                       bp_finalize_kernel
//   out      one thread per output point: float32 sums in sorted (= input) order, one division; a pass-through scan's points are
//            copied bit for bit                                                            bp_centroid_kernel (+ bp_copy_back_kernel in place)
//
// What comes out is, per scan, locgpu_cloud_voxel_filter(locgpu_cloud_remove_nan(scan), leaf): the same kernels' arithmetic on the
// same operands in the same order (the sort is stable, and a scan's points keep their relative order whatever else is in the batch),
// so the same bytes, for every n_scans. No floating-point atomics, no atomics at all.
//
// A slot that holds no finite point (padding behind a scan's count, NaN / inf points) gets the voxel index 0xFFFFFFFF of its own scan:
// it sorts behind the scan's voxels and is never a head. (A VALID index of that value would need 2^32 − 1 cells in a grid that passed
// PCL's 2^31 overflow test — div_b can exceed the tested extent by one per axis — i.e. a scan some 2^30 leaves long and two wide;
// such a point would be dropped here and kept by the single-cloud filter.)
//
// The pass works on the batch's padded layout [n_scans][max_n]: every slot is keyed and sorted, whatever the scans' counts. A batch
// of real scans is nearly full; a very ragged one pays for its padding.
//
// Scratch, grow-only on the context (freed by filters_free): per SLOT (= per input point of a full batch)
//   keys 2 × 8 B, values 2 × 4 B, heads 4 B, ranks 4 B = 32 B, + rocPRIM's sort workspace (≈ 12 B: its own ping-pong of the pairs),
//   + 16 B of staging when dst == src; per scan 6 × 4 B × 64 partial boxes, a VoxelParams, 16 B of segment marks, 8 B of result.
// Algorithmic bytes per slot: 16 (box) + 16 + 12 (keys) + 24 · passes (sort: 12 in, 12 out) + 16 + 4 (heads) + 8 (scan) + 28 (starts)
//   + 4 + 16 (gather) + 16 per output point = 120 + 24 · passes; 5 passes for 256 scans: 240 B.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "batch_upload.hpp"
#include "cloud_filters.hpp"
#include "context.hpp"
#include "device_prims.hpp"

namespace locgpu {

namespace {

constexpr int kBF = 256;                      // threads per block of every kernel here (but the set-up wave)
constexpr int kBoxItems = 4;                  // independent 16-byte loads in flight per thread of the box pass
constexpr int kBoxTile = kBF * kBoxItems;     // points a box block takes per trip
constexpr int kBoxBlocksMax = 64;             // partial boxes per scan: one per lane of the set-up wave
constexpr uint32_t kNoVoxel = 0xFFFFFFFFu;    // voxel index of a slot without a finite point

struct ScanSeg {          // per scan, written by the starts kernel (zeroed by the set-up kernel)
    uint32_t first_rank;  // rank of the scan's first run
    uint32_t end_rank;    // one past the rank of its last run
    uint32_t seg_end;     // one past the sorted position of its last valid point
    uint32_t pad;
};

struct TableEntry { const float4* p; uint32_t n; uint32_t pad; };  // locgpu_batch_upload_clouds: one resident cloud

__device__ __forceinline__ bool finite3(const float4& p) { return isfinite(p.x) && isfinite(p.y) && isfinite(p.z); }

// getMinMax3D per scan: block (x, s) folds the finite points x·kBF + t, + gridDim.x·kBF, … of scan s into one partial box.
__global__ __launch_bounds__(kBF) void bp_box_kernel(const float4* __restrict__ src, const int* __restrict__ counts, uint32_t max_n, float* __restrict__ partial) {
    const uint32_t s = blockIdx.y;
    const uint32_t n = (uint32_t)counts[s];
    const float4* __restrict__ pts = src + (size_t)s * max_n;
    float mn[3] = {FLT_MAX, FLT_MAX, FLT_MAX}, mx[3] = {-FLT_MAX, -FLT_MAX, -FLT_MAX};
    const uint32_t stride = gridDim.x * kBF;
    uint32_t i = blockIdx.x * kBF + threadIdx.x;
    auto take = [&](const float4& p) {
        if (!finite3(p)) return;
        const float c[3] = {p.x, p.y, p.z};
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            mn[a] = c[a] < mn[a] ? c[a] : mn[a];
            mx[a] = c[a] > mx[a] ? c[a] : mx[a];
        }
    };
    for (; (unsigned long long)i + 3ull * stride < n; i += 4 * stride) {
        const float4 p0 = pts[i], p1 = pts[i + stride], p2 = pts[i + 2 * stride], p3 = pts[i + 3 * stride];
        take(p0); take(p1); take(p2); take(p3);
    }
    for (; i < n; i += stride) take(pts[i]);
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int off = 32; off > 0; off >>= 1) {
            const float o1 = __shfl_xor(mn[a], off, 64), o2 = __shfl_xor(mx[a], off, 64);
            mn[a] = o1 < mn[a] ? o1 : mn[a];
            mx[a] = o2 > mx[a] ? o2 : mx[a];
        }
    }
    __shared__ float s_box[kBF / 64][6];
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int a = 0; a < 3; ++a) { s_box[wave][a] = mn[a]; s_box[wave][3 + a] = mx[a]; }
    }
    __syncthreads();
    if (threadIdx.x < 6) {
        float v = s_box[0][threadIdx.x];
        for (int w = 1; w < kBF / 64; ++w) {
            const float o = s_box[w][threadIdx.x];
            v = threadIdx.x < 3 ? (o < v ? o : v) : (o > v ? o : v);
        }
        partial[((size_t)s * gridDim.x + blockIdx.x) * 6 + threadIdx.x] = v;
    }
}

// VoxelGrid::applyFilter's set-up for scan blockIdx.x, in the arithmetic of voxel_setup_kernel (cloud_filters.hip): one wave folds the
// scan's partial boxes (n_partial <= 64: one per lane), lane 0 does the scalar part.
__global__ __launch_bounds__(64) void bp_setup_kernel(VoxelParams* __restrict__ params, ScanSeg* __restrict__ seg, const float* __restrict__ partial, int n_partial,
                                                      float inv_leaf) {
    const uint32_t s = blockIdx.x;
    float box[6] = {FLT_MAX, FLT_MAX, FLT_MAX, -FLT_MAX, -FLT_MAX, -FLT_MAX};
    for (int b = threadIdx.x; b < n_partial; b += 64) {
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            const float lo = partial[((size_t)s * n_partial + b) * 6 + a], hi = partial[((size_t)s * n_partial + b) * 6 + 3 + a];
            box[a] = lo < box[a] ? lo : box[a];
            box[3 + a] = hi > box[3 + a] ? hi : box[3 + a];
        }
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        for (int off = 32; off > 0; off >>= 1) {
            const float o1 = __shfl_xor(box[a], off, 64), o2 = __shfl_xor(box[3 + a], off, 64);
            box[a] = o1 < box[a] ? o1 : box[a];
            box[3 + a] = o2 > box[3 + a] ? o2 : box[3 + a];
        }
    }
    if (threadIdx.x != 0) return;
    seg[s] = ScanSeg{0u, 0u, 0u, 0u};
    VoxelParams* P = params + s;
    const float inv = inv_leaf;
    const float* mn = box;
    const float* mx = box + 3;
    P->inv_leaf = inv;
    P->n_out = 0;
    P->status = 0;
    P->invalid_key = kNoVoxel;
    for (int a = 0; a < 3; ++a) { P->min_b[a] = 0; P->div_b[a] = 0; P->mul[a] = 0; }
    if (mn[0] > mx[0]) { P->status = 2; return; }  // no finite point at all
    const long long dx = (long long)((mx[0] - mn[0]) * inv) + 1, dy = (long long)((mx[1] - mn[1]) * inv) + 1, dz = (long long)((mx[2] - mn[2]) * inv) + 1;
    if ((double)dx * (double)dy * (double)dz > 2147483647.0) { P->status = 1; return; }  // "Leaf size is too small…": output = the finite points
    for (int a = 0; a < 3; ++a) {
        P->min_b[a] = (int)floorf(mn[a] * inv);
        P->div_b[a] = (int)floorf(mx[a] * inv) - P->min_b[a] + 1;
    }
    P->mul[0] = 1;
    P->mul[1] = P->div_b[0];
    P->mul[2] = P->div_b[0] * P->div_b[1];
}

// Slot i of scan s (blockIdx.y): key = s << 32 | voxel index, value = the slot. A pass-through scan's finite points all get index 0:
// the stable sort then leaves them in input order.
__global__ __launch_bounds__(kBF) void bp_key_kernel(const float4* __restrict__ src, const int* __restrict__ counts, uint32_t max_n,
                                                     const VoxelParams* __restrict__ params, unsigned long long* __restrict__ keys, uint32_t* __restrict__ vals) {
    const uint32_t s = blockIdx.y;
    const uint32_t i = blockIdx.x * kBF + threadIdx.x;
    if (i >= max_n) return;
    const size_t slot = (size_t)s * max_n + i;
    uint32_t idx = kNoVoxel;
    if (i < (uint32_t)counts[s]) {
        const float4 p = src[slot];
        const VoxelParams* P = params + s;
        if (finite3(p) && P->status != 2) {
            if (P->status == 1) {
                idx = 0u;
            } else {
                const float inv = P->inv_leaf;
                const int ijk0 = (int)(floorf(p.x * inv) - (float)P->min_b[0]);
                const int ijk1 = (int)(floorf(p.y * inv) - (float)P->min_b[1]);
                const int ijk2 = (int)(floorf(p.z * inv) - (float)P->min_b[2]);
                idx = (uint32_t)(ijk0 * P->mul[0] + ijk1 * P->mul[1] + ijk2 * P->mul[2]);
            }
        }
    }
    keys[slot] = ((unsigned long long)s << 32) | idx;
    vals[slot] = (uint32_t)slot;
}

__global__ __launch_bounds__(kBF) void bp_head_kernel(const unsigned long long* __restrict__ keys, size_t n, const VoxelParams* __restrict__ params,
                                                      uint32_t* __restrict__ head) {
    const size_t j = (size_t)blockIdx.x * kBF + threadIdx.x;
    if (j >= n) return;
    const unsigned long long k = keys[j];
    const bool valid = (uint32_t)k != kNoVoxel;
    const bool passthrough = valid && params[k >> 32].status == 1;  // every point is its own run
    head[j] = (valid && (passthrough || j == 0 || keys[j - 1] != k)) ? 1u : 0u;
}

// start[r] = sorted position of run r's first point (runs are numbered through the whole batch); per scan, the marks that give its
// output offset and count. A scan's valid points are contiguous in sorted order, its first valid point is a head.
__global__ __launch_bounds__(kBF) void bp_starts_kernel(const unsigned long long* __restrict__ keys, const uint32_t* __restrict__ head,
                                                        const uint32_t* __restrict__ rank, size_t n, uint32_t* __restrict__ start, ScanSeg* __restrict__ seg) {
    const size_t j = (size_t)blockIdx.x * kBF + threadIdx.x;
    if (j >= n) return;
    const unsigned long long k = keys[j];
    if ((uint32_t)k == kNoVoxel) return;
    const uint32_t s = (uint32_t)(k >> 32);
    const uint32_t h = head[j], r = rank[j];
    if (h) start[r] = (uint32_t)j;
    if (j == 0 || (uint32_t)(keys[j - 1] >> 32) != s) seg[s].first_rank = r;
    bool last = j + 1 == n;
    if (!last) {
        const unsigned long long kn = keys[j + 1];
        last = (uint32_t)kn == kNoVoxel || (uint32_t)(kn >> 32) != s;
    }
    if (last) {
        seg[s].end_rank = r + h;
        seg[s].seg_end = (uint32_t)(j + 1);
    }
}

// One block: res[s] = {count, status}, res[n_scans] = {largest count, 0}.
__global__ __launch_bounds__(kBF) void bp_finalize_kernel(const VoxelParams* __restrict__ params, const ScanSeg* __restrict__ seg, int n_scans, int2* __restrict__ res) {
    int mx = 0;
    for (int s = threadIdx.x; s < n_scans; s += kBF) {
        const int status = params[s].status;
        const int count = status == 2 ? 0 : (int)(seg[s].end_rank - seg[s].first_rank);
        res[s] = int2{count, status};
        mx = count > mx ? count : mx;
    }
    for (int off = 32; off > 0; off >>= 1) {
        const int o = __shfl_xor(mx, off, 64);
        mx = o > mx ? o : mx;
    }
    __shared__ int s_mx[kBF / 64];
    if ((threadIdx.x & 63) == 0) s_mx[threadIdx.x >> 6] = mx;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kBF / 64; ++w) mx = s_mx[w] > mx ? s_mx[w] : mx;
        res[n_scans] = int2{mx, 0};
    }
}

// Output point v of scan s (blockIdx.y): CentroidPoint's float32 running sums over the run in sorted (= input) order and one division
// each, as voxel_centroid_kernel (cloud_filters.hip) — the gathers of a run do not depend on the sums and go four at a time — or, in a
// pass-through scan, the point itself. Nothing is written when a scan does not fit `out` (dst_max_n): the call fails and leaves dst
// alone. `counts_out`: dst's device counts, or nullptr when the copy-back kernel writes them (in place).
__global__ __launch_bounds__(kBF) void bp_centroid_kernel(const float4* __restrict__ src, const uint32_t* __restrict__ vals, const uint32_t* __restrict__ start,
                                                          const ScanSeg* __restrict__ seg, const int2* __restrict__ res, int n_scans, uint32_t dst_max_n,
                                                          float4* __restrict__ out, int* __restrict__ counts_out) {
    if ((uint32_t)res[n_scans].x > dst_max_n) return;
    const uint32_t s = blockIdx.y;
    const uint32_t v = blockIdx.x * kBF + threadIdx.x;
    const int2 cs = res[s];
    if (v == 0 && counts_out) counts_out[s] = cs.x;
    if (v >= (uint32_t)cs.x) return;
    const ScanSeg sg = seg[s];
    const uint32_t g = sg.first_rank + v;
    const uint32_t b = start[g], e = v + 1 < (uint32_t)cs.x ? start[g + 1] : sg.seg_end;
    float4 o;
    if (cs.y == 1) {
        const float4 p = src[vals[b]];
        o = float4{p.x, p.y, p.z, 0.f};  // no "0.f +": a negative zero stays one
    } else {
        float sx = 0.f, sy = 0.f, sz = 0.f;
        uint32_t j = b;
        for (; j + 4 <= e; j += 4) {
            const uint32_t i0 = vals[j], i1 = vals[j + 1], i2 = vals[j + 2], i3 = vals[j + 3];
            const float4 p0 = src[i0], p1 = src[i1], p2 = src[i2], p3 = src[i3];
            sx += p0.x; sy += p0.y; sz += p0.z;
            sx += p1.x; sy += p1.y; sz += p1.z;
            sx += p2.x; sy += p2.y; sz += p2.z;
            sx += p3.x; sy += p3.y; sz += p3.z;
        }
        for (; j < e; ++j) {
            const float4 p = src[vals[j]];
            sx += p.x; sy += p.y; sz += p.z;
        }
        const float cnt = (float)(e - b);
        o = float4{sx / cnt, sy / cnt, sz / cnt, 0.f};
    }
    out[(size_t)s * dst_max_n + v] = o;
}

// In place: the centroids were produced in staging (the gathers read the batch's own points); now they go home, with the counts.
__global__ __launch_bounds__(kBF) void bp_copy_back_kernel(const float4* __restrict__ stage, const int2* __restrict__ res, uint32_t max_n, float4* __restrict__ dst,
                                                           int* __restrict__ counts_out) {
    const uint32_t s = blockIdx.y;
    const uint32_t v = blockIdx.x * kBF + threadIdx.x;
    const int count = res[s].x;
    if (v == 0) counts_out[s] = count;
    if (v >= (uint32_t)count) return;
    const size_t slot = (size_t)s * max_n + v;
    dst[slot] = stage[slot];
}

// locgpu_batch_upload_clouds: scan s (blockIdx.y) = {x, y, z, 0} of the points of table entry s.
__global__ __launch_bounds__(kBF) void bp_gather_clouds_kernel(const TableEntry* __restrict__ table, uint32_t max_n, float4* __restrict__ dst, int* __restrict__ counts) {
    const uint32_t s = blockIdx.y;
    const TableEntry t = table[s];
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[s] = (int)t.n;
    float4* __restrict__ out = dst + (size_t)s * max_n;
    const uint32_t stride = gridDim.x * kBF;
    uint32_t i = blockIdx.x * kBF + threadIdx.x;
    for (; (unsigned long long)i + 3ull * stride < t.n; i += 4 * stride) {
        const float4 p0 = t.p[i], p1 = t.p[i + stride], p2 = t.p[i + 2 * stride], p3 = t.p[i + 3 * stride];
        out[i] = float4{p0.x, p0.y, p0.z, 0.f};
        out[i + stride] = float4{p1.x, p1.y, p1.z, 0.f};
        out[i + 2 * stride] = float4{p2.x, p2.y, p2.z, 0.f};
        out[i + 3 * stride] = float4{p3.x, p3.y, p3.z, 0.f};
    }
    for (; i < t.n; i += stride) {
        const float4 p = t.p[i];
        out[i] = float4{p.x, p.y, p.z, 0.f};
    }
}

}  // namespace

// Two groups that grow together: per slot {keys, vals, head, rank} and per scan {params … h_table}. The buffer grown last (rank,
// h_table) has the capacity of its whole group.
struct BatchFilterScratch {
    DevBuf<unsigned long long> keys[2];
    DevBuf<uint32_t> vals[2], head, rank;
    DevBuf<unsigned char> temp;
    DevBuf<float4> stage;  // in place only
    DevBuf<VoxelParams> params;
    DevBuf<ScanSeg> seg;
    DevBuf<float> partial;
    DevBuf<int2> res;      // [scans + 1]
    PinnedBuf<int2> h_res;
    DevBuf<TableEntry> table;
    PinnedBuf<TableEntry> h_table;
};

namespace {

BatchFilterScratch* scratch(locgpu_ctx* ctx) {
    if (!ctx->bfilt) ctx->bfilt = new BatchFilterScratch();
    return ctx->bfilt;
}

hipError_t ensure_scans(locgpu_ctx* ctx, int n_scans) {
    BatchFilterScratch* S = scratch(ctx);
    if ((size_t)n_scans <= S->h_table.cap()) return hipSuccess;
    const size_t cap = (size_t)n_scans + 16;
    LOCGPU_TRY(S->params.alloc(cap));
    LOCGPU_TRY(S->seg.alloc(cap));
    LOCGPU_TRY(S->partial.alloc(cap * kBoxBlocksMax * 6));
    LOCGPU_TRY(S->res.alloc(cap + 1));
    LOCGPU_TRY(S->table.alloc(cap));
    LOCGPU_TRY(S->h_res.alloc(cap + 1));
    return S->h_table.alloc(cap);
}

hipError_t ensure_slots(locgpu_ctx* ctx, size_t n, unsigned end_bit, bool in_place) {
    BatchFilterScratch* S = scratch(ctx);
    if (n > S->rank.cap()) {
        const size_t cap = with_headroom(n);
        for (int j = 0; j < 2; ++j) {
            LOCGPU_TRY(S->keys[j].alloc(cap));
            LOCGPU_TRY(S->vals[j].alloc(cap));
        }
        LOCGPU_TRY(S->head.alloc(cap));
        LOCGPU_TRY(S->rank.alloc(cap));
    }
    size_t b1 = 0, b2 = 0;
    LOCGPU_TRY(prim::sort_pairs((void*)nullptr, b1, S->keys[0].get(), S->keys[1].get(), S->vals[0].get(), S->vals[1].get(), n, 0, end_bit, ctx->stream));
    LOCGPU_TRY(prim::exclusive_sum((void*)nullptr, b2, S->head.get(), S->rank.get(), n, ctx->stream));
    const size_t need = std::max(b1, b2) + 256;
    if (need > S->temp.cap()) LOCGPU_TRY(S->temp.alloc(need + need / 4));
    if (in_place && n > S->stage.cap()) LOCGPU_TRY(S->stage.alloc(with_headroom(n)));
    return hipSuccess;
}

inline unsigned blocks_for(size_t n) { return (unsigned)((n + kBF - 1) / kBF); }

// The launches of one pass; the result pairs are on their way to S->h_res when it returns.
hipError_t preprocess_dev(locgpu_ctx* ctx, locgpu_batch* src, float leaf, locgpu_batch* dst) {
    BatchFilterScratch* S = scratch(ctx);
    hipStream_t s = ctx->stream;
    const int n_scans = src->n_scans;
    const uint32_t max_n = (uint32_t)src->max_n, dst_max_n = (uint32_t)dst->max_n;
    const size_t n = src->pitch;
    const bool in_place = src == dst;
    unsigned scan_bits = 0;
    while ((1u << scan_bits) < (unsigned)n_scans) ++scan_bits;
    const unsigned end_bit = 32 + scan_bits;
    LOCGPU_TRY(ensure_scans(ctx, n_scans));
    LOCGPU_TRY(ensure_slots(ctx, n, end_bit, in_place));
    const float inv = 1.0f / leaf;  // inverse_leaf_size_
    const int n_partial = (int)std::min<size_t>(((size_t)max_n + kBoxTile - 1) / kBoxTile, (size_t)kBoxBlocksMax);
    hipLaunchKernelGGL(bp_box_kernel, dim3(n_partial, n_scans), dim3(kBF), 0, s, src->d_src, src->d_counts, max_n, S->partial);
    hipLaunchKernelGGL(bp_setup_kernel, dim3(n_scans), dim3(64), 0, s, S->params, S->seg, S->partial, n_partial, inv);
    hipLaunchKernelGGL(bp_key_kernel, dim3(blocks_for(max_n), n_scans), dim3(kBF), 0, s, src->d_src, src->d_counts, max_n, S->params, S->keys[0], S->vals[0]);
    LOCGPU_TRY(hipGetLastError());
    size_t tb = S->temp.cap();
    LOCGPU_TRY(prim::sort_pairs(S->temp, tb, S->keys[0].get(), S->keys[1].get(), S->vals[0].get(), S->vals[1].get(), n, 0, end_bit, s));
    hipLaunchKernelGGL(bp_head_kernel, dim3(blocks_for(n)), dim3(kBF), 0, s, S->keys[1], n, S->params, S->head);
    tb = S->temp.cap();
    LOCGPU_TRY(prim::exclusive_sum(S->temp, tb, S->head.get(), S->rank.get(), n, s));
    uint32_t* start = S->vals[0].get();  // free again after the sort; a rank is below n
    hipLaunchKernelGGL(bp_starts_kernel, dim3(blocks_for(n)), dim3(kBF), 0, s, S->keys[1], S->head, S->rank, n, start, S->seg);
    hipLaunchKernelGGL(bp_finalize_kernel, dim3(1), dim3(kBF), 0, s, S->params, S->seg, n_scans, S->res);
    const uint32_t out_rows = std::min(max_n, dst_max_n);  // no scan has more output points than input points, and none may have more than dst holds
    hipLaunchKernelGGL(bp_centroid_kernel, dim3(blocks_for(out_rows), n_scans), dim3(kBF), 0, s, src->d_src, S->vals[1], start, S->seg, S->res, n_scans, dst_max_n,
                       in_place ? S->stage.get() : dst->d_src.get(), in_place ? (int*)nullptr : dst->d_counts.get());
    if (in_place) hipLaunchKernelGGL(bp_copy_back_kernel, dim3(blocks_for(out_rows), n_scans), dim3(kBF), 0, s, S->stage, S->res, max_n, dst->d_src, dst->d_counts);
    LOCGPU_TRY(hipGetLastError());
    return hipMemcpyAsync(S->h_res, S->res, ((size_t)n_scans + 1) * sizeof(int2), hipMemcpyDeviceToHost, s);
}

int hip_fail(locgpu_ctx* ctx, hipError_t e, const char* what) {
    hip_ok(ctx, e, what);
    return e == hipErrorOutOfMemory ? LOCGPU_ERR_OOM : LOCGPU_ERR_NO_DEVICE;
}

}  // namespace

// The context's stream behind everything that may still touch `b`'s points: its pending upload (the host side is waited for) and the
// idle launches a paced one-scan alignment may have left queued.
int order_behind_batch(locgpu_ctx* ctx, locgpu_batch* b, const char* who) {
    const int rc = upload_join_batch(b);
    if (rc != LOCGPU_OK) return rc;
    if (!hip_ok(ctx, upload_order_after(b, ctx->stream), who)) return LOCGPU_ERR_NO_DEVICE;
    if (b->paced_tail && b->stream != ctx->stream) {
        if (!hip_ok(ctx, b->tail_ev.ensure(), who)) return LOCGPU_ERR_NO_DEVICE;
        if (!hip_ok(ctx, hipEventRecord(b->tail_ev, b->stream), who) || !hip_ok(ctx, hipStreamWaitEvent(ctx->stream, b->tail_ev, 0), who)) return LOCGPU_ERR_NO_DEVICE;
    }
    return LOCGPU_OK;
}

// The batch's three copies of its counts agree again (d_counts was written on the device).
void set_host_counts(locgpu_batch* b, const int* counts) {
    for (int s = 0; s < b->n_scans; ++s) {
        b->counts[s] = counts[s];
        if (b->upl.h_counts) b->upl.h_counts[s] = counts[s];
    }
}

void batch_filters_free(locgpu_ctx* ctx) {
    delete ctx->bfilt;
    ctx->bfilt = nullptr;
}

}  // namespace locgpu

using namespace locgpu;

extern "C" {

int locgpu_batch_preprocess(locgpu_batch* src, float leaf, locgpu_batch* dst, int32_t* out_counts, int32_t* out_status) {
    if (!src || !dst) return fail(src ? src->ctx : (dst ? dst->ctx : nullptr), LOCGPU_ERR_INVALID, "batch_preprocess: NULL batch");
    locgpu_ctx* ctx = src->ctx;
    if (dst->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, "batch_preprocess: the batches belong to different contexts");
    if (src->sharded || dst->sharded) return fail(ctx, LOCGPU_ERR_INVALID, "batch_preprocess: sharded batches are not supported");
    if (src->shared_src || dst->shared_src) return fail(ctx, LOCGPU_ERR_INVALID, "batch_preprocess: shared-source batches are not supported");
    if (src->pending.active || dst->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "batch_preprocess: an alignment of the batch has been begun and not finished");
    if (src->n_scans != dst->n_scans) return fail(ctx, LOCGPU_ERR_INVALID, "batch_preprocess: src and dst hold different numbers of scans");
    if (!(leaf > 0.f) || !std::isfinite(leaf)) return fail(ctx, LOCGPU_ERR_INVALID, "batch_preprocess: leaf size must be positive");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    int rc = order_behind_batch(ctx, src, "batch_preprocess: ordering behind src");
    if (rc == LOCGPU_OK && dst != src) rc = order_behind_batch(ctx, dst, "batch_preprocess: ordering behind dst");
    if (rc != LOCGPU_OK) return rc;
    hipError_t e = preprocess_dev(ctx, src, leaf, dst);
    // the one read-back: when it is there the whole pass has run, and whatever uses dst next — on any stream — finds it complete
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return hip_fail(ctx, e, "batch_preprocess"); }
    src->paced_tail = dst->paced_tail = false;
    const int n_scans = src->n_scans;
    const int2* res = ctx->bfilt->h_res;
    std::vector<int> counts(n_scans);
    for (int s = 0; s < n_scans; ++s) {
        counts[s] = res[s].x;
        if (out_counts) out_counts[s] = res[s].x;
        if (out_status) out_status[s] = res[s].y;
    }
    if (res[n_scans].x > dst->max_n)
        return fail(ctx, LOCGPU_ERR_INVALID, "batch_preprocess: a filtered scan has " + std::to_string(res[n_scans].x) + " points, dst was created for " +
                                                 std::to_string(dst->max_n) + " per scan (dst is unchanged)");
    set_host_counts(dst, counts.data());
    dst->rings_valid = dst->times_valid = false;  // centroids have no ring and no time (locgpu_batch_upload_ranges' ring bytes, range_ingest.hip)
    return LOCGPU_OK;
}

int locgpu_batch_upload_clouds(locgpu_batch* b, const locgpu_cloud* const* clouds, int n) {
    if (!b) return LOCGPU_ERR_INVALID;
    locgpu_ctx* ctx = b->ctx;
    if (b->shared_src) return fail(ctx, LOCGPU_ERR_INVALID, "batch upload: a shared-source batch takes its cloud when it is created");
    if (!clouds || n != b->n_scans) return fail(ctx, LOCGPU_ERR_INVALID, "batch_upload_clouds: bad arguments (one cloud per scan of the batch)");
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "batch upload: an alignment of this batch has been begun and not finished");
    size_t longest = 0;
    for (int s = 0; s < n; ++s) {
        if (!clouds[s] || !clouds[s]->ctx) return fail(ctx, LOCGPU_ERR_INVALID, "batch_upload_clouds: NULL cloud");
        if (clouds[s]->n > (size_t)b->max_n) return fail(ctx, LOCGPU_ERR_INVALID, "batch upload: a scan has more points than the batch was created for");
        if (clouds[s]->ctx->device != ctx->device) return fail(ctx, LOCGPU_ERR_INVALID, "batch_upload_clouds: a cloud belongs to a context on another GPU");
        longest = std::max(longest, clouds[s]->n);
    }
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = order_behind_batch(ctx, b, "batch_upload_clouds: ordering behind the batch");
    if (rc != LOCGPU_OK) return rc;
    hipError_t e = ensure_scans(ctx, n);
    if (e != hipSuccess) return hip_fail(ctx, e, "batch_upload_clouds: scratch");
    BatchFilterScratch* S = ctx->bfilt;
    std::vector<int> counts(n);
    for (int s = 0; s < n; ++s) {
        e = cloud_input_ready(ctx, clouds[s]);
        if (e != hipSuccess) return hip_fail(ctx, e, "batch_upload_clouds: ordering behind the cloud's context");
        S->h_table[s] = TableEntry{clouds[s]->d.get(), (uint32_t)clouds[s]->n, 0u};
        counts[s] = (int)clouds[s]->n;
    }
    hipStream_t st = ctx->stream;
    e = hipMemcpyAsync(S->table, S->h_table, (size_t)n * sizeof(TableEntry), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        const unsigned bx = (unsigned)std::min<size_t>(std::max<size_t>((longest + kBoxTile - 1) / kBoxTile, 1), 64);
        hipLaunchKernelGGL(bp_gather_clouds_kernel, dim3(bx, n), dim3(kBF), 0, st, S->table, (uint32_t)b->max_n, b->d_src, b->d_counts);
        e = hipGetLastError();
    }
    // blocking, like every consumer of a foreign cloud (cloud_input_ready): the clouds may be written again when the call returns
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) { (void)hipStreamSynchronize(st); return hip_fail(ctx, e, "batch_upload_clouds"); }
    b->paced_tail = false;
    b->rings_valid = b->times_valid = false;
    set_host_counts(b, counts.data());
    return LOCGPU_OK;
}

int locgpu_batch_download_scan(locgpu_batch* b, int scan, void* out, size_t capacity, size_t stride_bytes, size_t* n) {
    if (!b) return LOCGPU_ERR_INVALID;
    locgpu_ctx* ctx = b->ctx;
    if (b->shared_src) return fail(ctx, LOCGPU_ERR_INVALID, "batch_download_scan: a shared-source batch holds one cloud, not scans");
    if (scan < 0 || scan >= b->n_scans) return fail(ctx, LOCGPU_ERR_INVALID, "batch_download_scan: scan index out of range");
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "batch_download_scan: an alignment of this batch has been begun and not finished");
    const size_t cnt = (size_t)b->counts[scan];
    if (n) *n = cnt;
    if (!out) return LOCGPU_OK;
    if (stride_bytes < 12) return fail(ctx, LOCGPU_ERR_INVALID, "batch_download_scan: stride < 12");
    if (cnt > capacity) return fail(ctx, LOCGPU_ERR_INVALID, "batch_download_scan: capacity < the scan's size");
    if (cnt == 0) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = order_behind_batch(ctx, b, "batch_download_scan: ordering behind the batch");
    if (rc != LOCGPU_OK) return rc;
    float4* stage = nullptr;
    hipError_t e = cloud_stage(ctx, cnt, &stage);
    if (e != hipSuccess) return hip_fail(ctx, e, "batch_download_scan: hipHostMalloc");
    e = hipMemcpyAsync(stage, b->d_src + (size_t)scan * b->max_n, cnt * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "batch_download_scan: D2H");
    char* base = (char*)out;
    const size_t row = stride_bytes >= sizeof(float4) ? sizeof(float4) : 12;  // with room for it, the fourth lane too
    for (size_t i = 0; i < cnt; ++i) std::memcpy(base + i * stride_bytes, &stage[i], row);
    return LOCGPU_OK;
}

}  // extern "C"
