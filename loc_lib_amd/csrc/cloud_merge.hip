// loc_lib_amd/csrc/cloud_merge.hip — the global map of a mapping run on the device (include/locgpu.h, "The global map …"):
// locgpu_clouds_merge, locgpu_batch_merge, locgpu_batch_export_cloud.
//
// Lio::GetGlobalMap (lio.cpp:550-580; the LOAM pair :582-614), called by SaveGlobalMap (:131-207), takes every keyframe through
// pcl::transformPointCloud(kf, kf, estimated_poses_[i].matrix()) (:571, the DOUBLE 4×4), `*global_map += *kf`, and ONE
// VoxelFilter::Filter (voxel_filter.cpp:19-25). Through the single-cloud entry points that is a transform launch, a device-to-device
// copy and a temporary cloud PER KEYFRAME before the one filter; a mapping session has thousands of keyframes. Here the transform and
// the join are ONE launch whatever the number of clouds, and the filter is the existing one (voxel_filter_dev):
//
//   table   n entries {source pointer, first output index, count, flags, 3×4 doubles} and the n first indices once more as a dense
//           array (what the kernel searches), built on the host — clouds and batches keep their counts there — and sent in one copy
//   merge   one thread per OUTPUT point: a block finds the entry of its first point by an upper bound over the first indices, its
//           threads walk forward from there; one 16-byte load, transform_point_f64 (cloud_filters.hpp: the arithmetic of
//           locgpu_cloud_transform, bit for bit), one 16-byte store                                                     merge_kernel
//   filter  voxel_filter_dev on the joined cloud, into `out`
//
// Empty clouds give runs of EQUAL first indices; "the last entry whose first index is <= i" is then the one that holds point i (the
// entries before it in the run are empty), and that is what both the upper bound and the walk find. No atomics, nothing per cloud.
// Bytes: 16 in + 16 out per point, + 124 per entry.
//
// The joined cloud lives in a cloud the context keeps (MergeScratch::joined, grow-only) and `out` is only written by the last step —
// the filter's swap, or a swap with the joined cloud when leaf == 0 — so every refusal leaves `out` as it was.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "cloud_filters.hpp"
#include "context.hpp"

namespace locgpu {

namespace {

constexpr int kMB = 256;                    // threads per block = output points per block
constexpr size_t kMaxPoints = 0x7FFFFF00u;  // a cloud's limit (locgpu_cloud_upload, locgpu_cloud_append)

constexpr uint32_t kDense = 1u;      // the source is flagged dense: every point is transformed, finite or not
constexpr uint32_t kTransform = 2u;  // m is applied (poses != NULL); otherwise the bits are carried through
constexpr uint32_t kZeroW = 4u;      // the source is a batch's scan: the fourth lane comes out +0

struct MergeEntry {
    const float4* p;
    uint32_t first;  // index of the source's first point in the joined cloud: the exclusive sum of the counts
    uint32_t n;
    uint32_t flags;
    uint32_t pad;
    double m[12];    // row-major 3×4 (M34)
};

__device__ __forceinline__ float4 merged_point(const MergeEntry* __restrict__ t, uint32_t i) {
    const uint32_t flags = t->flags;
    float4 p = t->p[i - t->first];
    if (flags & kTransform) p = transform_point_f64(p, t->m, (flags & kDense) != 0);
    if (flags & kZeroW) p.w = 0.f;
    return p;
}

// Point i of the joined cloud. `first[e]` = table[e].first, dense (the search reads nothing else); first[0] = 0 and i < total, so the
// upper bound is at least 1 and the walk stops at an entry with n > 0. The search is a chain of dependent loads in front of the one
// load and store a block is there for, so it starts at the entry a table of equal clouds would have the block in (guess_scale =
// n_entries / total: keyframes are about one size, the guess is then right or next to it), widens by doubling steps until the upper
// bound is bracketed, and bisects what is left: two or three loads instead of log2(n_entries), and never more than twice that.
__global__ __launch_bounds__(kMB) void merge_kernel(const MergeEntry* __restrict__ table, const uint32_t* __restrict__ first, uint32_t n_entries, uint32_t total,
                                                    float guess_scale, float4* __restrict__ out) {
    const uint32_t b0 = blockIdx.x * kMB;  // block-uniform: the search below runs on the scalar unit
    uint32_t lo = 0, hi = n_entries;       // first[j] <= b0 for every j < lo, first[j] > b0 for every j >= hi
    const uint32_t g = min(n_entries - 1, (uint32_t)((float)b0 * guess_scale));
    if (first[g] <= b0) {
        lo = g + 1;
        for (uint32_t step = 1; lo < hi; step <<= 1) {
            const uint32_t probe = min(lo + step - 1, hi - 1);
            if (first[probe] <= b0) lo = probe + 1;
            else { hi = probe; break; }
        }
    } else {  // g >= 1 here, and first[0] = 0 <= b0 ends the loop at the latest
        hi = g;
        for (uint32_t step = 1; lo < hi; step <<= 1) {
            const uint32_t probe = hi > step ? hi - step : 0u;
            if (first[probe] > b0) hi = probe;
            else { lo = probe + 1; break; }
        }
    }
    while (lo < hi) {  // upper bound: the first entry whose first index is > b0
        const uint32_t mid = (lo + hi) >> 1;
        if (first[mid] <= b0) lo = mid + 1;
        else hi = mid;
    }
    const uint32_t i = b0 + threadIdx.x;
    if (i >= total) return;
    uint32_t e = lo - 1;
    while (e + 1 < n_entries && first[e + 1] <= i) ++e;
    // a wave that lies inside one cloud (nearly all do) reads the entry — pointer, flags, matrix — through the scalar cache
    const uint32_t eu = (uint32_t)__builtin_amdgcn_readfirstlane((int)e);
    float4 o;
    if (__all(e == eu)) o = merged_point(table + eu, i);
    else o = merged_point(table + e, i);
    out[i] = o;
}

}  // namespace

struct MergeScratch {
    DevBuf<unsigned char> table;     // n MergeEntry, then n uint32 first indices
    PinnedBuf<unsigned char> h_table;
    locgpu_cloud joined;             // the transformed and joined clouds, before the filter
};

namespace {

int hip_fail(locgpu_ctx* ctx, hipError_t e, const char* what) {
    hip_ok(ctx, e, what);
    return e == hipErrorOutOfMemory ? LOCGPU_ERR_OOM : LOCGPU_ERR_NO_DEVICE;
}

MergeScratch* scratch(locgpu_ctx* ctx) {
    if (!ctx->merge) {
        ctx->merge = new MergeScratch();
        ctx->merge->joined.ctx = ctx;
    }
    return ctx->merge;
}

// What the host knows of one source before anything is enqueued.
struct Source {
    const float4* p;
    size_t n;
    uint32_t flags;         // kDense | kZeroW
    const double* pose;     // 7 doubles or nullptr
};

// dst[0, total) = the sources, transformed and joined, on ctx->stream. total <= kMaxPoints and dst has room for it.
hipError_t merge_dev(locgpu_ctx* ctx, const std::vector<Source>& src, size_t total, float4* dst) {
    if (total == 0) return hipSuccess;
    MergeScratch* S = scratch(ctx);
    const size_t n = src.size();
    const size_t bytes = n * sizeof(MergeEntry) + n * sizeof(uint32_t);
    if (bytes > S->h_table.cap()) {
        const size_t cap = with_headroom(n + 16) * (sizeof(MergeEntry) + sizeof(uint32_t));
        LOCGPU_TRY(S->table.alloc(cap));
        LOCGPU_TRY(S->h_table.alloc(cap));
    }
    MergeEntry* entries = (MergeEntry*)S->h_table.get();
    uint32_t* first = (uint32_t*)(S->h_table.get() + n * sizeof(MergeEntry));
    size_t at = 0;
    for (size_t k = 0; k < n; ++k) {
        MergeEntry& t = entries[k];
        t.p = src[k].p;
        t.first = first[k] = (uint32_t)at;
        t.n = (uint32_t)src[k].n;
        t.flags = src[k].flags;
        t.pad = 0u;
        if (src[k].pose) {
            M34 m;
            pose_to_m34(src[k].pose, m);
            std::memcpy(t.m, m.v, sizeof(t.m));
            t.flags |= kTransform;
        } else {
            std::memset(t.m, 0, sizeof(t.m));
        }
        at += src[k].n;
    }
    // the caller synchronises the stream before it returns: the pinned table is free again at the next call
    LOCGPU_TRY(hipMemcpyAsync(S->table, S->h_table, bytes, hipMemcpyHostToDevice, ctx->stream));
    const unsigned blocks = (unsigned)((total + kMB - 1) / kMB);
    hipLaunchKernelGGL(merge_kernel, dim3(blocks), dim3(kMB), 0, ctx->stream, (const MergeEntry*)S->table.get(),
                       (const uint32_t*)(S->table.get() + n * sizeof(MergeEntry)), (uint32_t)n, (uint32_t)total, (float)((double)n / (double)total), dst);
    return hipGetLastError();
}

// GetGlobalMap's tail on ctx->stream: the sources joined into the context's scratch cloud, then the filter into `out` (leaf > 0) or
// the joined cloud itself swapped into `out` (leaf == 0). `dense` = is_dense of the joined cloud: operator+= ANDs the flags.
// Returns with the stream synchronised.
int merge_into(locgpu_ctx* ctx, const char* who, const std::vector<Source>& src, size_t total, int dense, float leaf, locgpu_cloud* out, int* passthrough) {
    locgpu_cloud* J = &scratch(ctx)->joined;
    hipError_t e = cloud_reserve(J, total, false);
    if (e == hipSuccess) e = merge_dev(ctx, src, total, J->d);
    J->n = total;
    J->is_dense = dense;
    int status = 0;
    if (e == hipSuccess) {
        if (leaf > 0.f) {
            e = voxel_filter_dev(ctx, J, leaf, out, &status);
        } else {
            out->d.swap(J->d);
            out->n = total;
            out->is_dense = dense;
        }
    }
    J->n = 0;
    const hipError_t se = hipStreamSynchronize(ctx->stream);  // blocking: foreign clouds and the batch are free again, the table too
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return hip_fail(ctx, e, who);
    if (passthrough) *passthrough = status == 1 ? 1 : 0;
    (void)cloud_mark_ready(out);
    return LOCGPU_OK;
}

bool leaf_ok(float leaf) { return leaf >= 0.f && std::isfinite(leaf); }

// The refusals locgpu_batch_download_scan makes of a batch.
const char* batch_refusal(const locgpu_batch* b) {
    if (b->shared_src) return "a shared-source batch holds one cloud, not scans";
    if (b->pending.active) return "an alignment of this batch has been begun and not finished";
    return nullptr;
}

}  // namespace

void merge_free(locgpu_ctx* ctx) {
    delete ctx->merge;
    ctx->merge = nullptr;
}

}  // namespace locgpu

using namespace locgpu;

extern "C" {

int locgpu_clouds_merge(locgpu_ctx* ctx, const locgpu_cloud* const* clouds, const double* poses, int n, float leaf, locgpu_cloud* out, int* passthrough) {
    if (!ctx || !clouds || !out) return fail(ctx, LOCGPU_ERR_INVALID, "clouds_merge: NULL context, cloud list or output cloud");
    if (n < 1) return fail(ctx, LOCGPU_ERR_INVALID, "clouds_merge: n >= 1 clouds required");
    if (!leaf_ok(leaf)) return fail(ctx, LOCGPU_ERR_INVALID, "clouds_merge: leaf size must be finite and >= 0 (0 joins without filtering)");
    if (out->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, "clouds_merge: the output cloud belongs to another context");
    size_t total = 0;
    int dense = 1;
    for (int i = 0; i < n; ++i) {
        const locgpu_cloud* c = clouds[i];
        if (!c || !c->ctx) return fail(ctx, LOCGPU_ERR_INVALID, "clouds_merge: NULL cloud " + std::to_string(i));
        if (c == out) return fail(ctx, LOCGPU_ERR_INVALID, "clouds_merge: the output cloud is among the inputs");
        if (c->ctx->device != ctx->device) return fail(ctx, LOCGPU_ERR_INVALID, "clouds_merge: cloud " + std::to_string(i) + " belongs to a context on another GPU");
        total += c->n;
        dense = (dense && c->is_dense) ? 1 : 0;
    }
    if (total > kMaxPoints) return fail(ctx, LOCGPU_ERR_INVALID, "clouds_merge: more than 2^31 points in total");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<Source> src((size_t)n);
    for (int i = 0; i < n; ++i) {
        const locgpu_cloud* c = clouds[i];
        const hipError_t e = cloud_input_ready(ctx, c);
        if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); return hip_fail(ctx, e, "clouds_merge: ordering behind the cloud's context"); }
        src[i] = Source{c->d.get(), c->n, c->is_dense ? kDense : 0u, poses ? poses + 7 * (size_t)i : nullptr};
    }
    return merge_into(ctx, "clouds_merge", src, total, dense, leaf, out, passthrough);
}

int locgpu_batch_merge(locgpu_batch* b, const double* poses, const uint8_t* use, float leaf, locgpu_cloud* out, int* passthrough) {
    if (!b || !out) return fail(b ? b->ctx : nullptr, LOCGPU_ERR_INVALID, "batch_merge: NULL batch or output cloud");
    locgpu_ctx* ctx = b->ctx;
    if (b->sharded) return fail(ctx, LOCGPU_ERR_INVALID, "batch_merge: sharded batches are not supported");
    if (const char* why = batch_refusal(b)) return fail(ctx, LOCGPU_ERR_INVALID, std::string("batch_merge: ") + why);
    if (!leaf_ok(leaf)) return fail(ctx, LOCGPU_ERR_INVALID, "batch_merge: leaf size must be finite and >= 0 (0 joins without filtering)");
    if (out->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, "batch_merge: the output cloud belongs to another context than the batch");
    std::vector<Source> src;
    src.reserve((size_t)b->n_scans);
    size_t total = 0;
    for (int s = 0; s < b->n_scans; ++s) {
        if (use && !use[s]) continue;
        // a scan as locgpu_batch_export_cloud makes it: {x, y, z, 0}, not flagged dense
        src.push_back(Source{b->d_src.get() + (size_t)s * b->max_n, (size_t)b->counts[s], kZeroW, poses ? poses + 7 * (size_t)s : nullptr});
        total += (size_t)b->counts[s];
    }
    if (total > kMaxPoints) return fail(ctx, LOCGPU_ERR_INVALID, "batch_merge: more than 2^31 points in total");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = order_behind_batch(ctx, b, "batch_merge: ordering behind the batch");
    if (rc != LOCGPU_OK) return rc;
    // no scan in use: the fresh cloud GetGlobalMap starts from (dense); otherwise operator+= has ANDed in a flag that is not set
    return merge_into(ctx, "batch_merge", src, total, src.empty() ? 1 : 0, leaf, out, passthrough);
}

int locgpu_batch_export_cloud(locgpu_batch* b, int scan, locgpu_cloud* cloud) {
    if (!b || !cloud || !cloud->ctx) return fail(b ? b->ctx : nullptr, LOCGPU_ERR_INVALID, "batch_export_cloud: NULL batch or cloud");
    locgpu_ctx* bctx = b->ctx;
    if (const char* why = batch_refusal(b)) return fail(bctx, LOCGPU_ERR_INVALID, std::string("batch_export_cloud: ") + why);
    if (scan < 0 || scan >= b->n_scans) return fail(bctx, LOCGPU_ERR_INVALID, "batch_export_cloud: scan index out of range");
    locgpu_ctx* ctx = cloud->ctx;  // the copy runs on the stream of the cloud's owner, like everything that writes the cloud
    if (ctx->device != bctx->device) return fail(bctx, LOCGPU_ERR_INVALID, "batch_export_cloud: the cloud belongs to a context on another GPU");
    LOCGPU_HIP(bctx, hipSetDevice(ctx->device));
    const int rc = order_behind_batch(ctx, b, "batch_export_cloud: ordering behind the batch");
    if (rc != LOCGPU_OK) {
        if (ctx != bctx) fail(bctx, rc, locgpu_last_error(ctx));
        return rc;
    }
    const size_t n = (size_t)b->counts[scan];
    hipError_t e = cloud_reserve(cloud, n, false);
    if (e == hipSuccess) e = merge_dev(ctx, std::vector<Source>{Source{b->d_src.get() + (size_t)scan * b->max_n, n, kZeroW, nullptr}}, n, cloud->d);
    // blocking: the batch may be written again when the call returns
    const hipError_t se = hipStreamSynchronize(ctx->stream);
    if (e == hipSuccess) e = se;
    if (e != hipSuccess) return hip_fail(bctx, e, "batch_export_cloud");
    cloud->n = n;
    cloud->is_dense = 0;  // a batch carries no flag: its scans are always tested for non-finite points (locgpu_batch_preprocess)
    (void)cloud_mark_ready(cloud);
    return LOCGPU_OK;
}

}  // extern "C"
