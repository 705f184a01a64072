// loc_lib_amd/csrc/icp_target.hip — SetInputTarget of the ICP matcher: the host-built packed KD-tree, its ingest into HBM (blocking, on
// a worker thread, broadcast over the communicator, from a resident cloud) and the exact-search grid built from it.
#include <chrono>
#include <cstdio>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "cloud_filters.hpp"
#include "context.hpp"
#include "env.hpp"
#include "kdtree_build.hpp"
#include "search_dispatch.hpp"

using namespace locgpu;

void locgpu::free_grid(locgpu_ctx* ctx) {
    locgpu::grid_free(ctx->grid_buf);
    ctx->grid = locgpu::GridView();
}

// Build the exact-search grid from the packed tree already in HBM (first use of LOCGPU_SEARCH_GRID_EXACT after a set_target).
int locgpu::ensure_grid(locgpu_ctx* ctx) {
    if (ctx->grid.pts) return LOCGPU_OK;
    { const int frc = refuse_forest(ctx, "grid search"); if (frc != LOCGPU_OK) return frc; }
    std::string msg;
    const hipError_t e = locgpu::grid_build_device(ctx->d_tree, ctx->d_leaf_slots, ctx->num_leaves, ctx->stream, ctx->grid_buf, ctx->grid, msg);
    if (e != hipSuccess) {
        free_grid(ctx);
        if (!msg.empty()) return locgpu::fail(ctx, LOCGPU_ERR_INVALID, "grid search: " + msg);
        locgpu::hip_ok(ctx, e, "grid build");
        return LOCGPU_ERR_NO_DEVICE;
    }
    return LOCGPU_OK;
}

// --------------------------------------------------------------------------------------------- target
// One target ingest's host side: the deep copy of the points, the packed tree, and — for the asynchronous entry points — the
// worker thread that builds it. The context keeps ONE of these between ingests (target_scratch): a keyframe front-end re-ingests
// its ≈35 k-point local map every few scans, and the vectors' capacity (≈1.4 MB: fresh mmaps and page faults per ingest) is
// worth keeping.
namespace locgpu {
struct PendingTarget {
    std::thread worker;
    std::vector<float> xyz;
    PackedKdTree tree;
    std::string err;
    bool ok = false;
};
}  // namespace locgpu

static locgpu::PendingTarget* take_target_scratch(locgpu_ctx* ctx) {
    locgpu::PendingTarget* p = ctx->target_scratch;
    ctx->target_scratch = nullptr;
    if (!p) p = new locgpu::PendingTarget();
    p->err.clear();
    p->ok = false;
    return p;
}

void locgpu::free_target_scratch(locgpu_ctx* ctx) {
    delete ctx->target_scratch;  // never holds a running worker (keep_target_scratch joins first)
    ctx->target_scratch = nullptr;
}

static void keep_target_scratch(locgpu_ctx* ctx, locgpu::PendingTarget* p) {
    if (p->worker.joinable()) p->worker.join();
    // a 10 M-point map's buffers (≈360 MB) go back to the allocator; a local map's stay
    if (ctx->target_scratch || p->xyz.capacity() > (size_t)3 << 21) delete p;
    else ctx->target_scratch = p;
}

// The reference's tree for `pts`, built on the host (kdtree_build.cpp).
static int build_host_tree(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes, std::vector<float>& xyz, PackedKdTree& t) {
    if (!pts || n == 0 || stride_bytes < 12) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target: empty cloud or stride < 12");
    // deep copy (icp_registration.cpp:16 + kdtree.cpp:267 copy too): pack xyz
    xyz.resize(3 * n);
    const char* base = (const char*)pts;
    for (size_t i = 0; i < n; ++i) std::memcpy(&xyz[3 * i], base + i * stride_bytes, 12);
    std::string err;
    if (!build_packed_kdtree(xyz.data(), n, t, err)) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target: " + err);
    if (t.depth > 64) return fail(ctx, LOCGPU_ERR_DEPTH, "icp_set_target: KD-tree depth " + std::to_string(t.depth) + " exceeds the 64-entry traversal stack");
    return LOCGPU_OK;
}

// meta = {slots, leaves, nodes, points, depth, bounded}. The device buffers only ever grow: a streaming front-end re-ingests its
// local map every keyframe (lio.cpp:296-305) and must not pay a hipMalloc/hipFree pair (≈100 µs each) per ingest.
int locgpu::install_tree_meta(locgpu_ctx* ctx, const long long meta[6]) {
    for (hipStream_t st : ctx->slot_stream) LOCGPU_HIP(ctx, hipStreamSynchronize(st));  // nobody reads the old tree any more (a begun alignment must be finished first)
    free_grid(ctx);
    const size_t slots = (size_t)meta[0], leaves = (size_t)meta[1];
    if (slots + 2 > ctx->d_tree.cap()) LOCGPU_HIP(ctx, ctx->d_tree.alloc(with_headroom(slots)));  // + the sentinel leaf behind the tree (search_walk.hpp)
    if (leaves > ctx->d_leaf_slots.cap()) LOCGPU_HIP(ctx, ctx->d_leaf_slots.alloc(with_headroom(leaves)));
    ctx->tree_slots = slots;
    ctx->num_leaves = leaves;
    ctx->num_nodes = (size_t)meta[2];
    ctx->num_points = (size_t)meta[3];
    ctx->depth = (int)meta[4];
    ctx->tree_bounded = meta[5] != 0 && slots + 2 <= kWalkMaxSlots;  // … and small enough for the walk kernels' 32-bit node references
    ctx->target_epoch++;
    ctx->planes_ready = false;  // the plane table belongs to the previous target (rebuilt on the next use of LOCGPU_P2PLANE_MAP)
    ctx->planes_rows = 0;
    ctx->planes_valid = 0;
    ctx->forest_n = 0;  // an ordinary target (set_target_forest_packed sets it again behind this call)
    ctx->forest_base.clear(); ctx->forest_leaves.clear(); ctx->forest_depth.clear();
    return LOCGPU_OK;
}

// The sentinel leaf behind the packed tree (two slots at index tree_slots): what a lane of the search kernel "visits" when it has
// no node to visit. Its coordinates are so large that the squared distance overflows to +inf for every sane query.
static hipError_t write_sentinel_leaf(locgpu_ctx* ctx) {
    return hipMemcpyAsync(ctx->d_tree + ctx->tree_slots, kSentinelLeafSlots, sizeof(kSentinelLeafSlots), hipMemcpyHostToDevice, ctx->stream);
}

// ---- SetInputTarget with the host build off the caller's thread (locgpu_icp_set_target_cloud_async) ----
// The mean-split tree is built on the host (its float32 sums are sequential by definition), 0.5–0.7 ms for a 35 k-pt local map. A
// streaming front-end that re-ingests its local map every keyframe (lio.cpp:296-305) has work to do in the meantime — upload and
// filter the next scan — so the build may run on a worker thread. Only the BUILD does: the worker touches its own copy of the points,
// its own PackedKdTree and the process-wide build pool, nothing of HIP and nothing of the context; every HIP call of the ingest
// (buffers, H2D, sentinel) is made by the caller's thread in target_join(), which every entry point that reads the target calls first.

static int install_built_tree(locgpu_ctx* ctx, const PackedKdTree& t) {
    const long long meta[6] = {(long long)t.slots.size(), (long long)t.num_leaves, (long long)t.num_nodes, (long long)t.num_points, t.depth, t.bounded ? 1 : 0};
    const int rc = install_tree_meta(ctx, meta);
    if (rc != LOCGPU_OK) return rc;
    LOCGPU_HIP(ctx, hipMemcpyAsync(ctx->d_tree, t.slots.data(), t.slots.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    LOCGPU_HIP(ctx, hipMemcpyAsync(ctx->d_leaf_slots, t.leaf_slots.data(), t.leaf_slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    LOCGPU_HIP(ctx, write_sentinel_leaf(ctx));
    LOCGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    return LOCGPU_OK;
}

// Finishes a pending asynchronous ingest (no-op without one). install = false: only wait for the worker (context teardown, or a new
// target that supersedes the pending one).
int locgpu::target_join(locgpu_ctx* ctx, bool install) {
    if (!ctx || !ctx->pending_target) return LOCGPU_OK;
    locgpu::PendingTarget* p = ctx->pending_target;
    ctx->pending_target = nullptr;
    if (p->worker.joinable()) p->worker.join();
    int rc = LOCGPU_OK;
    if (install) {
        if (!p->ok) rc = fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target: " + p->err);
        else if (p->tree.depth > 64) rc = fail(ctx, LOCGPU_ERR_DEPTH, "icp_set_target: KD-tree depth " + std::to_string(p->tree.depth) + " exceeds the 64-entry traversal stack");
        else if (hipSetDevice(ctx->device) != hipSuccess) rc = LOCGPU_ERR_NO_DEVICE;
        else rc = install_built_tree(ctx, p->tree);
    }
    keep_target_scratch(ctx, p);
    return rc;
}

// SetInputTarget from a resident cloud (locgpu_icp_set_target_cloud[_async]; the LOAM handle's classes, whose clouds always belong to
// another context: ctx's stream is then ordered behind the call that produced the cloud).
int locgpu::icp_set_target_from_cloud(locgpu_ctx* ctx, const locgpu_cloud* target, bool async) {
    if (target->n == 0) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target: empty cloud or stride < 12");
    (void)target_join(ctx, false);  // a pending asynchronous ingest is superseded
    // The mean-split tree is built on the host (its float32 sums are sequential by definition, kdtree.cpp:94-123), so the
    // cloud crosses PCIe once in each direction: 16 B/point down, the packed tree (≈24 B/point) up.
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    {
        const hipError_t ce = cloud_input_ready(ctx, target);
        if (ce == hipErrorInvalidDevice) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target_cloud: the cloud belongs to a context on another GPU");
        if (!hip_ok(ctx, ce, "icp_set_target_cloud: ordering behind the cloud's context")) return LOCGPU_ERR_NO_DEVICE;
    }
    float4* stage = nullptr;
    if (!hip_ok(ctx, cloud_stage(ctx, target->n, &stage), "pinned staging")) return LOCGPU_ERR_OOM;
    LOCGPU_HIP(ctx, hipMemcpyAsync(stage, target->d, target->n * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    LOCGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    if (!async) return locgpu_icp_set_target(ctx, stage, target->n, sizeof(float4));
    locgpu::PendingTarget* p = take_target_scratch(ctx);
    p->xyz.resize(3 * target->n);  // the deep copy of SetInputTarget (icp_registration.cpp:16): the staging block is free again after it
    for (size_t i = 0; i < target->n; ++i) std::memcpy(&p->xyz[3 * i], &stage[i], 12);
    const size_t n = target->n;
    p->worker = std::thread([p, n] { p->ok = build_packed_kdtree(p->xyz.data(), n, p->tree, p->err); });
    ctx->pending_target = p;
    return LOCGPU_OK;
}

// ---- a forest target: n trees behind one another in d_tree (kdtree_build.hpp, PackedForest), for the pairs calls ----
int locgpu::refuse_forest(locgpu_ctx* ctx, const char* who) {
    if (ctx->forest_n == 0) return LOCGPU_OK;
    return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": the context holds a forest target (locgpu_icp_set_target_forest), which only locgpu_icp_align_pairs / "
                                         "locgpu_icp_fitness_pairs read; locgpu_icp_set_target* makes it an ordinary target again");
}

// xyz[j]: n[j] packed float32 triples (already deep copies). Builds on the host, refuses before the context is touched, then replaces
// the target: one host-to-device copy for all trees and their sentinel leaves, and the table of bases.
static int set_target_forest_packed(locgpu_ctx* ctx, const float* const* xyz, const size_t* n, int n_targets, const char* who) {
    static const bool times = env_flag("LOCGPU_FOREST_TIMES");  // diagnostic: phase times on stderr
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!times) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[locgpu forest ingest] %s %.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    };
    PackedForest f;
    std::string err;
    int bad = -1;
    if (!build_packed_forest(xyz, n, n_targets, f, err, &bad))
        return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + (bad >= 0 ? ": target " + std::to_string(bad) + ": " : ": ") + err);
    for (int j = 0; j < n_targets; ++j)
        if (f.depth[j] > kMaxSearchDepth)
            return fail(ctx, LOCGPU_ERR_DEPTH, std::string(who) + ": target " + std::to_string(j) + ": KD-tree depth " + std::to_string(f.depth[j]) + " exceeds the " +
                                                   std::to_string(kMaxSearchDepth) + "-entry traversal stack");
    lap("host build");
    (void)target_join(ctx, false);  // a pending asynchronous ingest is superseded
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    // tree_slots: up to the LAST segment's sentinel leaf, which then stands where an ordinary tree's does
    const long long meta[6] = {(long long)f.slots.size() - 2, (long long)f.num_leaves, (long long)f.num_nodes, (long long)f.num_points, f.max_depth, f.bounded ? 1 : 0};
    if ((size_t)n_targets > ctx->d_forest_base.cap()) LOCGPU_HIP(ctx, ctx->d_forest_base.alloc(with_headroom((size_t)n_targets)));
    const int rc = install_tree_meta(ctx, meta);
    if (rc != LOCGPU_OK) return rc;
    LOCGPU_HIP(ctx, hipMemcpyAsync(ctx->d_tree, f.slots.data(), f.slots.size() * sizeof(uint64_t), hipMemcpyHostToDevice, ctx->stream));
    LOCGPU_HIP(ctx, hipMemcpyAsync(ctx->d_forest_base, f.base.data(), (size_t)n_targets * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    LOCGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    lap("device buffers + H2D");
    ctx->forest_n = n_targets;
    ctx->forest_base = std::move(f.base);
    ctx->forest_leaves = std::move(f.leaves);
    ctx->forest_depth = std::move(f.depth);
    return LOCGPU_OK;
}

extern "C" {

int locgpu_icp_set_target_forest(locgpu_ctx* ctx, const void* const* pts, const size_t* n, int n_targets, size_t stride_bytes) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!pts || !n || n_targets < 1) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target_forest: NULL arrays or n_targets < 1");
    for (int j = 0; j < n_targets; ++j)
        if (!pts[j] || n[j] == 0 || stride_bytes < 12)
            return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target_forest: target " + std::to_string(j) + ": empty cloud or stride < 12");
    // deep copies (icp_registration.cpp:16), packed xyz
    std::vector<std::vector<float>> xyz((size_t)n_targets);
    std::vector<const float*> ptr((size_t)n_targets);
    for (int j = 0; j < n_targets; ++j) {
        xyz[j].resize(3 * n[j]);
        const char* base = (const char*)pts[j];
        for (size_t i = 0; i < n[j]; ++i) std::memcpy(&xyz[j][3 * i], base + i * stride_bytes, 12);
        ptr[j] = xyz[j].data();
    }
    return set_target_forest_packed(ctx, ptr.data(), n, n_targets, "icp_set_target_forest");
}

int locgpu_icp_set_target_forest_batch(locgpu_ctx* ctx, const locgpu_batch* b) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!b || b->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target_forest_batch: NULL batch or a batch of another context");
    if (b->sharded || b->shared_src) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target_forest_batch: sharded and shared-source batches hold no scans of their own");
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target_forest_batch: an alignment of this batch has been begun and not finished");
    if (b->n_scans < 1) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target_forest_batch: the batch holds no scan");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    { const int orc = order_behind_batch(ctx, const_cast<locgpu_batch*>(b), "icp_set_target_forest_batch: ordering behind the batch"); if (orc != LOCGPU_OK) return orc; }
    const int n_targets = b->n_scans;
    std::vector<size_t> n((size_t)n_targets), off((size_t)n_targets);
    size_t total = 0;
    for (int j = 0; j < n_targets; ++j) {
        if (b->counts[j] <= 0) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target_forest_batch: target " + std::to_string(j) + ": empty cloud or stride < 12");
        n[j] = (size_t)b->counts[j];
        off[j] = total;
        total += n[j];
    }
    // The scans cross PCIe the way a cloud's points do in locgpu_icp_set_target_cloud: 16 B a point into the context's pinned staging
    // block, all scans behind one another, one wait.
    float4* stage = nullptr;
    if (!hip_ok(ctx, cloud_stage(ctx, total, &stage), "pinned staging")) return LOCGPU_ERR_OOM;
    for (int j = 0; j < n_targets; ++j)
        LOCGPU_HIP(ctx, hipMemcpyAsync(stage + off[j], b->d_src + (size_t)j * b->max_n, n[j] * sizeof(float4), hipMemcpyDeviceToHost, ctx->stream));
    LOCGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<float> xyz(3 * total);
    for (size_t i = 0; i < total; ++i) std::memcpy(&xyz[3 * i], &stage[i], 12);
    std::vector<const float*> ptr((size_t)n_targets);
    for (int j = 0; j < n_targets; ++j) ptr[j] = xyz.data() + 3 * off[j];
    return set_target_forest_packed(ctx, ptr.data(), n.data(), n_targets, "icp_set_target_forest_batch");
}

int locgpu_icp_forest_info(const locgpu_ctx* ctx, int* n_targets, size_t* leaves, int* depth) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    { const int jrc = target_join(const_cast<locgpu_ctx*>(ctx)); if (jrc != LOCGPU_OK) return jrc; }
    if (n_targets) *n_targets = ctx->forest_n;
    if (ctx->forest_n == 0) return fail(const_cast<locgpu_ctx*>(ctx), ctx->d_tree ? LOCGPU_ERR_INVALID : LOCGPU_ERR_NO_TARGET, "icp_forest_info: the context holds no forest target");
    for (int j = 0; j < ctx->forest_n; ++j) {
        if (leaves) leaves[j] = ctx->forest_leaves[j];
        if (depth) depth[j] = ctx->forest_depth[j];
    }
    return LOCGPU_OK;
}

int locgpu_icp_set_target(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    (void)target_join(ctx, false);  // a pending asynchronous ingest is superseded
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    static const bool times = env_flag("LOCGPU_INGEST_TIMES");  // diagnostic: phase times on stderr
    auto t0 = std::chrono::steady_clock::now();
    auto lap = [&](const char* what) {
        if (!times) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[locgpu ingest] %s %.3f ms\n", what, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    };
    locgpu::PendingTarget* p = take_target_scratch(ctx);
    int rc = build_host_tree(ctx, pts, n, stride_bytes, p->xyz, p->tree);
    lap("host build");
    if (rc == LOCGPU_OK) {
        rc = install_built_tree(ctx, p->tree);
        lap("device buffers + H2D");
    }
    keep_target_scratch(ctx, p);
    return rc;
}

// The same with the host build on a worker thread (see PendingTarget): returns once the points have been copied.
int locgpu_icp_set_target_async(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!pts || n == 0 || stride_bytes < 12) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target: empty cloud or stride < 12");
    (void)target_join(ctx, false);  // an earlier pending ingest is superseded
    locgpu::PendingTarget* p = take_target_scratch(ctx);
    p->xyz.resize(3 * n);  // the deep copy of SetInputTarget (icp_registration.cpp:16)
    const char* base = (const char*)pts;
    for (size_t i = 0; i < n; ++i) std::memcpy(&p->xyz[3 * i], base + i * stride_bytes, 12);
    p->worker = std::thread([p, n] { p->ok = build_packed_kdtree(p->xyz.data(), n, p->tree, p->err); });
    ctx->pending_target = p;
    return LOCGPU_OK;
}

// Collective over the context's communicator: rank `root` builds the tree from its `pts` (the other ranks' pts/n are ignored)
// and broadcasts the packed tree over xGMI — one host build per node instead of one per GPU.
int locgpu_icp_set_target_bcast(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes, int root) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!ctx->comm) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target_bcast: locgpu_comm_init has not been called");
    if (root < 0 || root >= ctx->comm_world) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target_bcast: bad root");
    (void)target_join(ctx, false);  // a pending asynchronous ingest is superseded
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    PackedKdTree t;
    std::vector<float> xyz;
    long long meta[8] = {0, 0, 0, 0, 0, 0, 0, 0};  // [6] = the root's status
    int rc = LOCGPU_OK;
    if (ctx->comm_rank == root) {
        rc = build_host_tree(ctx, pts, n, stride_bytes, xyz, t);
        if (rc == LOCGPU_OK) { meta[0] = (long long)t.slots.size(); meta[1] = (long long)t.num_leaves; meta[2] = (long long)t.num_nodes; meta[3] = (long long)t.num_points; meta[4] = t.depth; meta[5] = t.bounded ? 1 : 0; }
        meta[6] = rc;
    }
    DevBuf<long long> d_meta;
    LOCGPU_HIP(ctx, d_meta.alloc(8));
    bool ok = hip_ok(ctx, hipMemcpyAsync(d_meta, meta, sizeof(meta), hipMemcpyHostToDevice, s), "bcast meta H2D");
    ok = ok && comm_broadcast(ctx, d_meta, sizeof(meta), root, s);
    ok = ok && hip_ok(ctx, hipMemcpyAsync(meta, d_meta, sizeof(meta), hipMemcpyDeviceToHost, s), "bcast meta D2H") && hip_ok(ctx, hipStreamSynchronize(s), "sync");
    d_meta.reset();
    if (!ok) return fail(ctx, LOCGPU_ERR_NO_DEVICE, "icp_set_target_bcast: broadcast of the tree header failed");
    if (meta[6] != LOCGPU_OK) return ctx->comm_rank == root ? (int)meta[6] : fail(ctx, (int)meta[6], "icp_set_target_bcast: the root rank could not build the tree");
    rc = install_tree_meta(ctx, meta);
    {
        // collective error exit: a rank that could not make room for the tree must not leave the others waiting in the broadcast
        DevBuf<int> d_rc;
        int all_rc = rc;
        bool okc = hip_ok(ctx, d_rc.alloc(1), "bcast status") &&
                   hip_ok(ctx, hipMemcpyAsync(d_rc, &rc, sizeof(int), hipMemcpyHostToDevice, s), "bcast status H2D");
        okc = okc && comm_all_reduce_min_int(ctx, d_rc, s);  // status codes are <= 0
        okc = okc && hip_ok(ctx, hipMemcpyAsync(&all_rc, d_rc, sizeof(int), hipMemcpyDeviceToHost, s), "bcast status D2H") && hip_ok(ctx, hipStreamSynchronize(s), "sync");
        if (!okc) return fail(ctx, LOCGPU_ERR_NO_DEVICE, "icp_set_target_bcast: status exchange failed");
        if (rc != LOCGPU_OK) return rc;
        if (all_rc != LOCGPU_OK) return fail(ctx, all_rc, "icp_set_target_bcast: another rank could not allocate the tree buffers");
    }
    if (ctx->comm_rank == root) {
        LOCGPU_HIP(ctx, hipMemcpyAsync(ctx->d_tree, t.slots.data(), t.slots.size() * sizeof(uint64_t), hipMemcpyHostToDevice, s));
        LOCGPU_HIP(ctx, hipMemcpyAsync(ctx->d_leaf_slots, t.leaf_slots.data(), t.leaf_slots.size() * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    }
    if (!comm_broadcast(ctx, ctx->d_tree, ctx->tree_slots * sizeof(uint64_t), root, s) || !comm_broadcast(ctx, ctx->d_leaf_slots, ctx->num_leaves * sizeof(uint32_t), root, s))
        return fail(ctx, LOCGPU_ERR_NO_DEVICE, "icp_set_target_bcast: broadcast of the tree failed");
    LOCGPU_HIP(ctx, write_sentinel_leaf(ctx));
    LOCGPU_HIP(ctx, hipStreamSynchronize(s));
    return LOCGPU_OK;
}

int locgpu_icp_target_info(const locgpu_ctx* ctx, int64_t out[4]) {
    if (!ctx || !out) return LOCGPU_ERR_INVALID;
    { const int jrc = target_join(const_cast<locgpu_ctx*>(ctx)); if (jrc != LOCGPU_OK) return jrc; }
    out[0] = (int64_t)ctx->num_leaves;
    out[1] = (int64_t)ctx->num_nodes;
    out[2] = ctx->depth;
    out[3] = (int64_t)(ctx->tree_slots * sizeof(uint64_t));
    return ctx->d_tree ? LOCGPU_OK : LOCGPU_ERR_NO_TARGET;
}

// ---- from a cloud resident in HBM (cloud_filters.hpp) ----
int locgpu_icp_set_target_cloud(locgpu_ctx* ctx, const locgpu_cloud* target) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!target || target->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target_cloud: bad cloud");
    return icp_set_target_from_cloud(ctx, target, false);
}

int locgpu_icp_set_target_cloud_async(locgpu_ctx* ctx, const locgpu_cloud* target) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!target || target->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, "icp_set_target_cloud: bad cloud");
    return icp_set_target_from_cloud(ctx, target, true);
}

}  // extern "C"
