// loc_lib_amd/csrc/locgpu_api.hip — C ABI of include/locgpu.h: context, batches, k-NN and the matchers' entry points.
//
// An entry point checks its arguments and calls into the Gauss–Newton driver (gn_driver.hip), the target ingest (icp_target.hip) or the
// communicator (comm.hip). Host control flow mirrors the reference's matcher (IcpRegistration, icp_registration.cpp): SetInputTarget
// builds the search structure once per map; ScanMatch runs the Gauss–Newton loop.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "batch_upload.hpp"
#include "cloud_filters.hpp"
#include "context.hpp"
#include "gn_driver.hpp"
#include "launch.hpp"
#include "ndt_inc.hpp"
#include "ndt_kernels.hpp"
#include "ndt_pairs.hpp"
#include "search_chunks.hpp"

using namespace locgpu;

namespace {
std::string g_create_err;
}  // namespace

namespace locgpu {
int fail(locgpu_ctx* ctx, int code, const std::string& msg) {
    if (ctx) ctx->err = msg;
    else g_create_err = msg;
    return code;
}
bool hip_ok(locgpu_ctx* ctx, hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    fail(ctx, LOCGPU_ERR_NO_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return false;
}
}  // namespace locgpu

// Zero-fill of device memory that is COMPLETE when the call returns (see alloc_batch: a plain hipMemset is not, and is not ordered
// with the context's non-blocking streams either).
static bool fill_now(locgpu_ctx* ctx, void* p, size_t bytes, const char* what) {
    return hip_ok(ctx, hipMemsetAsync(p, 0, bytes, ctx->stream), what) && hip_ok(ctx, hipStreamSynchronize(ctx->stream), what);
}

void locgpu::free_batch(locgpu_batch* b) {
    if (!b) return;
    upload_free_batch(b);
    if (b->leased) b->ctx->slot_load[b->slot]--;  // destroyed with an alignment begun and not ended: its stream is free again
    if (b->graph_exec) (void)hipGraphExecDestroy(b->graph_exec);
    if (b->graph_exec_next) (void)hipGraphExecDestroy(b->graph_exec_next);
    delete b;
}

// The two solve-stage test hooks: caller-chosen block partials through the production launchers (launch_gn_solve, launch_sum_partials,
// launch_loam_solve) on buffers that live for the call. A state row is a PoseState, byte for byte (the header documents the offsets).
static_assert(sizeof(PoseState) == 160 && offsetof(PoseState, t) == 32 && offsetof(PoseState, R) == 56 && offsetof(PoseState, last_dx_norm) == 128 &&
                  offsetof(PoseState, last_eff) == 136 && offsetof(PoseState, iterations) == 144 && offsetof(PoseState, converged) == 148 &&
                  offsetof(PoseState, done) == 152 && offsetof(PoseState, status) == 156,
              "the state row of locgpu_debug_gn_solve / locgpu_debug_loam_solve (include/locgpu.h) is PoseState");
constexpr int kDebugMaxScans = 1024, kDebugMaxBlocks = 4096;

// upload → `launch` on the context's stream → state and hb back; the stream is synchronised before the buffers die, whatever failed
template <typename Launch>
static int debug_solve_run(locgpu_ctx* ctx, const double* const partials[2], const int blocks[2], int n_scans, const int* scans, int n_launch, bool want_acc,
                           const void* state_in, void* state_out, double* hb_out, int hb_w, Launch launch) {
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    DevBuf<double> d_part[2], d_acc, d_hb;
    DevBuf<PoseState> d_st;
    DevBuf<int> d_scans;
    const size_t st_bytes = (size_t)n_scans * sizeof(PoseState), hb_bytes = (size_t)n_scans * hb_w * sizeof(double);
    bool ok = hip_ok(ctx, d_st.alloc(n_scans), "hipMalloc state") && hip_ok(ctx, d_hb.alloc((size_t)n_scans * hb_w), "hipMalloc hb") &&
              (!want_acc || hip_ok(ctx, d_acc.alloc((size_t)n_scans * kAccW), "hipMalloc acc")) && (!scans || hip_ok(ctx, d_scans.alloc(n_launch), "hipMalloc scans"));
    for (int c = 0; ok && c < 2; ++c)
        if (partials[c]) ok = hip_ok(ctx, d_part[c].alloc((size_t)n_scans * blocks[c] * kAccW), "hipMalloc partials");
    if (!ok) return LOCGPU_ERR_OOM;
    for (int c = 0; ok && c < 2; ++c)
        if (partials[c]) ok = hip_ok(ctx, hipMemcpyAsync(d_part[c], partials[c], (size_t)n_scans * blocks[c] * kAccW * sizeof(double), hipMemcpyHostToDevice, s), "H2D partials");
    ok = ok && hip_ok(ctx, hipMemcpyAsync(d_st, state_in, st_bytes, hipMemcpyHostToDevice, s), "H2D state") &&
         hip_ok(ctx, hipMemcpyAsync(d_hb, hb_out, hb_bytes, hipMemcpyHostToDevice, s), "H2D hb") &&  // rows no block writes come back as they went in
         (!scans || hip_ok(ctx, hipMemcpyAsync(d_scans, scans, (size_t)n_launch * sizeof(int), hipMemcpyHostToDevice, s), "H2D scans"));
    if (ok) {
        launch(d_part[0].get(), d_part[1].get(), d_st.get(), d_acc.get(), d_hb.get(), scans ? d_scans.get() : nullptr, s);
        ok = hip_ok(ctx, hipGetLastError(), "debug solve launch") && hip_ok(ctx, hipMemcpyAsync(state_out, d_st, st_bytes, hipMemcpyDeviceToHost, s), "D2H state") &&
             hip_ok(ctx, hipMemcpyAsync(hb_out, d_hb, hb_bytes, hipMemcpyDeviceToHost, s), "D2H hb");
    }
    if (!hip_ok(ctx, hipStreamSynchronize(s), "debug solve sync")) ok = false;
    return ok ? LOCGPU_OK : LOCGPU_ERR_NO_DEVICE;
}

extern "C" {

void locgpu_icp_opts_default(locgpu_icp_opts* o) {
    if (!o) return;
    o->method = LOCGPU_P2P;  // IcpOptions::method_{IcpMethod::P2P}, icp_registration.hpp:38
    o->max_iteration = 20;
    o->max_nn_distance = 1.0;
    o->max_plane_distance = 0.1;
    o->max_line_distance = 0.5;
    o->min_effective_pts = 10;
    o->eps = 1e-2;
    o->approximate = 1;
    o->ann_alpha = 0.1f;
    o->search_mode = LOCGPU_SEARCH_TREE_FAITHFUL;
}

void locgpu_ndt_opts_default(locgpu_ndt_opts* o) {
    if (!o) return;
    o->max_iteration = 20;
    o->voxel_size = 1.0;
    o->min_effective_pts = 10;
    o->min_pts_in_voxel = 3;
    o->eps = 1e-2;
    o->res_outlier_th = 20.0;
    o->nearby_type = kNearby6;
    o->method = kNdtOptDirect;
    o->capacity = 100000;
}

int locgpu_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return 0;
    return n;
}

int locgpu_create(int device_id, locgpu_ctx** out) {
    if (!out) return fail(nullptr, LOCGPU_ERR_INVALID, "locgpu_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, LOCGPU_ERR_NO_DEVICE, std::string("no HIP device available (there is no CPU fallback): ") + hipGetErrorString(e));
    if (device_id < 0 || device_id >= n) return fail(nullptr, LOCGPU_ERR_INVALID, "locgpu_create: device_id out of range");
    auto* ctx = new locgpu_ctx();
    ctx->device = device_id;
    locgpu_ndt_opts_default(&ctx->ndt_opts);
    bool ok = hip_ok(nullptr, hipSetDevice(device_id), "hipSetDevice");
    for (int i = 0; ok && i < locgpu_ctx::kSlots; ++i) ok = hip_ok(nullptr, hipStreamCreateWithFlags(&ctx->slot_stream[i], hipStreamNonBlocking), "hipStreamCreate");
    // The copy stream and the communication stream are created HERE, right behind the compute streams: HIP deals streams to its
    // (four) hardware queues in creation order, and a copy stream that lands in the queue of a compute stream gets its H2D chunks
    // in between that stream's kernels only. (Seen with an RCCL communicator on the context: its internal streams shifted the
    // lazily created copy stream onto the first compute stream's queue — every upload that ran beside an alignment on that stream took
    // 31 ms instead of 14.)
    ok = ok && hip_ok(nullptr, hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking), "hipStreamCreate");
    ok = ok && hip_ok(nullptr, hipStreamCreateWithFlags(&ctx->comm_stream, hipStreamNonBlocking), "hipStreamCreate");
    if (!ok) {
        for (hipStream_t st : ctx->slot_stream) if (st) (void)hipStreamDestroy(st);
        if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
        if (ctx->comm_stream) (void)hipStreamDestroy(ctx->comm_stream);
        delete ctx;
        return LOCGPU_ERR_NO_DEVICE;
    }
    ctx->stream = ctx->slot_stream[0];
    if (!search_kernels_lds_ok()) {
        locgpu_destroy(ctx);
        return fail(nullptr, LOCGPU_ERR_INVALID, "locgpu_create: a search kernel of this build owns static LDS — its traversal stack would not start at LDS address 0 (search_walk.hpp)");
    }
    *out = ctx;
    return LOCGPU_OK;
}

void locgpu_destroy(locgpu_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    (void)target_join(ctx, false);
    free_target_scratch(ctx);
    for (hipStream_t st : ctx->slot_stream) if (st) (void)hipStreamSynchronize(st);
    if (ctx->comm_stream) (void)hipStreamSynchronize(ctx->comm_stream);
    delete ctx->worker;  // joins the helper thread (no job outlives the call that started it)
    free_batch(ctx->single);
    free_batch(ctx->search);
    free_batch(ctx->planes_ws);
    upload_free_ctx(ctx);
    comm_destroy(ctx);
    if (ctx->comm_stream) (void)hipStreamDestroy(ctx->comm_stream);
    if (ctx->copy_stream) (void)hipStreamDestroy(ctx->copy_stream);
    free_grid(ctx);
    ndt_free(ctx);
    filters_free(ctx);
    loam_free(ctx);
    range_ingest_free(ctx);
    record_ingest_free(ctx);
    resident_deskew_free(ctx);
    forest_build_free(ctx);
    for (hipStream_t st : ctx->slot_stream) if (st) (void)hipStreamDestroy(st);
    delete ctx;
}

const char* locgpu_last_error(const locgpu_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_err.c_str(); }

// --------------------------------------------------------------------------------------------- k-NN
int locgpu_knn(locgpu_ctx* ctx, const float* queries, size_t nq, int k, int approximate, float alpha, int search_mode, int32_t* out_idx,
               uint32_t* visits) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    { const int jrc = target_join(ctx); if (jrc != LOCGPU_OK) return jrc; }
    if (!ctx->d_tree) return fail(ctx, LOCGPU_ERR_NO_TARGET, "knn: no target set");
    { const int frc = refuse_forest(ctx, "knn"); if (frc != LOCGPU_OK) return frc; }
    if (!queries || !out_idx || k < 1 || k > 8) return fail(ctx, LOCGPU_ERR_INVALID, "knn: bad arguments (1 <= k <= 8)");
    if (search_mode != LOCGPU_SEARCH_TREE_FAITHFUL && search_mode != LOCGPU_SEARCH_GRID_EXACT) return fail(ctx, LOCGPU_ERR_INVALID, "knn: unknown search mode");
    if ((size_t)k > ctx->num_leaves) return fail(ctx, LOCGPU_ERR_K_TOO_LARGE, "knn: k larger than the number of tree leaves");
    if (nq == 0) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    const bool grid = search_mode == LOCGPU_SEARCH_GRID_EXACT;
    if (grid) {
        if (k != 1 && k != 5) return fail(ctx, LOCGPU_ERR_INVALID, "knn: grid search supports k = 1 or 5");
        const int grc = ensure_grid(ctx);
        if (grc != LOCGPU_OK) return grc;
    }
    DevBuf<float> d_q;
    DevBuf<int32_t> d_out;
    DevBuf<uint32_t> d_vis;
    DevBuf<unsigned int> d_flag;
    int rc = LOCGPU_OK;
    if (!hip_ok(ctx, d_q.alloc(nq * 3), "hipMalloc") || !hip_ok(ctx, d_out.alloc(nq * k), "hipMalloc") || !hip_ok(ctx, d_flag.alloc(1), "hipMalloc") ||
        (visits && !hip_ok(ctx, d_vis.alloc(nq * 2), "hipMalloc")))
        return LOCGPU_ERR_OOM;
    hipStream_t s = ctx->stream;
    if (!hip_ok(ctx, hipMemcpyAsync(d_q, queries, nq * 12, hipMemcpyHostToDevice, s), "H2D")) rc = LOCGPU_ERR_NO_DEVICE;
    if (rc == LOCGPU_OK && grid) {
        // grid kernel first; the queries it cannot settle (out_idx[i*k] == -2) are answered by the exact tree traversal
        unsigned int flagged = 0;
        (void)hipMemsetAsync(d_flag, 0, 4, s);
        if (!launch_knn_grid_query(ctx->grid, ctx->d_tree, d_q, nq, k, d_out, d_flag, s)) rc = fail(ctx, LOCGPU_ERR_INVALID, "knn: unsupported k");
        if (rc == LOCGPU_OK && (!hip_ok(ctx, hipMemcpyAsync(out_idx, d_out, nq * k * 4, hipMemcpyDeviceToHost, s), "D2H") ||
                                !hip_ok(ctx, hipMemcpyAsync(&flagged, d_flag, 4, hipMemcpyDeviceToHost, s), "D2H") ||
                                !hip_ok(ctx, hipStreamSynchronize(s), "sync")))
            rc = LOCGPU_ERR_NO_DEVICE;
        if (rc == LOCGPU_OK && visits) std::memset(visits, 0, nq * 8);
        if (rc == LOCGPU_OK && flagged) {
            std::vector<int32_t> tmp(nq * k);
            if (!launch_knn_query(ctx->d_tree, ctx->depth, d_q, nq, k, 1.0f, d_out, nullptr, s)) rc = fail(ctx, LOCGPU_ERR_DEPTH, "knn: unsupported k/depth");
            if (rc == LOCGPU_OK && (!hip_ok(ctx, hipMemcpyAsync(tmp.data(), d_out, nq * k * 4, hipMemcpyDeviceToHost, s), "D2H") ||
                                    !hip_ok(ctx, hipStreamSynchronize(s), "sync")))
                rc = LOCGPU_ERR_NO_DEVICE;
            if (rc == LOCGPU_OK)
                for (size_t i = 0; i < nq; ++i)
                    if (out_idx[i * k] == -2)
                        for (int j = 0; j < k; ++j) out_idx[i * k + j] = tmp[i * k + j];
        }
        return rc;
    }
    if (rc == LOCGPU_OK && !launch_knn_query(ctx->d_tree, ctx->depth, d_q, nq, k, approximate ? alpha : 1.0f, d_out, d_vis, s))
        rc = fail(ctx, LOCGPU_ERR_DEPTH, "knn: unsupported k/depth");
    if (rc == LOCGPU_OK && !hip_ok(ctx, hipGetLastError(), "knn launch")) rc = LOCGPU_ERR_NO_DEVICE;
    if (rc == LOCGPU_OK && !hip_ok(ctx, hipMemcpyAsync(out_idx, d_out, nq * k * 4, hipMemcpyDeviceToHost, s), "D2H")) rc = LOCGPU_ERR_NO_DEVICE;
    if (rc == LOCGPU_OK && visits && !hip_ok(ctx, hipMemcpyAsync(visits, d_vis, nq * 8, hipMemcpyDeviceToHost, s), "D2H")) rc = LOCGPU_ERR_NO_DEVICE;
    if (!hip_ok(ctx, hipStreamSynchronize(s), "sync") && rc == LOCGPU_OK) rc = LOCGPU_ERR_NO_DEVICE;
    return rc;
}

// --------------------------------------------------------------------------------------------- batches
}  // extern "C"

// Device buffers + pinned result staging for n_scans scans of at most max_n points each; no points yet.
int locgpu::alloc_batch(locgpu_ctx* ctx, int n_scans, size_t max_n, locgpu_batch** out, int first, int n_total, bool shared_src) {
    if (!ctx || !out) return LOCGPU_ERR_INVALID;
    *out = nullptr;
    const bool sharded = n_total >= 0;
    if (!sharded) n_total = n_scans;
    if (shared_src && (sharded || n_scans < 1)) return fail(ctx, LOCGPU_ERR_INVALID, "batch_create: a shared-source batch cannot be sharded or empty");
    // a sharded batch may hold NO scan on this rank (more ranks than scans): it then only contributes zeros to the exchange
    if (n_scans < 0 || (n_scans == 0 && !sharded) || first < 0 || first + n_scans > n_total) return fail(ctx, LOCGPU_ERR_INVALID, "batch_create: bad arguments");
    if (n_total > 65535) return fail(ctx, LOCGPU_ERR_INVALID, "batch_create: at most 65535 scans per batch");
    if (n_scans > 65535) return fail(ctx, LOCGPU_ERR_INVALID, "batch_create: at most 65535 scans per batch");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    if (n_scans == 0) max_n = 1;
    if (max_n == 0 || max_n > 0x7FFFFF00u || (size_t)n_scans * max_n > 0xFFFFFFF0ull)
        return fail(ctx, LOCGPU_ERR_INVALID, "batch_create: scans are empty or the batch exceeds 2^32 points");
    auto* b = new locgpu_batch();
    b->ctx = ctx;
    b->slot = ctx->next_slot;
    ctx->next_slot = (ctx->next_slot + 1) % locgpu_ctx::kSlots;
    b->stream = ctx->slot_stream[b->slot];
    b->n_scans = n_scans;
    b->n_total = n_total;
    b->first = first;
    b->sharded = sharded;
    b->max_n = (int)max_n;
    b->blocks_per_scan = (int)((max_n + kBlock - 1) / kBlock);
    b->pitch = (size_t)n_scans * max_n;
    b->counts.assign(n_scans, 0);
    b->shared_src = shared_src;
    b->cap_scans = n_scans;
    b->cap_points = max_n;
    // a shared-source batch holds ONE region of points, whatever its number of entries, and a zero per entry that says so
    bool ok = hip_ok(ctx, b->d_src.alloc(std::max<size_t>(shared_src ? max_n : b->pitch, 1)), "hipMalloc src") &&
              (!shared_src || (hip_ok(ctx, b->d_src_of.alloc((size_t)n_scans), "hipMalloc src_of") &&
                               fill_now(ctx, b->d_src_of, (size_t)n_scans * sizeof(int), "hipMemset src_of"))) &&
              hip_ok(ctx, b->d_counts.alloc(std::max(n_scans, 1)), "hipMalloc counts") &&
              hip_ok(ctx, b->d_state.alloc(n_total), "hipMalloc state") &&
              (!sharded || hip_ok(ctx, b->d_acc.alloc((size_t)kFirstChunk * n_total * kAccW), "hipMalloc acc")) &&  // one slot per iteration of a chunk
              hip_ok(ctx, b->d_nn.alloc(5 * std::max<size_t>(b->pitch, 1)), "hipMalloc nn") &&
              hip_ok(ctx, b->d_run_flags.alloc(std::max<size_t>((size_t)n_scans * ((max_n + 63) / 64), 1)), "hipMalloc run flags") &&  // a smaller shape of a shared-source batch needs no more words
              hip_ok(ctx, b->d_partials.alloc((size_t)std::max(n_scans, 1) * b->blocks_per_scan * kAccW), "hipMalloc partials") &&
              hip_ok(ctx, b->d_hb.alloc((size_t)n_total * 44), "hipMalloc hb") &&
              hip_ok(ctx, b->d_redo_list.alloc((stamp_build() ? 2 : 1) * std::max<size_t>(b->pitch, 1)), "hipMalloc redo") &&  // diagnostic build: + per-query trip counts
              hip_ok(ctx, b->d_redo_list2.alloc(std::max<size_t>(b->pitch, 1)), "hipMalloc redo2") &&  // deep pass / grid search: second work list
              hip_ok(ctx, b->d_redo_count.alloc(4), "hipMalloc redo") &&  // [0] redo list, [1] deep list, [2..3] spare
              hip_ok(ctx, b->h_state.alloc(n_total), "hipHostMalloc state") &&
              hip_ok(ctx, b->h_hb.alloc((size_t)n_total * 44), "hipHostMalloc hb") &&
              hip_ok(ctx, b->h_active.alloc((size_t)std::max(n_scans, 1)), "hipHostMalloc active") &&
              hip_ok(ctx, b->d_active.alloc((size_t)std::max(n_scans, 1)), "hipMalloc active") &&
              // hipMemset runs on the NULL stream and returns before it has run; the context's streams are non-blocking, i.e. NOT ordered
              // behind it — the first upload of the scan counts could be overtaken by this very fill (the first alignment of a fresh
              // batch then saw a scan of zero points and ran its 20 iterations on nothing; once in ≈1000 first calls, found by
              // tools/fuzz_align.py --cases 120 in round 4). fill_now: on the context's stream, and waited for.
              fill_now(ctx, b->d_counts, std::max(n_scans, 1) * sizeof(int), "hipMemset counts") &&
              fill_now(ctx, b->d_redo_count, 4 * sizeof(unsigned int), "hipMemset redo");  // kept zero between searches by gn_solve_kernel
    if (!ok) { free_batch(b); return LOCGPU_ERR_OOM; }
    *out = b;
    return LOCGPU_OK;
}

extern "C" {

// Batch with the given scans resident when the call returns (deep copy of the sources, icp_registration.cpp:259).
static int make_batch(locgpu_ctx* ctx, const void* const* srcs, const size_t* counts, size_t stride_bytes, int n_scans, locgpu_batch** out,
                      int first = 0, int n_total = -1) {
    if (!ctx || !out) return LOCGPU_ERR_INVALID;
    *out = nullptr;
    if (n_scans < 0 || (n_scans > 0 && (!srcs || !counts)) || stride_bytes < 12) return fail(ctx, LOCGPU_ERR_INVALID, "batch_create: bad arguments");
    size_t max_n = 0;
    for (int s = 0; s < n_scans; ++s) max_n = std::max(max_n, counts[s]);
    for (int s = 0; s < n_scans; ++s)
        if (!srcs[s] && counts[s]) return fail(ctx, LOCGPU_ERR_INVALID, "batch_create: NULL scan pointer");
    locgpu_batch* b = nullptr;
    int rc = alloc_batch(ctx, n_scans, max_n, &b, first, n_total);
    if (rc != LOCGPU_OK) return rc;
    if (n_scans > 0) {
        rc = upload_start(b, srcs, counts, stride_bytes);
        if (rc == LOCGPU_OK) rc = upload_join_batch(b);
        if (rc == LOCGPU_OK && !hip_ok(ctx, upload_wait_landed(b), "batch_create: H2D")) rc = LOCGPU_ERR_NO_DEVICE;
    }
    if (rc != LOCGPU_OK) { free_batch(b); return rc; }
    *out = b;
    return LOCGPU_OK;
}

int locgpu_batch_create(locgpu_ctx* ctx, const void* const* srcs, const size_t* counts, size_t stride_bytes, int n_scans, locgpu_batch** out) {
    return make_batch(ctx, srcs, counts, stride_bytes, n_scans, out);
}

int locgpu_batch_create_empty(locgpu_ctx* ctx, int n_scans, size_t max_points_per_scan, locgpu_batch** out) {
    return alloc_batch(ctx, n_scans, max_points_per_scan, out);
}

int locgpu_batch_upload_async(locgpu_batch* b, const void* const* srcs, const size_t* counts, size_t stride_bytes) {
    if (!b) return LOCGPU_ERR_INVALID;
    if (b->shared_src) return fail(b->ctx, LOCGPU_ERR_INVALID, "batch upload: a shared-source batch takes its cloud when it is created");
    LOCGPU_HIP(b->ctx, hipSetDevice(b->ctx->device));
    return upload_start(b, srcs, counts, stride_bytes);
}

int locgpu_batch_upload_wait(locgpu_batch* b) {
    if (!b) return LOCGPU_ERR_INVALID;
    return upload_join_batch(b);
}

int locgpu_batch_create_sharded(locgpu_ctx* ctx, const void* const* srcs, const size_t* counts, size_t stride_bytes, int n_local, int first_scan,
                                int n_total, locgpu_batch** out) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (n_total <= 0) return fail(ctx, LOCGPU_ERR_INVALID, "batch_create_sharded: n_total must be positive");
    // Without a communicator nobody else can contribute the scans this rank does not hold: their sums would silently stay zero.
    if (!ctx->comm && !(first_scan == 0 && n_local == n_total))
        return fail(ctx, LOCGPU_ERR_INVALID, "batch_create_sharded: this rank holds only part of the batch and locgpu_comm_init has not been called");
    const int rc = make_batch(ctx, srcs, counts, stride_bytes, n_local, out, first_scan, n_total);
    if (rc != LOCGPU_OK) return rc;
    locgpu_batch* b = *out;
    if (!hip_ok(ctx, b->ev_ready.ensure(), "batch_create_sharded: hipEventCreate") || !hip_ok(ctx, b->ev_reduced.ensure(), "batch_create_sharded: hipEventCreate")) {
        free_batch(b);
        *out = nullptr;
        return LOCGPU_ERR_OOM;
    }
    return LOCGPU_OK;
}

void locgpu_batch_destroy(locgpu_batch* b) {
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    (void)hipStreamSynchronize(b->stream);
    if (b->sharded && b->ctx->comm_stream) (void)hipStreamSynchronize(b->ctx->comm_stream);
    free_batch(b);
}

}  // extern "C"

namespace locgpu {

// The batch argument of entry point `who` (args_ok: its other pointers are there). Scan pools and sharded batches do not take the
// map-plane method (locgpu.h).
static int check_batch(locgpu_ctx* ctx, const locgpu_batch* b, bool args_ok, const AlignSpec& spec, const char* who) {
    if (!b || b->ctx != ctx || !args_ok) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": bad arguments");
    if (b->sharded && spec.prm.method == LOCGPU_P2PLANE_MAP)
        return fail(ctx, LOCGPU_ERR_INVALID, "icp: LOCGPU_P2PLANE_MAP is not available on a sharded batch");
    return LOCGPU_OK;
}

// pairs: the request of locgpu_icp_align_pairs, which reads a forest target and nothing else; every other request reads an ordinary one.
static int check_icp_request(locgpu_ctx* ctx, const locgpu_icp_opts* o, AlignSpec& spec, bool pairs) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!o) return fail(ctx, LOCGPU_ERR_INVALID, "icp: opts is NULL");
    { const int jrc = target_join(ctx); if (jrc != LOCGPU_OK) return jrc; }  // an asynchronous SetInputTarget ends here at the latest
    if (!ctx->d_tree) return fail(ctx, LOCGPU_ERR_NO_TARGET, "icp: SetInputTarget has not been called");
    if (!pairs) { const int frc = refuse_forest(ctx, "icp"); if (frc != LOCGPU_OK) return frc; }
    if (pairs && ctx->forest_n == 0)
        return fail(ctx, LOCGPU_ERR_INVALID, "icp_align_pairs: the context holds an ordinary target; the pairs calls read a forest target (locgpu_icp_set_target_forest)");
    if ((o->method < LOCGPU_P2P || o->method > LOCGPU_P2PLANE) && o->method != LOCGPU_P2PLANE_MAP) return fail(ctx, LOCGPU_ERR_INVALID, "icp: unknown method");
    if (o->search_mode != LOCGPU_SEARCH_TREE_FAITHFUL && o->search_mode != LOCGPU_SEARCH_GRID_EXACT)
        return fail(ctx, LOCGPU_ERR_INVALID, "icp: unknown search mode");
    if (pairs && (o->method == LOCGPU_P2PLANE_MAP || o->search_mode == LOCGPU_SEARCH_GRID_EXACT))
        return fail(ctx, LOCGPU_ERR_INVALID, "icp_align_pairs: LOCGPU_P2PLANE_MAP and LOCGPU_SEARCH_GRID_EXACT are not available over a forest target");
    spec.pairs = pairs;
    if (o->search_mode == LOCGPU_SEARCH_GRID_EXACT) {
        const int rc = ensure_grid(ctx);
        if (rc != LOCGPU_OK) return rc;
    }
    GnParams& prm = spec.prm;
    prm.method = o->method;
    prm.max_iteration = o->max_iteration;
    prm.min_effective_pts = o->min_effective_pts;
    prm.eps = o->eps;
    prm.max_nn_distance = o->max_nn_distance;
    prm.max_plane_distance = o->max_plane_distance;
    prm.max_line_distance = o->max_line_distance;
    if (o->method == LOCGPU_P2PLANE_MAP) {  // the first use without a table builds it
        const int rc = ensure_map_planes(ctx);
        if (rc != LOCGPU_OK) return rc;
    }
    spec.grid = o->search_mode == LOCGPU_SEARCH_GRID_EXACT;  // exact by construction: `approximate` and ann_alpha are ignored
    spec.alpha = (o->approximate && !spec.grid) ? o->ann_alpha : 1.0f;
    // k > size_: GetClosestPoint logs an error and returns nothing (kdtree.cpp:149-153) ⇒ no correspondences at all.
    // The search kernel reproduces that by never filling the k-th slot; nothing to reject here.
    return LOCGPU_OK;
}

int check_icp(locgpu_ctx* ctx, const locgpu_icp_opts* o, AlignSpec& spec) { return check_icp_request(ctx, o, spec, false); }

// The batch and the target_of array of pairs call `who`, checked in full before anything of the batch is written; then the per-scan
// words the driver uploads (b->pair_base, b->pair_skip; pair_words, ndt_set_key.hpp): of n_targets targets, word i = base[target_of[i]]
// (ICP: the tree bases of the forest) or, base == nullptr, target_of[i] itself (NDT: the target's index in the voxel set).
static int check_pairs(locgpu_ctx* ctx, locgpu_batch* b, const int* target_of, bool args_ok, const char* who, int n_targets, const uint32_t* base) {
    if (!b || b->ctx != ctx || !target_of || !args_ok) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": bad arguments (NULL, or a batch of another context)");
    if (b->sharded || b->shared_src) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": sharded and shared-source batches are not aligned in pairs");
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": an alignment of this batch has been begun and not finished");
    if (b->n_scans < 1) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": the batch holds no scan");
    std::string err;
    if (!pair_words(target_of, b->n_scans, n_targets, base, b->pair_base, b->pair_skip, err)) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": " + err);
    return LOCGPU_OK;
}

// The reusable one-scan batch (device buffers + pinned staging) with room for n points.
static int single_reserve(locgpu_ctx* ctx, size_t n, locgpu_batch** out) {
    if (n == 0) return fail(ctx, LOCGPU_ERR_INVALID, "source cloud is empty");
    locgpu_batch* b = ctx->single;
    if (!b || (size_t)b->max_n < n || !b->h_src) {
        if (b) { free_batch(b); ctx->single = nullptr; }
        // device buffers with headroom, then pinned staging of the same capacity
        const size_t cap = with_headroom(n);
        const int rc = alloc_batch(ctx, 1, cap, &ctx->single);
        if (rc != LOCGPU_OK) return rc;
        b = ctx->single;
        b->slot = 0;  // single-scan calls share the stream of the clouds and of the target ingest
        b->stream = ctx->stream;
        b->pinned = true;
        if (!hip_ok(ctx, b->h_src.alloc(cap), "hipHostMalloc src")) { free_batch(b); ctx->single = nullptr; return LOCGPU_ERR_OOM; }
    }
    *out = b;
    return LOCGPU_OK;
}

static int single_batch(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, locgpu_batch** out) {
    // The reference deep-copies the source on every call (SetSource, icp_registration.cpp:252-265); so do we — but into buffers
    // that are kept between calls: a per-scan caller (Loc::Update at 10-20 Hz) must not pay a dozen hipMalloc/hipFree per scan.
    if (n == 0) return fail(ctx, LOCGPU_ERR_INVALID, "source cloud is empty");
    if (!src || stride_bytes < 12) return fail(ctx, LOCGPU_ERR_INVALID, "source cloud: NULL pointer or stride < 12");
    locgpu_batch* b = nullptr;
    const int rc = single_reserve(ctx, n, &b);
    if (rc != LOCGPU_OK) return rc;
    pack_points((const char*)src, stride_bytes, n, b->h_src);
    b->d_src_ext = nullptr;
    b->counts[0] = (int)n;
    LOCGPU_HIP(ctx, hipMemcpyAsync(b->d_src, b->h_src, n * sizeof(float4), hipMemcpyHostToDevice, b->stream));
    LOCGPU_HIP(ctx, hipMemcpyAsync(b->d_counts, b->counts.data(), sizeof(int), hipMemcpyHostToDevice, b->stream));
    *out = b;
    return LOCGPU_OK;
}

// Same, from a cloud that is already in HBM (the w lane carries the intensity; no kernel of the matcher reads it).
static int single_batch_dev(locgpu_ctx* ctx, const float4* d_src, size_t n, locgpu_batch** out) {
    locgpu_batch* b = nullptr;
    const int rc = single_reserve(ctx, n, &b);
    if (rc != LOCGPU_OK) return rc;
    b->counts[0] = (int)n;
    // The call that follows is synchronous and only reads the points: they stay where the cloud holds them (a D2D copy was one more
    // dispatch in front of every match of the streaming loop). A captured graph has the batch's own buffer in its kernel arguments.
    b->d_src_ext = ctx->use_graph ? nullptr : d_src;
    if (!b->d_src_ext) LOCGPU_HIP(ctx, hipMemcpyAsync(b->d_src, d_src, n * sizeof(float4), hipMemcpyDeviceToDevice, b->stream));
    LOCGPU_HIP(ctx, hipMemcpyAsync(b->d_counts, b->counts.data(), sizeof(int), hipMemcpyHostToDevice, b->stream));
    *out = b;
    return LOCGPU_OK;
}

// The single-scan alignment of entry point `who`: the scan is `cloud`, resident in HBM, or else n points on the host at `src`.
static int align_single(locgpu_ctx* ctx, const AlignSpec& spec, const char* who, bool args_ok, const void* src, size_t n, size_t stride_bytes,
                        const locgpu_cloud* cloud, const double init_pose[7], double out_pose[7], locgpu_align_stats* stats) {
    if (!args_ok) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": bad arguments");
    locgpu_batch* b = nullptr;
    int rc;
    if (cloud) {
        const hipError_t ce = cloud_input_ready(ctx, cloud);
        if (ce == hipErrorInvalidDevice) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": the cloud belongs to a context on another GPU");
        if (!hip_ok(ctx, ce, (std::string(who) + ": ordering behind the cloud's context").c_str())) return LOCGPU_ERR_NO_DEVICE;
        rc = single_batch_dev(ctx, cloud->d, cloud->n, &b);
    } else {
        rc = single_batch(ctx, src, n, stride_bytes, &b);
    }
    return rc != LOCGPU_OK ? rc : run_align(ctx, b, init_pose, spec, out_pose, stats);
}

}  // namespace locgpu

extern "C" {

int locgpu_icp_align_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* init_poses, const locgpu_icp_opts* opts, double* out_poses,
                           locgpu_align_stats* stats) {
    AlignSpec spec;
    int rc = check_icp(ctx, opts, spec);
    if (rc == LOCGPU_OK) rc = check_batch(ctx, b, init_poses && out_poses, spec, "icp_align_batch");
    return rc != LOCGPU_OK ? rc : run_align(ctx, b, init_poses, spec, out_poses, stats);
}

int locgpu_icp_align_pairs(locgpu_ctx* ctx, locgpu_batch* b, const int* target_of, const double* init_poses, const locgpu_icp_opts* opts, double* out_poses,
                           locgpu_align_stats* stats) {
    AlignSpec spec;
    int rc = check_icp_request(ctx, opts, spec, true);
    if (rc == LOCGPU_OK) rc = check_pairs(ctx, b, target_of, out_poses != nullptr, "icp_align_pairs", ctx->forest_n, ctx->forest_base.data());
    if (rc != LOCGPU_OK) return rc;
    std::vector<double> identity;
    if (!init_poses) {  // the reference's `SE3 init_pos` of every scan-to-scan match (test_node.cpp:289)
        identity.assign(7 * (size_t)b->n_total, 0.0);
        for (int i = 0; i < b->n_total; ++i) identity[7 * (size_t)i + 3] = 1.0;
        init_poses = identity.data();
    }
    return run_align(ctx, b, init_poses, spec, out_poses, stats);
}

int locgpu_icp_fitness_pairs(locgpu_ctx* ctx, locgpu_batch* b, const int* target_of, const double* poses, double max_range, locgpu_fitness* out) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    { const int jrc = target_join(ctx); if (jrc != LOCGPU_OK) return jrc; }
    if (!ctx->d_tree) return fail(ctx, LOCGPU_ERR_NO_TARGET, "icp_fitness_pairs: SetInputTarget has not been called");
    if (ctx->forest_n == 0)
        return fail(ctx, LOCGPU_ERR_INVALID, "icp_fitness_pairs: the context holds an ordinary target; the pairs calls read a forest target (locgpu_icp_set_target_forest)");
    const int rc = check_pairs(ctx, b, target_of, poses && out && !std::isnan(max_range), "icp_fitness_pairs", ctx->forest_n, ctx->forest_base.data());
    return rc != LOCGPU_OK ? rc : fitness_pairs_on_batch(ctx, b, poses, max_range, out);
}

int locgpu_icp_align_batch_begin(locgpu_ctx* ctx, locgpu_batch* b, const double* init_poses, const locgpu_icp_opts* opts) {
    AlignSpec spec;
    int rc = check_icp(ctx, opts, spec);
    if (rc == LOCGPU_OK) rc = check_batch(ctx, b, init_poses != nullptr, spec, "icp_align_batch_begin");
    return rc != LOCGPU_OK ? rc : align_begin(ctx, b, init_poses, spec);
}

int locgpu_align_batch_end(locgpu_ctx* ctx, locgpu_batch* b, double* out_poses, locgpu_align_stats* stats) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!b || b->ctx != ctx || !out_poses) return fail(ctx, LOCGPU_ERR_INVALID, "align_batch_end: bad arguments");
    return align_finish(ctx, b, out_poses, stats);
}

int locgpu_icp_align(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double init_pose[7], const locgpu_icp_opts* opts,
                     double out_pose[7], locgpu_align_stats* stats) {
    AlignSpec spec;
    const int rc = check_icp(ctx, opts, spec);
    return rc != LOCGPU_OK ? rc : align_single(ctx, spec, "icp_align", src && init_pose && out_pose, src, n, stride_bytes, nullptr, init_pose, out_pose, stats);
}

int locgpu_icp_hb_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, const locgpu_icp_opts* opts, double* hb) {
    AlignSpec spec;
    int rc = check_icp(ctx, opts, spec);
    if (rc == LOCGPU_OK) rc = check_batch(ctx, b, poses && hb, spec, "icp_hb_batch");
    return rc != LOCGPU_OK ? rc : eval_hb_batch(ctx, b, poses, spec, hb, "icp_hb_batch");
}

int locgpu_debug_batch_nn(locgpu_ctx* ctx, locgpu_batch* b, int k, int32_t* out) {
    if (!ctx || !b || b->ctx != ctx || !out || k < 1 || k > 5) return fail(ctx, LOCGPU_ERR_INVALID, "debug_batch_nn: bad arguments");
    { const int jrc = target_join(ctx); if (jrc != LOCGPU_OK) return jrc; }
    if (!ctx->d_tree) return fail(ctx, LOCGPU_ERR_NO_TARGET, "debug_batch_nn: no ICP target");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    const size_t nq = (size_t)b->n_scans * b->max_n;
    DevBuf<int32_t> d_out;
    LOCGPU_HIP(ctx, d_out.alloc(nq * k));
    launch_nn_to_index(ctx->d_tree, ctx->tree_slots, b->d_nn, b->pitch, b->d_counts, b->max_n, nq, k, d_out, b->stream);
    const hipError_t e = hipMemcpyAsync(out, d_out, nq * k * sizeof(int32_t), hipMemcpyDeviceToHost, b->stream);
    const hipError_t e2 = hipStreamSynchronize(b->stream);
    LOCGPU_HIP(ctx, e);
    LOCGPU_HIP(ctx, e2);
    return LOCGPU_OK;
}

int locgpu_debug_batch_run_flags(locgpu_ctx* ctx, locgpu_batch* b, uint64_t* out, int* written) {
    if (!ctx || !b || b->ctx != ctx || !out || !written) return fail(ctx, LOCGPU_ERR_INVALID, "debug_batch_run_flags: bad arguments");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    const size_t words = (size_t)b->n_scans * (((size_t)b->max_n + 63) / 64);
    const hipError_t e = hipMemcpyAsync(out, b->d_run_flags, words * sizeof(uint64_t), hipMemcpyDeviceToHost, b->stream);
    const hipError_t e2 = hipStreamSynchronize(b->stream);
    LOCGPU_HIP(ctx, e);
    LOCGPU_HIP(ctx, e2);
    *written = b->run_flags_written ? 1 : 0;
    return LOCGPU_OK;
}

int locgpu_debug_gn_solve(locgpu_ctx* ctx, const double* partials, int n_scans, int blocks_per_scan, int method, int min_effective_pts, double eps,
                          int max_iteration, int do_update, int two_stage, const int* scans, int n_launch, const void* state_in, void* state_out, double* hb_out) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!partials || !state_in || !state_out || !hb_out) return fail(ctx, LOCGPU_ERR_INVALID, "debug_gn_solve: NULL argument");
    if (n_scans < 1 || n_scans > kDebugMaxScans || blocks_per_scan < 1 || blocks_per_scan > kDebugMaxBlocks)
        return fail(ctx, LOCGPU_ERR_INVALID, "debug_gn_solve: n_scans outside [1, 1024] or blocks_per_scan outside [1, 4096]");
    if (!(method == LOCGPU_P2P || method == LOCGPU_P2LINE || method == LOCGPU_P2PLANE || method == LOCGPU_P2PLANE_MAP || method_is_ndt(method)))
        return fail(ctx, LOCGPU_ERR_INVALID, "debug_gn_solve: unknown method");
    if (scans) {
        if (n_launch < 1 || n_launch > n_scans) return fail(ctx, LOCGPU_ERR_INVALID, "debug_gn_solve: n_launch outside [1, n_scans]");
        std::vector<char> seen(n_scans, 0);
        for (int i = 0; i < n_launch; ++i) {  // two blocks on one scan would race on its state
            if (scans[i] < 0 || scans[i] >= n_scans || seen[scans[i]]) return fail(ctx, LOCGPU_ERR_INVALID, "debug_gn_solve: a scans entry is out of range or listed twice");
            seen[scans[i]] = 1;
        }
    }
    GnParams prm{};
    prm.method = method;
    prm.max_iteration = max_iteration;
    prm.min_effective_pts = min_effective_pts;
    prm.eps = eps;
    const double* const parts[2] = {partials, nullptr};
    const int blocks[2] = {blocks_per_scan, 0};
    const int n_solve = scans ? n_launch : n_scans;
    return debug_solve_run(ctx, parts, blocks, n_scans, scans, n_solve, two_stage != 0, state_in, state_out, hb_out, 44,
                           [&](const double* d_part, const double*, PoseState* d_st, double* d_acc, double* d_hb, const int* d_scans, hipStream_t s) {
                               if (two_stage) {  // the sharded route: every scan's sum as a one-row partial, then the solve on those rows
                                   launch_sum_partials(d_part, blocks_per_scan, d_st, 0, n_scans, n_scans, d_acc, s);
                                   launch_gn_solve(d_acc, 1, d_st, n_solve, prm, do_update, d_hb, nullptr, s, d_scans);
                               } else {
                                   launch_gn_solve(d_part, blocks_per_scan, d_st, n_solve, prm, do_update, d_hb, nullptr, s, d_scans);
                               }
                           });
}

int locgpu_debug_loam_solve(locgpu_ctx* ctx, const double* partials_surf, int blocks_surf, const double* partials_edge, int blocks_edge, int n_scans,
                            const int min_effective_pts[2], double eps, int max_iteration, int do_update, const void* state_in, void* state_out, double* hb_out) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if ((!partials_surf && !partials_edge) || !min_effective_pts || !state_in || !state_out || !hb_out) return fail(ctx, LOCGPU_ERR_INVALID, "debug_loam_solve: NULL argument");
    if (n_scans < 1 || n_scans > kDebugMaxScans || (partials_surf && (blocks_surf < 1 || blocks_surf > kDebugMaxBlocks)) ||
        (partials_edge && (blocks_edge < 1 || blocks_edge > kDebugMaxBlocks)))
        return fail(ctx, LOCGPU_ERR_INVALID, "debug_loam_solve: n_scans outside [1, 1024] or a class's blocks outside [1, 4096]");
    const double* const parts[2] = {partials_surf, partials_edge};
    const int blocks[2] = {partials_surf ? blocks_surf : 0, partials_edge ? blocks_edge : 0};
    return debug_solve_run(ctx, parts, blocks, n_scans, nullptr, n_scans, false, state_in, state_out, hb_out, kLoamHbW,
                           [&](const double* d_surf, const double* d_edge, PoseState* d_st, double*, double* d_hb, const int*, hipStream_t s) {
                               LoamSolveArgs a{};
                               a.partials[0] = d_surf; a.partials[1] = d_edge;
                               for (int c = 0; c < 2; ++c) { a.blocks_per_scan[c] = blocks[c]; a.min_effective_pts[c] = min_effective_pts[c]; a.list_counts[c] = nullptr; }
                               a.max_iteration = max_iteration;
                               a.eps = eps;
                               a.st = d_st;
                               a.do_update = do_update;
                               a.hb_out = d_hb;
                               a.scans = nullptr;
                               launch_loam_solve(a, n_scans, s);
                           });
}

int locgpu_icp_hb(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double pose[7], const locgpu_icp_opts* opts, double H[36],
                  double B[6], int64_t* effective_num, int* ok) {
    AlignSpec spec;
    int rc = check_icp(ctx, opts, spec);
    if (rc != LOCGPU_OK) return rc;
    if (!src || !pose || !H || !B) return fail(ctx, LOCGPU_ERR_INVALID, "icp_hb: bad arguments");
    locgpu_batch* b = nullptr;
    rc = single_batch(ctx, src, n, stride_bytes, &b);
    if (rc != LOCGPU_OK) return rc;
    double hb[44];
    rc = eval_hb_batch(ctx, b, pose, spec, hb, "icp_hb");
    if (rc != LOCGPU_OK) return rc;
    std::memcpy(H, hb, 36 * sizeof(double));
    std::memcpy(B, hb + 36, 6 * sizeof(double));
    if (effective_num) *effective_num = (int64_t)hb[42];
    if (ok) *ok = hb[43] != 0.0;
    return LOCGPU_OK;
}

int locgpu_icp_build_map_planes(locgpu_ctx* ctx) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    { const int jrc = target_join(ctx); if (jrc != LOCGPU_OK) return jrc; }
    if (!ctx->d_tree) return fail(ctx, LOCGPU_ERR_NO_TARGET, "icp_build_map_planes: SetInputTarget has not been called");
    { const int frc = refuse_forest(ctx, "icp_build_map_planes"); if (frc != LOCGPU_OK) return frc; }
    return ensure_map_planes(ctx);
}

int locgpu_icp_map_planes_info(const locgpu_ctx* ctx, int64_t out[3]) {
    if (!ctx || !out) return LOCGPU_ERR_INVALID;
    { const int jrc = target_join(const_cast<locgpu_ctx*>(ctx)); if (jrc != LOCGPU_OK) return jrc; }
    out[0] = out[1] = out[2] = 0;
    if (!ctx->d_tree) return LOCGPU_ERR_NO_TARGET;
    if (!ctx->planes_ready) return LOCGPU_OK;
    out[0] = (int64_t)ctx->planes_rows;
    out[1] = (int64_t)ctx->planes_valid;
    out[2] = (int64_t)((ctx->tree_slots / 2 + 2) * 4 * sizeof(double));
    return LOCGPU_OK;
}

int locgpu_icp_map_planes_dump(locgpu_ctx* ctx, double* n4, uint8_t* valid, size_t cap, size_t* n_out) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    int rc = locgpu_icp_build_map_planes(ctx);
    if (rc != LOCGPU_OK) return rc;
    const size_t n = ctx->num_points;
    if (n_out) *n_out = n;
    if (!n4 && !valid && cap == 0 && n_out) return LOCGPU_OK;  // size query
    if (!n4 || !valid || cap < n) return fail(ctx, LOCGPU_ERR_INVALID, "icp_map_planes_dump: NULL output or capacity below the number of target points");
    DevBuf<double> d_n4;
    DevBuf<unsigned char> d_valid;
    hipStream_t s = ctx->stream;
    bool ok = hip_ok(ctx, d_n4.alloc(std::max<size_t>(n, 1) * 4), "hipMalloc") && hip_ok(ctx, d_valid.alloc(std::max<size_t>(n, 1)), "hipMalloc");
    if (!ok) rc = LOCGPU_ERR_OOM;
    ok = ok && hip_ok(ctx, hipMemsetAsync(d_n4, 0, n * 4 * sizeof(double), s), "hipMemset") && hip_ok(ctx, hipMemsetAsync(d_valid, 0, n, s), "hipMemset");
    if (ok && ctx->num_leaves > 0) launch_map_plane_dump(ctx->d_tree, ctx->d_leaf_slots, ctx->num_leaves, ctx->d_planes, n, d_n4, d_valid, s);
    ok = ok && hip_ok(ctx, hipGetLastError(), "map_planes_dump launch") && hip_ok(ctx, hipMemcpyAsync(n4, d_n4, n * 4 * sizeof(double), hipMemcpyDeviceToHost, s), "D2H") &&
         hip_ok(ctx, hipMemcpyAsync(valid, d_valid, n, hipMemcpyDeviceToHost, s), "D2H");
    if (!hip_ok(ctx, hipStreamSynchronize(s), "sync")) ok = false;
    return ok ? LOCGPU_OK : (rc != LOCGPU_OK ? rc : LOCGPU_ERR_NO_DEVICE);
}

int locgpu_gn_update(const double hb[44], int method, int min_effective_pts, double eps, double pose[7], double dx[6], int* applied, int* stop) {
    if (!hb || !pose || !dx) return LOCGPU_ERR_INVALID;
    for (int i = 0; i < 6; ++i) dx[i] = 0.0;
    if (applied) *applied = 0;
    if (stop) *stop = 0;
    const double det = lu6_det_solve(hb, hb + 36, dx);
    const bool ok = ((long long)hb[42] >= min_effective_pts) && !(det == 0.0);
    if (!ok) { for (int i = 0; i < 6; ++i) dx[i] = 0.0; return LOCGPU_OK; }
    if (method == LOCGPU_P2P)
        for (int i = 0; i < 6; ++i) dx[i] = dx[i] / 16;
    se3_apply_update(pose, pose + 4, dx);
    // dx.norm() in the association of gn_solve_kernel and of the reference's binary (icp_fit.hip, gn_update): summed left to
    // right the square can differ in its last bit, and with it a stop decision that falls on eps
    const double n2 = (dx[0] * dx[0] + (dx[2] * dx[2] + dx[4] * dx[4])) + (dx[1] * dx[1] + (dx[3] * dx[3] + dx[5] * dx[5]));
    if (applied) *applied = 1;
    if (stop) *stop = std::sqrt(n2) < eps;
    return LOCGPU_OK;
}

// The output cloud of ScanMatch (pcl::transformPointCloud(*src, *out, pose.matrix().cast<float>()), icp_registration.cpp:241,
// ndt_registration.cpp:258): the points of the one-scan batch `b` (they are in HBM from the alignment, or were just uploaded) go through
// transform_cloud_kernel into the batch's neighbour-list array (dead by now: 20 B per point, 12 needed), come back through the batch's
// pinned staging and are written x, y, z into the caller's points. No allocation, no second upload, one kernel, one copy.
static int write_output_cloud(locgpu_ctx* ctx, locgpu_batch* b, const float4* d_points, size_t n, const double pose[7], void* out, size_t out_stride) {
    double R[9];
    quat_to_R(pose, R);
    M12f m;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) m.v[4 * r + c] = (float)R[3 * r + c];
        m.v[4 * r + 3] = (float)pose[4 + r];
    }
    float* d_xyz = reinterpret_cast<float*>(b->d_nn.get());
    float* h_xyz = reinterpret_cast<float*>(b->h_src.get());
    launch_transform_cloud(d_points, n, m, d_xyz, b->stream);
    LOCGPU_HIP(ctx, hipGetLastError());
    // back in up to eight pieces, each with an event: the host writes piece i into the caller's points while the later ones cross PCIe —
    // the even pieces on the caller's thread, the odd ones on the context's helper thread (12 of every 32 bytes of a 3.7 MB array: the
    // write is what costs, and two cores do it in half the time)
    constexpr int kMaxPieces = 8;
    const size_t piece = std::max<size_t>(32 * 1024, (n + kMaxPieces - 1) / kMaxPieces);
    const int pieces = (int)((n + piece - 1) / piece);
    for (int p = 0; p < pieces; ++p) {
        LOCGPU_HIP(ctx, b->xyz_ev[p].ensure());
        const size_t lo = (size_t)p * piece, len = std::min(piece, n - lo);
        LOCGPU_HIP(ctx, hipMemcpyAsync(h_xyz + 3 * lo, d_xyz + 3 * lo, len * 3 * sizeof(float), hipMemcpyDeviceToHost, b->stream));
        LOCGPU_HIP(ctx, hipEventRecord(b->xyz_ev[p], b->stream));
    }
    char* ob = (char*)out;
    std::atomic<int> failed{0};
    auto scatter = [&, ob, h_xyz](int first) {
        for (int p = first; p < pieces; p += 2) {
            if (hipEventSynchronize(b->xyz_ev[p]) != hipSuccess) { failed = 1; return; }
            const size_t lo = (size_t)p * piece, hi = std::min(n, lo + piece);
            for (size_t i = lo; i < hi; ++i) std::memcpy(ob + i * out_stride, h_xyz + 3 * i, 12);
        }
    };
    if (ctx->worker) ctx->worker->wait();  // the copy of the other fields (scan_match_fields) is through
    const bool two = pieces > 1 && ctx->worker;
    if (two) ctx->worker->run([&] { (void)hipSetDevice(ctx->device); scatter(1); });
    scatter(0);
    if (two) ctx->worker->wait(); else if (pieces > 1) scatter(1);
    if (failed) return fail(ctx, LOCGPU_ERR_NO_DEVICE, "output cloud: copy back");
    return LOCGPU_OK;
}

// "*out = *src" of pcl::transformPointCloud — every field of a source point that the output point has room for — on the context's
// helper thread so that it runs beside the alignment; with out_fn the helper first ASKS for the output array (a façade sizes the
// caller's container there: 3.7 MB of first-touch page faults for a full scan, off the caller's thread). scan_match_output waits for
// it, then writes the coordinates. *dst receives the output array (written by the helper; read after wait()).
static void scan_match_fields(locgpu_ctx* ctx, const void* src, size_t n, size_t src_stride, void* out, size_t out_stride, locgpu_out_cloud_fn out_fn,
                              void* user, void** dst) {
    *dst = out;
    if (out_stride & LOCGPU_OUT_FIELDS_DONE) {  // the caller (or its callback) leaves the fields in place itself
        if (!out_fn) return;
        if (!ctx->worker) ctx->worker = new locgpu::HostWorker();
        ctx->worker->run([=] { *dst = out_fn(user, n); });
        return;
    }
    if ((!out && !out_fn) || (!out_fn && out == src) || n == 0) return;
    if (!ctx->worker) ctx->worker = new locgpu::HostWorker();
    ctx->worker->run([=] {
        void* o = out_fn ? out_fn(user, n) : out;
        *dst = o;
        if (!o || o == src) return;
        if (src_stride == out_stride) { std::memcpy(o, src, n * src_stride); return; }
        const size_t w = std::min(src_stride, out_stride);
        const char* sb = (const char*)src;
        char* ob = (char*)o;
        for (size_t i = 0; i < n; ++i) std::memcpy(ob + i * out_stride, sb + i * src_stride, w);
    });
}
static int scan_match_output(locgpu_ctx* ctx, locgpu_batch* b, size_t n, int rc, const double pose[7], void** dst, size_t out_stride) {
    if (ctx->worker) ctx->worker->wait();
    if (rc != LOCGPU_OK || !*dst) return rc;
    return write_output_cloud(ctx, b, b->d_src, n, pose, *dst, out_stride & ~LOCGPU_OUT_FIELDS_DONE);
}

// ScanMatch of either matcher: align the scan, then transform it by the result into the caller's output cloud.
static int scan_match(locgpu_ctx* ctx, const AlignSpec& spec, const char* who, const void* src, size_t n, size_t stride_bytes, const double init_pose[7],
                      double result_pose[7], locgpu_align_stats* stats, void* out_cloud, size_t out_stride_bytes, locgpu_out_cloud_fn out_fn, void* out_user) {
    if (!src || !init_pose || !result_pose || ((out_cloud || out_fn) && (out_stride_bytes & ~LOCGPU_OUT_FIELDS_DONE) < 12)) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": bad arguments");
    locgpu_batch* b = nullptr;
    int rc = single_batch(ctx, src, n, stride_bytes, &b);
    if (rc != LOCGPU_OK) return rc;
    void* dst = nullptr;
    scan_match_fields(ctx, src, n, stride_bytes, out_cloud, out_stride_bytes, out_fn, out_user, &dst);
    double pose[7];
    locgpu_align_stats st{};
    rc = run_align(ctx, b, init_pose, spec, pose, &st);
    if (stats && (rc == LOCGPU_OK || spec.ndt())) *stats = st;  // a failed call: ICP leaves *stats alone, NDT zeroes it
    // NDT, det(H) == 0 (status 1): AlignNdt returns before it assigns result_pose (ndt_registration.cpp:435-436) — the caller's value stays,
    // and the output cloud is transformed by THAT pose (:258)
    if (rc == LOCGPU_OK && !(spec.ndt() && st.status == 1)) std::memcpy(result_pose, pose, sizeof(pose));
    return scan_match_output(ctx, b, n, rc, result_pose, &dst, out_stride_bytes);
}

int locgpu_icp_scan_match(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double init_pose[7], const locgpu_icp_opts* opts,
                          double out_pose[7], locgpu_align_stats* stats, void* out_cloud, size_t out_stride_bytes, locgpu_out_cloud_fn out_fn, void* out_user) {
    AlignSpec spec;
    const int rc = check_icp(ctx, opts, spec);
    return rc != LOCGPU_OK ? rc : scan_match(ctx, spec, "icp_scan_match", src, n, stride_bytes, init_pose, out_pose, stats, out_cloud, out_stride_bytes, out_fn, out_user);
}

int locgpu_ndt_scan_match(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double init_pose[7], double result_pose[7],
                          locgpu_align_stats* stats, void* out_cloud, size_t out_stride_bytes, locgpu_out_cloud_fn out_fn, void* out_user) {
    AlignSpec spec;
    const int rc = check_ndt(ctx, spec);
    return rc != LOCGPU_OK ? rc : scan_match(ctx, spec, "ndt_scan_match", src, n, stride_bytes, init_pose, result_pose, stats, out_cloud, out_stride_bytes, out_fn, out_user);
}

int locgpu_transform_cloud(locgpu_ctx* ctx, const double pose[7], const void* src, size_t n, size_t src_stride_bytes, void* out,
                           size_t out_stride_bytes) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!pose || (n && (!src || !out)) || src_stride_bytes < 12 || out_stride_bytes < 12) return fail(ctx, LOCGPU_ERR_INVALID, "transform_cloud: bad arguments");
    if (n == 0) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    // through the context's one-scan batch: its pinned staging, its source array, its (idle) neighbour-list array — nothing is allocated per call
    locgpu_batch* b = nullptr;
    const int rc = single_batch(ctx, src, n, src_stride_bytes, &b);
    if (rc != LOCGPU_OK) return rc;
    return write_output_cloud(ctx, b, b->d_src, n, pose, out, out_stride_bytes);
}

// --------------------------------------------------------------------------------------------- fitness score, shared-source batches, initial-pose search
}  // extern "C"

namespace {
// The context's own shared-source batch (locgpu_icp_fitness with several poses, locgpu_icp_init_search) is bounded as search_chunks.hpp
// says; its per-entry workspace is neighbour lists 20 B + two work lists 8 B per point and entry.
constexpr size_t kSearchBytesPerPoint = 28;

void drop_graphs(locgpu_batch* b) {
    if (b->graph_exec) { (void)hipGraphExecDestroy(b->graph_exec); b->graph_exec = nullptr; }
    if (b->graph_exec_next) { (void)hipGraphExecDestroy(b->graph_exec_next); b->graph_exec_next = nullptr; }
}

// What the next call uses of a shared-source batch's buffers: n_scans entries (<= cap_scans) of n points (<= cap_points), every entry
// n points long; split_scans as in locgpu_batch. Everything the kernels index goes through n_scans / max_n / pitch, so a smaller
// shape is the same batch as one created at that size.
int reshape_shared(locgpu_ctx* ctx, locgpu_batch* b, int n_scans, size_t n, int split_scans) {
    if (n_scans < 1 || n_scans > b->cap_scans || n == 0 || n > b->cap_points) return fail(ctx, LOCGPU_ERR_INVALID, "shared-source batch: shape exceeds its capacity");
    if (b->n_scans != n_scans || (size_t)b->max_n != n || b->split_scans != split_scans) {
        LOCGPU_HIP(ctx, hipStreamSynchronize(b->stream));
        drop_graphs(b);  // captured launches carry the old shape
        if ((size_t)n_scans * n > b->pitch) {  // the grid search's lists were sized by the old pitch (ensure_grid_lists)
            b->d_grid_qkey.reset();
            b->d_grid_sorted.reset();
        }
        b->n_scans = b->n_total = n_scans;
        b->max_n = (int)n;
        b->blocks_per_scan = (int)((n + kBlock - 1) / kBlock);
        b->pitch = (size_t)n_scans * n;
        b->split_scans = split_scans;
        b->last_iterations = -1;
    }
    b->counts.assign(n_scans, (int)n);
    LOCGPU_HIP(ctx, hipMemcpyAsync(b->d_counts, b->counts.data(), (size_t)n_scans * sizeof(int), hipMemcpyHostToDevice, b->stream));
    return LOCGPU_OK;
}

// The one upload of a shared-source batch: the deep copy of the source (SetSource, icp_registration.cpp:252-265), 16 B per point once.
int upload_shared(locgpu_ctx* ctx, locgpu_batch* b, const void* src, size_t n, size_t stride_bytes) {
    if (!b->h_src) LOCGPU_HIP(ctx, b->h_src.alloc(b->cap_points));
    pack_points((const char*)src, stride_bytes, n, b->h_src);
    LOCGPU_HIP(ctx, hipMemcpyAsync(b->d_src, b->h_src, n * sizeof(float4), hipMemcpyHostToDevice, b->stream));
    return LOCGPU_OK;
}

// The context's shared-source batch with the cloud resident, for m entries in all: *chunk = entries per chunk (equal chunks, the
// last one may be shorter).
int search_batch(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, int m, int* chunk, locgpu_batch** out) {
    *chunk = search_chunk(kSearchBytesPerPoint * n, m);
    locgpu_batch* b = ctx->search;
    if (!b || b->cap_scans < *chunk || b->cap_points < n) {
        // grow-only while the bound holds; else exactly what this call needs
        int cs = std::max(*chunk, b ? b->cap_scans : 0);
        size_t cp = std::max(n, b ? b->cap_points : (size_t)0);
        if ((size_t)cs * cp * kSearchBytesPerPoint > kSearchBytes) { cs = *chunk; cp = n; }
        if (b) { (void)hipStreamSynchronize(b->stream); free_batch(b); ctx->search = nullptr; }
        const int slot = ctx->next_slot;
        const int rc = alloc_batch(ctx, cs, cp, &ctx->search, 0, -1, true);
        ctx->next_slot = slot;  // the context's own batch does not take part in the rotation of the caller's batches over the streams
        if (rc != LOCGPU_OK) return rc;
        b = ctx->search;
        b->slot = 0;
        b->stream = ctx->stream;
        b->pinned = true;
    }
    const int rc = upload_shared(ctx, b, src, n, stride_bytes);
    if (rc != LOCGPU_OK) return rc;
    *out = b;
    return LOCGPU_OK;
}

int fitness_target(locgpu_ctx* ctx) {
    { const int jrc = target_join(ctx); if (jrc != LOCGPU_OK) return jrc; }
    if (!ctx->d_tree) return fail(ctx, LOCGPU_ERR_NO_TARGET, "icp_fitness: SetInputTarget has not been called");
    return refuse_forest(ctx, "icp_fitness");
}

// The NDT score reads the DIRECT table: the incremental voxel set has another table and weights its residuals differently.
int ndt_fitness_target(locgpu_ctx* ctx, const char* who) {
    if (ctx->ndt_opts.method == kNdtOptIncremental) {
        if (!ctx->inc) return fail(ctx, LOCGPU_ERR_NO_TARGET, std::string(who) + ": SetInputTarget has not been called");
        return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": the current NDT target is the incremental one (method 2); the score and the search are defined for the direct target only");
    }
    if (!ctx->ndt) return fail(ctx, LOCGPU_ERR_NO_TARGET, std::string(who) + ": SetInputTarget has not been called");
    return refuse_ndt_set(ctx, who);
}

// One cloud under n_poses > 1 poses, through the context's shared-source batch in chunks (search_chunks.hpp); score(batch, poses, out)
// scores a chunk.
template <class Score>
int ctx_fitness_in_chunks(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double* poses, int n_poses, locgpu_fitness* out, Score score) {
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    locgpu_batch* b = nullptr;
    int chunk = 0;
    const int rc = search_batch(ctx, src, n, stride_bytes, n_poses, &chunk, &b);
    if (rc != LOCGPU_OK) return rc;
    return fitness_in_chunks(n_poses, chunk, [&](int off, int cnt) {
        const int src_rc = reshape_shared(ctx, b, cnt, n, 0);
        return src_rc != LOCGPU_OK ? src_rc : score(b, poses + 7 * (size_t)off, out + off);
    });
}

// The candidate search of either matcher over the context's shared-source batch: every chunk is aligned under `spec` and scored by
// score(batch, poses, out); the driver of search_chunks.hpp picks the winner.
template <class Score>
int ctx_init_search_in_chunks(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double* candidates, int m, const AlignSpec& spec,
                              double min_inlier_ratio, double* out_poses, locgpu_fitness* out_fit, locgpu_align_stats* stats, int* best, Score score) {
    *best = -1;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    locgpu_batch* b = nullptr;
    int chunk = 0;
    const int brc = search_batch(ctx, src, n, stride_bytes, m, &chunk, &b);
    if (brc != LOCGPU_OK) return brc;
    return init_search_in_chunks(m, chunk, min_inlier_ratio, out_fit, 1, best, [&](int off, int cnt) {
        // every chunk sums as the plain batch of all m candidates would: chunking never shows in a pose
        int rc = reshape_shared(ctx, b, cnt, n, m);
        if (rc == LOCGPU_OK) rc = run_align(ctx, b, candidates + 7 * (size_t)off, spec, out_poses + 7 * (size_t)off, stats ? stats + off : nullptr);
        if (rc == LOCGPU_OK) rc = score(b, out_poses + 7 * (size_t)off, out_fit + off);
        return rc;
    });
}
}  // namespace

extern "C" {

int locgpu_batch_create_shared(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, int n_entries, locgpu_batch** out) {
    if (!ctx || !out) return LOCGPU_ERR_INVALID;
    *out = nullptr;
    if (!src || n == 0 || stride_bytes < 12 || n_entries < 1) return fail(ctx, LOCGPU_ERR_INVALID, "batch_create_shared: bad arguments");
    locgpu_batch* b = nullptr;
    int rc = alloc_batch(ctx, n_entries, n, &b, 0, -1, true);
    if (rc != LOCGPU_OK) return rc;
    rc = upload_shared(ctx, b, src, n, stride_bytes);
    if (rc == LOCGPU_OK) rc = reshape_shared(ctx, b, n_entries, n, 0);
    if (rc == LOCGPU_OK && !hip_ok(ctx, hipStreamSynchronize(b->stream), "batch_create_shared: H2D")) rc = LOCGPU_ERR_NO_DEVICE;
    if (rc != LOCGPU_OK) { free_batch(b); return rc; }
    *out = b;
    return LOCGPU_OK;
}

int locgpu_icp_fitness_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, double max_range, locgpu_fitness* out) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    const int rc = fitness_target(ctx);
    if (rc != LOCGPU_OK) return rc;
    if (!b || b->ctx != ctx || !poses || !out || std::isnan(max_range)) return fail(ctx, LOCGPU_ERR_INVALID, "icp_fitness_batch: bad arguments");
    if (b->n_scans < 1) return fail(ctx, LOCGPU_ERR_INVALID, "icp_fitness_batch: the batch holds no scan");
    return fitness_on_batch(ctx, b, poses, max_range, out);
}

int locgpu_icp_fitness(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double* poses, int n_poses, double max_range,
                       locgpu_fitness* out) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    int rc = fitness_target(ctx);
    if (rc != LOCGPU_OK) return rc;
    if (!src || n == 0 || stride_bytes < 12 || !poses || n_poses < 1 || !out || std::isnan(max_range)) return fail(ctx, LOCGPU_ERR_INVALID, "icp_fitness: bad arguments");
    if (n > 0x7FFFFF00u) return fail(ctx, LOCGPU_ERR_INVALID, "icp_fitness: too many points");
    locgpu_batch* b = nullptr;
    if (n_poses == 1) {
        rc = single_batch(ctx, src, n, stride_bytes, &b);
        return rc != LOCGPU_OK ? rc : fitness_on_batch(ctx, b, poses, max_range, out);
    }
    return ctx_fitness_in_chunks(ctx, src, n, stride_bytes, poses, n_poses, out,
                             [&](locgpu_batch* sb, const double* p, locgpu_fitness* o) { return fitness_on_batch(ctx, sb, p, max_range, o); });
}

int locgpu_icp_fitness_resident(locgpu_ctx* ctx, const double pose[7], double max_range, locgpu_fitness* out) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    const int rc = fitness_target(ctx);
    if (rc != LOCGPU_OK) return rc;
    if (!pose || !out || std::isnan(max_range)) return fail(ctx, LOCGPU_ERR_INVALID, "icp_fitness_resident: bad arguments");
    locgpu_batch* b = ctx->single;
    if (!b || b->d_src_ext || b->counts[0] <= 0) return fail(ctx, LOCGPU_ERR_INVALID, "icp_fitness_resident: no source cloud of a single-scan call is resident");
    return fitness_on_batch(ctx, b, pose, max_range, out);
}

void locgpu_init_search_opts_default(locgpu_init_search_opts* o) {
    if (!o) return;
    o->max_range = 1.0;
    o->min_inlier_ratio = 0.5;
}

int locgpu_icp_init_search(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double* candidates, int m, const locgpu_icp_opts* opts,
                           const locgpu_init_search_opts* sopts, double* out_poses, locgpu_fitness* out_fit, locgpu_align_stats* stats, int* best) {
    AlignSpec spec;
    int rc = check_icp(ctx, opts, spec);
    if (rc != LOCGPU_OK) return rc;
    locgpu_init_search_opts so;
    if (sopts) so = *sopts; else locgpu_init_search_opts_default(&so);
    if (!src || n == 0 || stride_bytes < 12 || !candidates || m < 1 || !out_poses || !out_fit || !best || std::isnan(so.max_range) ||
        !(so.min_inlier_ratio >= 0.0))
        return fail(ctx, LOCGPU_ERR_INVALID, "icp_init_search: bad arguments");
    if (n > 0x7FFFFF00u) return fail(ctx, LOCGPU_ERR_INVALID, "icp_init_search: too many points");
    return ctx_init_search_in_chunks(ctx, src, n, stride_bytes, candidates, m, spec, so.min_inlier_ratio, out_poses, out_fit, stats, best,
                                 [&](locgpu_batch* sb, const double* p, locgpu_fitness* o) { return fitness_on_batch(ctx, sb, p, so.max_range, o); });
}

// ---- the same three scores and the search against the direct NDT target (ndt_fitness.hip)
int locgpu_ndt_fitness_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, locgpu_fitness* out) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    const int rc = ndt_fitness_target(ctx, "ndt_fitness_batch");
    if (rc != LOCGPU_OK) return rc;
    if (!b || b->ctx != ctx || !poses || !out) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_fitness_batch: bad arguments");
    if (b->n_scans < 1) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_fitness_batch: the batch holds no scan");
    return ndt_fitness_on_batch(ctx, b, poses, out);
}

int locgpu_ndt_fitness(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double* poses, int n_poses, locgpu_fitness* out) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    int rc = ndt_fitness_target(ctx, "ndt_fitness");
    if (rc != LOCGPU_OK) return rc;
    if (!src || n == 0 || stride_bytes < 12 || !poses || n_poses < 1 || !out) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_fitness: bad arguments");
    if (n > 0x7FFFFF00u) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_fitness: too many points");
    if (n_poses == 1) {
        locgpu_batch* b = nullptr;
        rc = single_batch(ctx, src, n, stride_bytes, &b);
        return rc != LOCGPU_OK ? rc : ndt_fitness_on_batch(ctx, b, poses, out);
    }
    return ctx_fitness_in_chunks(ctx, src, n, stride_bytes, poses, n_poses, out,
                             [&](locgpu_batch* sb, const double* p, locgpu_fitness* o) { return ndt_fitness_on_batch(ctx, sb, p, o); });
}

int locgpu_ndt_fitness_resident(locgpu_ctx* ctx, const double pose[7], locgpu_fitness* out) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    const int rc = ndt_fitness_target(ctx, "ndt_fitness_resident");
    if (rc != LOCGPU_OK) return rc;
    if (!pose || !out) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_fitness_resident: bad arguments");
    locgpu_batch* b = ctx->single;
    if (!b || b->d_src_ext || b->counts[0] <= 0) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_fitness_resident: no source cloud of a single-scan call is resident");
    return ndt_fitness_on_batch(ctx, b, pose, out);
}

int locgpu_ndt_init_search(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double* candidates, int m,
                           const locgpu_init_search_opts* sopts, double* out_poses, locgpu_fitness* out_fit, locgpu_align_stats* stats, int* best) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    int rc = ndt_fitness_target(ctx, "ndt_init_search");
    if (rc != LOCGPU_OK) return rc;
    AlignSpec spec;
    rc = check_ndt(ctx, spec);
    if (rc != LOCGPU_OK) return rc;
    locgpu_init_search_opts so;
    if (sopts) so = *sopts; else locgpu_init_search_opts_default(&so);
    if (!src || n == 0 || stride_bytes < 12 || !candidates || m < 1 || !out_poses || !out_fit || !best || !(so.min_inlier_ratio >= 0.0))
        return fail(ctx, LOCGPU_ERR_INVALID, "ndt_init_search: bad arguments");
    if (n > 0x7FFFFF00u) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_init_search: too many points");
    return ctx_init_search_in_chunks(ctx, src, n, stride_bytes, candidates, m, spec, so.min_inlier_ratio, out_poses, out_fit, stats, best,
                                 [&](locgpu_batch* sb, const double* p, locgpu_fitness* o) { return ndt_fitness_on_batch(ctx, sb, p, o); });
}

int locgpu_pose_grid(const double centre[7], double xy_half, double xy_step, double yaw_half, double yaw_step, double* out, size_t cap, size_t* n_out) {
    if (!centre || !n_out || (cap && !out)) return LOCGPU_ERR_INVALID;
    auto steps = [](double half, double step, long* k) {
        if (!(half >= 0.0) || !std::isfinite(half)) return false;
        if (half == 0.0) { *k = 0; return true; }
        if (!(step > 0.0)) return false;
        const double r = std::floor(half / step + 1e-9);  // 0.15 / 0.05 is 2.9999999999999996 in binary64: the steps that divide the half reach it
        if (r > 1e6) return false;
        *k = (long)r;
        return true;
    };
    long kxy = 0, kyaw = 0;
    if (!steps(xy_half, xy_step, &kxy) || !steps(yaw_half, yaw_step, &kyaw)) return LOCGPU_ERR_INVALID;
    const size_t nxy = (size_t)(2 * kxy + 1), nyaw = (size_t)(2 * kyaw + 1);
    *n_out = nyaw * nxy * nxy;
    double R[9];
    quat_to_R(centre, R);
    size_t w = 0;
    for (long a = -kyaw; a <= kyaw && w < cap; ++a) {
        const double yaw = (double)a * yaw_step, sz = std::sin(0.5 * yaw), cz = std::cos(0.5 * yaw);
        // centre ⊗ (0, 0, sz, cz), Hamilton product in (x, y, z, w) order
        const double q[4] = {centre[0] * cz + centre[1] * sz, centre[1] * cz - centre[0] * sz, centre[2] * cz + centre[3] * sz, centre[3] * cz - centre[2] * sz};
        for (long ix = -kxy; ix <= kxy && w < cap; ++ix)
            for (long iy = -kxy; iy <= kxy && w < cap; ++iy) {
                const double x = (double)ix * xy_step, y = (double)iy * xy_step;
                double* o = out + 7 * w++;
                for (int j = 0; j < 4; ++j) o[j] = q[j];
                for (int r = 0; r < 3; ++r) o[4 + r] = centre[4 + r] + (R[3 * r] * x + R[3 * r + 1] * y);
            }
    }
    return LOCGPU_OK;
}

int locgpu_debug_batch_slot(const locgpu_batch* b) { return b ? b->slot : -1; }

// --------------------------------------------------------------------------------------------- measurement
int locgpu_graph_enable(locgpu_ctx* ctx, int on) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    ctx->use_graph = on != 0;
    return LOCGPU_OK;
}

int locgpu_profile_enable(locgpu_ctx* ctx, int on) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    ctx->profile = on == 2 ? 2 : (on != 0 ? 1 : 0);
    return LOCGPU_OK;
}

int locgpu_profile_read(locgpu_ctx* ctx, double out[6], int reset) {
    if (!ctx || !out) return LOCGPU_ERR_INVALID;
    for (int j = 0; j < 3; ++j) {
        out[j] = ctx->prof_n[j] ? ctx->prof_ms[j] / (double)ctx->prof_n[j] : 0.0;
        out[3 + j] = (double)ctx->prof_n[j];
    }
    if (reset)
        for (int j = 0; j < 3; ++j) { ctx->prof_ms[j] = 0; ctx->prof_n[j] = 0; }
    return LOCGPU_OK;
}

int locgpu_search_stats_read(locgpu_ctx* ctx, uint64_t out[4], int reset) {
    if (!ctx || !out) return LOCGPU_ERR_INVALID;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    if (!ctx->d_search_stats) {
        LOCGPU_HIP(ctx, ctx->d_search_stats.alloc(kSearchStatSlots));
        if (!fill_now(ctx, ctx->d_search_stats, kSearchStatSlots * sizeof(unsigned long long), "hipMemset search stats")) return LOCGPU_ERR_NO_DEVICE;
    }
    for (hipStream_t st : ctx->slot_stream) LOCGPU_HIP(ctx, hipStreamSynchronize(st));
    unsigned long long h[kSearchStatSlots];
    LOCGPU_HIP(ctx, hipMemcpy(h, ctx->d_search_stats, sizeof(h), hipMemcpyDeviceToHost));
    const bool stamp = stamp_build();
    // diagnostic build (LOCGPU_STAMP=1): out[2] = Σ over queries of the main-loop rounds the query needed, out[3] = Σ over queries of
    // the rounds its wave ran (what the wave paid for that lane) — lane efficiency of the search kernel = out[2] / out[3]
    out[0] = h[0]; out[1] = h[1]; out[2] = stamp ? h[4] : h[2]; out[3] = stamp ? h[13] : 0;
    if (stamp && h[12])
        fprintf(stderr, "[locgpu stamp] %llu queries in %llu waves: %.2f rounds per lane, %.2f per wave; lane efficiency %.3f\n", h[0], h[12], (double)h[4] / (double)h[0],
                (double)h[9] / (double)h[12], (double)h[4] / (double)std::max<unsigned long long>(h[13], 1ull));
    if (reset && !fill_now(ctx, ctx->d_search_stats, sizeof(h), "hipMemset search stats")) return LOCGPU_ERR_NO_DEVICE;
    return LOCGPU_OK;
}

int locgpu_visit_count_enable(locgpu_ctx* ctx, int on) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    if (on && !ctx->d_visits) {
        LOCGPU_HIP(ctx, ctx->d_visits.alloc(4));
        if (!fill_now(ctx, ctx->d_visits, 4 * sizeof(unsigned long long), "hipMemset visits")) return LOCGPU_ERR_NO_DEVICE;
    }
    ctx->count_visits = on != 0;
    return LOCGPU_OK;
}

int locgpu_visit_count_read(locgpu_ctx* ctx, uint64_t out[4], int reset) {
    if (!ctx || !out) return LOCGPU_ERR_INVALID;
    out[0] = out[1] = out[2] = out[3] = 0;
    if (!ctx->d_visits) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    for (hipStream_t st : ctx->slot_stream) LOCGPU_HIP(ctx, hipStreamSynchronize(st));
    unsigned long long h[4];
    LOCGPU_HIP(ctx, hipMemcpy(h, ctx->d_visits, sizeof(h), hipMemcpyDeviceToHost));
    out[0] = h[0]; out[1] = h[1]; out[2] = h[2]; out[3] = h[3];
    if (reset && !fill_now(ctx, ctx->d_visits, sizeof(h), "hipMemset visits")) return LOCGPU_ERR_NO_DEVICE;
    return LOCGPU_OK;
}

}  // extern "C"

// Diagnostic build only (LOCGPU_STAMP=1 when the batch was created): per query the main-loop rounds it needed in the batch's most
// recent search stage, out[n_scans * max_n].
extern "C" __attribute__((visibility("default"))) int locgpu_debug_stamp_trips(locgpu_ctx* ctx, locgpu_batch* b, uint32_t* out) {
    if (!ctx || !b || !out || !stamp_build()) return LOCGPU_ERR_INVALID;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    LOCGPU_HIP(ctx, hipStreamSynchronize(b->stream));
    LOCGPU_HIP(ctx, hipMemcpy(out, b->d_redo_list + b->pitch, b->pitch * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return LOCGPU_OK;
}

// Test hook (not part of include/locgpu.h): the device-built exact-search grid of the current target, copied out so the test-suite
// can check its invariants. info = {dims x,y,z, occupied cells, occupied tiles, hash capacity, tile dims x,y,z};
// params = {origin x,y,z, cell, inv_cell, slack}; pts: n × 4 floats (x, y, z, bits(leaf slot)) in (tile, cell) order; tiles: the raw
// 140-byte TileRec records; hash: {tile_lin, record} × capacity. Returns the number of grid points (0 on failure).
extern "C" __attribute__((visibility("default"))) size_t locgpu_debug_grid_dump(locgpu_ctx* ctx, int64_t info[9], float params[6], float* pts, size_t pts_cap,
                                                                                 void* tiles, size_t tiles_cap_bytes, uint32_t* hash, size_t hash_cap) {
    if (!ctx || target_join(ctx) != LOCGPU_OK || !ctx->d_tree || ensure_grid(ctx) != LOCGPU_OK) return 0;
    const locgpu::GridView& g = ctx->grid;
    if (info) {
        for (int a = 0; a < 3; ++a) { info[a] = g.dims[a]; info[6 + a] = g.tdims[a]; }
        info[3] = (int64_t)g.num_cells; info[4] = g.n_tocc; info[5] = (int64_t)g.tile_mask + 1;
    }
    if (params) { for (int a = 0; a < 3; ++a) params[a] = g.origin[a]; params[3] = g.cell; params[4] = g.inv_cell; params[5] = g.slack; }
    if (pts && hipMemcpy(pts, g.pts, std::min(pts_cap, g.num_points * 4) * sizeof(float), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    if (tiles && hipMemcpy(tiles, g.tiles, std::min(tiles_cap_bytes, (size_t)g.n_tocc * sizeof(locgpu::TileRec)), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    if (hash && hipMemcpy(hash, g.tile_hash, std::min(hash_cap, ((size_t)g.tile_mask + 1) * 2) * sizeof(uint32_t), hipMemcpyDeviceToHost) != hipSuccess) return 0;
    return g.num_points;
}

// --------------------------------------------------------------------------------------------- NDT
namespace locgpu {
// the context's direct table, an ordinary target's or a voxel set's, and what it knows about a set
static void ndt_drop_direct(locgpu_ctx* ctx) {
    delete ctx->ndt;
    ctx->ndt = nullptr;
    ctx->ndt_set_n = 0;
    ctx->ndt_set_points.clear(); ctx->ndt_set_voxels.clear(); ctx->ndt_set_first.clear();
}
void ndt_free(locgpu_ctx* ctx) {
    ndt_drop_direct(ctx);
    if (ctx->inc) { inc_ndt_destroy(ctx->inc); ctx->inc = nullptr; }
}
int refuse_ndt_set(locgpu_ctx* ctx, const char* who) {
    if (ctx->ndt_set_n == 0) return LOCGPU_OK;
    return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": the context holds a voxel-set target (locgpu_ndt_set_target_set), which only locgpu_ndt_align_pairs / "
                                         "locgpu_ndt_fitness_pairs read; locgpu_ndt_set_target* makes it an ordinary target again");
}
int check_ndt(locgpu_ctx* ctx, AlignSpec& spec, bool pairs) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    const bool inc = ctx->ndt_opts.method == kNdtOptIncremental;
    if ((inc && !ctx->inc) || (!inc && !ctx->ndt)) return fail(ctx, LOCGPU_ERR_NO_TARGET, "ndt: SetInputTarget has not been called");
    if (!pairs) { const int src = refuse_ndt_set(ctx, "ndt"); if (src != LOCGPU_OK) return src; }
    if (pairs && ctx->ndt_set_n == 0)
        return fail(ctx, LOCGPU_ERR_INVALID, "ndt_align_pairs: the context holds an ordinary target; the pairs calls read a voxel-set target (locgpu_ndt_set_target_set)");
    spec = AlignSpec{};
    spec.pairs = pairs;
    GnParams& prm = spec.prm;
    prm.method = inc ? kMethodNdtInc : kMethodNdtDirect;
    prm.max_iteration = ctx->ndt_opts.max_iteration;
    prm.min_effective_pts = ctx->ndt_opts.min_effective_pts;
    prm.eps = ctx->ndt_opts.eps;
    prm.max_nn_distance = prm.max_plane_distance = prm.max_line_distance = 0.0;
    return LOCGPU_OK;
}
}  // namespace locgpu

extern "C" {

// Target ingest from a cloud already in HBM. `host` (optional) = the same points on the host: the incremental method replays a
// cloud whose own working set exceeds the voxel capacity point by point there (ndt_inc.hip) and fetches them when absent.
static int ndt_set_target_dev(locgpu_ctx* ctx, const float4* d_pts, const float4* host, size_t n, const locgpu_ndt_opts* opts) {
    locgpu_ndt_opts o;
    if (opts) o = *opts; else locgpu_ndt_opts_default(&o);
    if (!(o.voxel_size > 0.0) || (o.nearby_type != kNearbyCenter && o.nearby_type != kNearby6) || (o.method != kNdtOptDirect && o.method != kNdtOptIncremental) ||
        (o.method == kNdtOptIncremental && o.capacity < 2))
        return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_target: bad options");
    if (ctx->ndt_set_n > 0) ndt_drop_direct(ctx);  // a voxel set is replaced: the context is an ordinary one again, whatever becomes of this ingest
    if (o.method == kNdtOptIncremental) {
        // incremental: keep the voxel set unless the grid itself changed
        if (ctx->inc && (ctx->ndt_opts.method != kNdtOptIncremental || ctx->ndt_opts.voxel_size != o.voxel_size || ctx->ndt_opts.capacity != o.capacity)) {
            inc_ndt_destroy(ctx->inc);
            ctx->inc = nullptr;
        }
        if (!ctx->inc) ctx->inc = inc_ndt_create((size_t)o.capacity, o.voxel_size);
        bool bad = false;
        const hipError_t e = inc_ndt_ingest(*ctx->inc, host, d_pts, n, ctx->stream, &bad);
        if (e != hipSuccess) {
            // an ingest that failed half way (its counters, slot arrays, free stack and table may disagree): the voxel set is gone,
            // the next SetInputTarget starts from an empty one
            (void)hipStreamSynchronize(ctx->stream);
            inc_ndt_destroy(ctx->inc);
            ctx->inc = nullptr;
            hip_ok(ctx, e, "inc_ndt_ingest");
            return LOCGPU_ERR_NO_DEVICE;
        }
        ctx->ndt_opts = o;
        ctx->target_epoch++;
        if (bad) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_target: a point lies outside the +-2^20-voxel key range (it was skipped)");
        return LOCGPU_OK;
    }
    if (ctx->inc) { inc_ndt_destroy(ctx->inc); ctx->inc = nullptr; }
    if (!ctx->ndt) ctx->ndt = new NdtTable();
    bool bad_key = false;
    const hipError_t e = ndt_build(*ctx->ndt, d_pts, n, o.voxel_size, o.min_pts_in_voxel, ctx->stream, &bad_key);
    if (e != hipSuccess) { ndt_free(ctx); hip_ok(ctx, e, "ndt_build"); return LOCGPU_ERR_NO_DEVICE; }
    if (bad_key) { ndt_free(ctx); return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_target: a point lies outside the +-2^20-voxel key range"); }
    ctx->ndt->res_outlier_th = o.res_outlier_th;
    ctx->ndt->n_nearby = ndt_n_nearby(o.nearby_type);
    ctx->ndt_opts = o;
    ctx->target_epoch++;
    return LOCGPU_OK;
}

int locgpu_ndt_set_target(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes, const locgpu_ndt_opts* opts) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!pts || n == 0 || stride_bytes < 12) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_target: empty cloud or stride < 12");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<float4> host(n);
    const char* base = (const char*)pts;
    for (size_t i = 0; i < n; ++i) { host[i] = float4{0.f, 0.f, 0.f, 0.f}; std::memcpy(&host[i], base + i * stride_bytes, 12); }
    DevBuf<float4> d_pts;
    LOCGPU_HIP(ctx, d_pts.alloc(n));
    if (!hip_ok(ctx, hipMemcpy(d_pts, host.data(), n * sizeof(float4), hipMemcpyHostToDevice), "H2D map")) return LOCGPU_ERR_NO_DEVICE;
    const int rc = ndt_set_target_dev(ctx, d_pts, host.data(), n, opts);
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

int locgpu_ndt_target_info(const locgpu_ctx* ctx, int64_t out[3]) {
    if (!ctx || !out) return LOCGPU_ERR_INVALID;
    if (ctx->ndt_opts.method == kNdtOptIncremental && ctx->inc) { out[0] = (int64_t)inc_ndt_num_voxels(ctx->inc); out[1] = ctx->ndt_opts.capacity; out[2] = 0; return LOCGPU_OK; }
    if (!ctx->ndt) { out[0] = out[1] = out[2] = 0; return LOCGPU_ERR_NO_TARGET; }
    out[0] = (int64_t)ctx->ndt->n_vox;
    out[1] = (int64_t)ctx->ndt->cap;
    out[2] = (int64_t)(ctx->ndt->cap * sizeof(NdtSlot) + ctx->ndt->n_vox * sizeof(NdtRecord));
    return LOCGPU_OK;
}

int locgpu_ndt_dump(locgpu_ctx* ctx, int32_t* keys, double* mu, double* info, size_t cap, size_t* n_out) {
    if (!ctx || !n_out) return LOCGPU_ERR_INVALID;
    if (ctx->ndt_opts.method == kNdtOptIncremental && ctx->inc) {
        LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
        LOCGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
        *n_out = inc_ndt_dump(ctx->inc, keys, mu, info, cap);
        return LOCGPU_OK;
    }
    if (!ctx->ndt) return fail(ctx, LOCGPU_ERR_NO_TARGET, "ndt_dump: no target");
    { const int src = refuse_ndt_set(ctx, "ndt_dump"); if (src != LOCGPU_OK) return src; }
    *n_out = ctx->ndt->n_vox;
    const size_t n = std::min(cap, ctx->ndt->n_vox);
    if (n == 0) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    LOCGPU_HIP(ctx, ndt_dump(*ctx->ndt, keys, mu, info, n, ctx->stream));
    return LOCGPU_OK;
}

int locgpu_debug_ndt_slots(locgpu_ctx* ctx, uint64_t* keys, int32_t* vid, size_t cap, size_t* n_slots) {
    if (!ctx || !n_slots) return LOCGPU_ERR_INVALID;
    if (ctx->ndt_opts.method == kNdtOptIncremental && ctx->inc) {
        *n_slots = inc_ndt_table_size(ctx->inc);
        if ((!keys && !vid) || cap == 0 || *n_slots == 0) return LOCGPU_OK;
        LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
        LOCGPU_HIP(ctx, inc_ndt_slots_read(ctx->inc, keys, vid, cap, ctx->stream));
        return LOCGPU_OK;
    }
    if (!ctx->ndt) return fail(ctx, LOCGPU_ERR_NO_TARGET, "debug_ndt_slots: no NDT target");
    *n_slots = ctx->ndt->cap;
    if ((!keys && !vid) || cap == 0) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    LOCGPU_HIP(ctx, ndt_slots_read(*ctx->ndt, keys, vid, cap, ctx->stream));
    return LOCGPU_OK;
}

int locgpu_ndt_align_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* init_poses, double* out_poses, locgpu_align_stats* stats) {
    AlignSpec spec;
    int rc = check_ndt(ctx, spec);
    if (rc == LOCGPU_OK) rc = check_batch(ctx, b, init_poses && out_poses, spec, "ndt_align_batch");
    return rc != LOCGPU_OK ? rc : run_align(ctx, b, init_poses, spec, out_poses, stats);
}

int locgpu_ndt_align_batch_begin(locgpu_ctx* ctx, locgpu_batch* b, const double* init_poses) {
    AlignSpec spec;
    int rc = check_ndt(ctx, spec);
    if (rc == LOCGPU_OK) rc = check_batch(ctx, b, init_poses != nullptr, spec, "ndt_align_batch_begin");
    return rc != LOCGPU_OK ? rc : align_begin(ctx, b, init_poses, spec);
}

int locgpu_ndt_align(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double init_pose[7], double out_pose[7],
                     locgpu_align_stats* stats) {
    AlignSpec spec;
    const int rc = check_ndt(ctx, spec);
    return rc != LOCGPU_OK ? rc : align_single(ctx, spec, "ndt_align", src && init_pose && out_pose, src, n, stride_bytes, nullptr, init_pose, out_pose, stats);
}

int locgpu_ndt_hb_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, double* hb) {
    AlignSpec spec;
    int rc = check_ndt(ctx, spec);
    if (rc == LOCGPU_OK) rc = check_batch(ctx, b, poses && hb, spec, "ndt_hb_batch");
    return rc != LOCGPU_OK ? rc : eval_hb_batch(ctx, b, poses, spec, hb, "ndt_hb_batch");
}

int locgpu_ndt_hb(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double pose[7], double H[36], double B[6], int64_t* effective_num,
                  int* ok) {
    AlignSpec spec;
    int rc = check_ndt(ctx, spec);
    if (rc != LOCGPU_OK) return rc;
    if (!src || !pose || !H || !B) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_hb: bad arguments");
    locgpu_batch* b = nullptr;
    rc = single_batch(ctx, src, n, stride_bytes, &b);
    if (rc != LOCGPU_OK) return rc;
    double hb[44];
    rc = eval_hb_batch(ctx, b, pose, spec, hb, "ndt_hb");
    if (rc != LOCGPU_OK) return rc;
    std::memcpy(H, hb, 36 * sizeof(double));
    std::memcpy(B, hb + 36, 6 * sizeof(double));
    if (effective_num) *effective_num = (int64_t)hb[42];
    if (ok) *ok = hb[43] != 0.0;
    return LOCGPU_OK;
}

// ---- matcher entry points on clouds resident in HBM (cloud_filters.hpp) ----
int locgpu_ndt_set_target_cloud(locgpu_ctx* ctx, const locgpu_cloud* target, const locgpu_ndt_opts* opts) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!target || target->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_target_cloud: bad cloud");
    if (target->n == 0) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_target: empty cloud or stride < 12");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = ndt_set_target_dev(ctx, target->d, nullptr, target->n, opts);
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

int locgpu_icp_align_cloud(locgpu_ctx* ctx, const locgpu_cloud* src, const double init_pose[7], const locgpu_icp_opts* opts, double out_pose[7],
                           locgpu_align_stats* stats) {
    AlignSpec spec;
    const int rc = check_icp(ctx, opts, spec);
    return rc != LOCGPU_OK ? rc : align_single(ctx, spec, "icp_align_cloud", src && src->ctx && init_pose && out_pose, nullptr, 0, 0, src, init_pose, out_pose, stats);
}

int locgpu_ndt_align_cloud(locgpu_ctx* ctx, const locgpu_cloud* src, const double init_pose[7], double out_pose[7], locgpu_align_stats* stats) {
    AlignSpec spec;
    const int rc = check_ndt(ctx, spec);
    return rc != LOCGPU_OK ? rc : align_single(ctx, spec, "ndt_align_cloud", src && src->ctx && init_pose && out_pose, nullptr, 0, 0, src, init_pose, out_pose, stats);
}

// ---- pairwise batch NDT: a voxel-set target and the pairs calls (ndt_pairs.hip) ----
// The set's options: what locgpu_ndt_set_target accepts, the direct method only.
static int ndt_set_opts(locgpu_ctx* ctx, const locgpu_ndt_opts* opts, const char* who, locgpu_ndt_opts& o) {
    if (opts) o = *opts; else locgpu_ndt_opts_default(&o);
    if (!(o.voxel_size > 0.0) || (o.nearby_type != kNearbyCenter && o.nearby_type != kNearby6) || (o.method != kNdtOptDirect && o.method != kNdtOptIncremental))
        return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": bad options");
    if (o.method == kNdtOptIncremental) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": a voxel set is built by the direct method only (method 1); the incremental method is refused");
    return LOCGPU_OK;
}

// Build from points on the device (ndt_set_build's layouts) into a local table; the context is touched only when all of it succeeded.
static int ndt_install_set(locgpu_ctx* ctx, const float4* d_pts, size_t scan_stride, const std::vector<int>& counts, const locgpu_ndt_opts& o, const char* who) {
    const int n_targets = (int)counts.size();
    NdtTable t;
    std::vector<NdtSetTarget> info;
    int bad = -1;
    const hipError_t e = ndt_set_build(t, d_pts, scan_stride, counts.data(), n_targets, o.voxel_size, o.min_pts_in_voxel, ctx->stream, info, &bad);
    if (e == hipErrorInvalidValue) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": the set is beyond its size limits (points of all targets, or scans x capacity of the batch)");
    if (e != hipSuccess) { (void)hipStreamSynchronize(ctx->stream); hip_ok(ctx, e, "ndt_set_build"); return LOCGPU_ERR_NO_DEVICE; }
    if (bad >= 0)
        return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": target " + std::to_string(bad) + ": a point lies outside the +-2^15-voxel key range of a voxel set");
    t.res_outlier_th = o.res_outlier_th;
    t.n_nearby = ndt_n_nearby(o.nearby_type);
    if (ctx->inc) { inc_ndt_destroy(ctx->inc); ctx->inc = nullptr; }
    if (!ctx->ndt) ctx->ndt = new NdtTable();
    *ctx->ndt = std::move(t);
    ctx->ndt_set_n = n_targets;
    ctx->ndt_set_points.assign((size_t)n_targets, 0); ctx->ndt_set_voxels.assign((size_t)n_targets, 0); ctx->ndt_set_first.assign((size_t)n_targets, 0);
    size_t first = 0;
    for (int j = 0; j < n_targets; ++j) {
        ctx->ndt_set_points[j] = (size_t)info[j].points;
        ctx->ndt_set_voxels[j] = (size_t)info[j].voxels;
        ctx->ndt_set_first[j] = first;  // records are numbered in (target, key) order
        first += (size_t)info[j].voxels;
    }
    ctx->ndt_opts = o;
    ctx->target_epoch++;
    return LOCGPU_OK;
}

int locgpu_ndt_set_target_set(locgpu_ctx* ctx, const void* const* pts, const size_t* n, int n_targets, size_t stride_bytes, const locgpu_ndt_opts* opts) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    std::string err;
    if (!ndt_set_check_targets(pts, n, n_targets, stride_bytes, err)) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_target_set: " + err);
    locgpu_ndt_opts o;
    { const int orc = ndt_set_opts(ctx, opts, "ndt_set_target_set", o); if (orc != LOCGPU_OK) return orc; }
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    std::vector<int> counts((size_t)n_targets);
    size_t total = 0;
    for (int j = 0; j < n_targets; ++j) { counts[j] = (int)n[j]; total += n[j]; }
    // the deep copy of SetInputTarget: all targets behind one another in the context's pinned staging block, one copy up
    float4* stage = nullptr;
    if (!hip_ok(ctx, cloud_stage(ctx, total, &stage), "pinned staging")) return LOCGPU_ERR_OOM;
    size_t w = 0;
    for (int j = 0; j < n_targets; ++j) {
        const char* base = (const char*)pts[j];
        for (size_t i = 0; i < n[j]; ++i, ++w) { stage[w] = float4{0.f, 0.f, 0.f, 0.f}; std::memcpy(&stage[w], base + i * stride_bytes, 12); }
    }
    DevBuf<float4> d_pts;
    if (!hip_ok(ctx, d_pts.alloc(total), "hipMalloc voxel-set points")) return LOCGPU_ERR_OOM;
    LOCGPU_HIP(ctx, hipMemcpyAsync(d_pts, stage, total * sizeof(float4), hipMemcpyHostToDevice, ctx->stream));
    const int rc = ndt_install_set(ctx, d_pts, 0, counts, o, "ndt_set_target_set");
    (void)hipStreamSynchronize(ctx->stream);  // the staging block and d_pts are free again
    return rc;
}

int locgpu_ndt_set_target_set_batch(locgpu_ctx* ctx, const locgpu_batch* b, const locgpu_ndt_opts* opts) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!b || b->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_target_set_batch: NULL batch or a batch of another context");
    if (b->sharded || b->shared_src) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_target_set_batch: sharded and shared-source batches hold no scans of their own");
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_target_set_batch: an alignment of this batch has been begun and not finished");
    if (b->n_scans < 1 || b->n_scans > kNdtSetMaxTargets)
        return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_target_set_batch: the batch holds " + std::to_string(b->n_scans) + " scans, a voxel set 1 ... " + std::to_string(kNdtSetMaxTargets) + " targets");
    locgpu_ndt_opts o;
    { const int orc = ndt_set_opts(ctx, opts, "ndt_set_target_set_batch", o); if (orc != LOCGPU_OK) return orc; }
    std::vector<int> counts((size_t)b->n_scans);
    for (int j = 0; j < b->n_scans; ++j) {
        if (b->counts[j] <= 0) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_target_set_batch: target " + std::to_string(j) + ": empty cloud");
        counts[j] = b->counts[j];
    }
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    { const int orc = order_behind_batch(ctx, const_cast<locgpu_batch*>(b), "ndt_set_target_set_batch: ordering behind the batch"); if (orc != LOCGPU_OK) return orc; }
    // the scans are read where the batch holds them: no point crosses PCIe
    const int rc = ndt_install_set(ctx, b->d_src, (size_t)b->max_n, counts, o, "ndt_set_target_set_batch");
    (void)hipStreamSynchronize(ctx->stream);
    return rc;
}

int locgpu_ndt_set_info(const locgpu_ctx* ctx, int* n_targets, size_t* points, size_t* voxels) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (n_targets) *n_targets = ctx->ndt_set_n;
    locgpu_ctx* c = const_cast<locgpu_ctx*>(ctx);
    if (ctx->ndt_set_n == 0) {
        const bool any = ctx->ndt_opts.method == kNdtOptIncremental ? ctx->inc != nullptr : ctx->ndt != nullptr;
        return any ? fail(c, LOCGPU_ERR_INVALID, "ndt_set_info: the context holds an ordinary NDT target") : fail(c, LOCGPU_ERR_NO_TARGET, "ndt_set_info: SetInputTarget has not been called");
    }
    for (int j = 0; j < ctx->ndt_set_n; ++j) {
        if (points) points[j] = ctx->ndt_set_points[j];
        if (voxels) voxels[j] = ctx->ndt_set_voxels[j];
    }
    return LOCGPU_OK;
}

int locgpu_ndt_set_dump(locgpu_ctx* ctx, int target, int32_t* keys, double* mu, double* info, size_t cap, size_t* n_out) {
    if (!ctx || !n_out) return LOCGPU_ERR_INVALID;
    if (ctx->ndt_set_n == 0 || !ctx->ndt) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_dump: the context holds no voxel-set target");
    if (target < 0 || target >= ctx->ndt_set_n) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_set_dump: target " + std::to_string(target) + " is not one of the " + std::to_string(ctx->ndt_set_n) + " targets");
    *n_out = ctx->ndt_set_voxels[(size_t)target];
    const size_t n = std::min(cap, *n_out);
    if (n == 0) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    LOCGPU_HIP(ctx, ndt_set_dump(*ctx->ndt, ctx->ndt_set_first[(size_t)target], n, keys, mu, info, ctx->stream));
    return LOCGPU_OK;
}

int locgpu_ndt_align_pairs(locgpu_ctx* ctx, locgpu_batch* b, const int* target_of, const double* init_poses, double* out_poses, locgpu_align_stats* stats) {
    AlignSpec spec;
    int rc = check_ndt(ctx, spec, true);
    if (rc == LOCGPU_OK) rc = check_pairs(ctx, b, target_of, out_poses != nullptr, "ndt_align_pairs", ctx->ndt_set_n, nullptr);
    if (rc != LOCGPU_OK) return rc;
    std::vector<double> identity;
    if (!init_poses) {  // the reference's `SE3 init_pos` of every scan-to-scan match (test_node.cpp:348)
        identity.assign(7 * (size_t)b->n_total, 0.0);
        for (int i = 0; i < b->n_total; ++i) identity[7 * (size_t)i + 3] = 1.0;
        init_poses = identity.data();
    }
    return run_align(ctx, b, init_poses, spec, out_poses, stats);
}

int locgpu_ndt_fitness_pairs(locgpu_ctx* ctx, locgpu_batch* b, const int* target_of, const double* poses, locgpu_fitness* out) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (ctx->ndt_opts.method == kNdtOptIncremental ? !ctx->inc : !ctx->ndt) return fail(ctx, LOCGPU_ERR_NO_TARGET, "ndt_fitness_pairs: SetInputTarget has not been called");
    if (ctx->ndt_set_n == 0)
        return fail(ctx, LOCGPU_ERR_INVALID, "ndt_fitness_pairs: the context holds an ordinary target; the pairs calls read a voxel-set target (locgpu_ndt_set_target_set)");
    const int rc = check_pairs(ctx, b, target_of, poses && out, "ndt_fitness_pairs", ctx->ndt_set_n, nullptr);
    return rc != LOCGPU_OK ? rc : ndt_fitness_pairs_on_batch(ctx, b, poses, out);
}

}  // extern "C"
