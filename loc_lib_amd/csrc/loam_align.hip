// loc_lib_amd/csrc/loam_align.hip — the LOAM matcher (LoamRegistration, loam_registration.cpp:22-99) behind locgpu_loam_*.
//
// A locgpu_loam owns what one LoamRegistration owns: a surface matcher (P2Plane) and an edge matcher (P2Line), here two locgpu_ctx on
// one device, each with one storage batch for its feature scans, and the JOINT alignment state: one PoseState per scan that both
// classes' local stages read and loam_solve_kernel (icp_fit.hip) writes. One Gauss–Newton iteration is, on ONE stream,
//     launch_local_stage(surface) → launch_local_stage(edge) → loam_solve_kernel
// in eager chunks of kFirstChunk / kNextChunk iterations between two host reads of the flags, later chunks over the open scans only —
// the chunks of align_begin / align_finish (gn_driver.hip) without graphs, shards, pools or host pacing.
// The _cloud entry points run the same loop on feature clouds that are already in HBM (the batches' d_src_ext, as single_batch_dev of
// locgpu_api.hip does) and write the output cloud on the device (loam_stream.hip).
// The joint score and the candidate search (locgpu_loam_fitness*, locgpu_loam_init_search*) give the storage batches their third,
// shared-source form — every entry of a class reads the ONE pair of scans — and go through the chunk driver of search_chunks.hpp.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "batch_upload.hpp"
#include "cloud_filters.hpp"
#include "context.hpp"
#include "gn_driver.hpp"
#include "launch.hpp"
#include "search_chunks.hpp"

using namespace locgpu;

namespace {
constexpr int kSurf = 0, kEdge = 1;  // the order the reference evaluates them in (loam_registration.cpp:53-71)
}

struct locgpu_loam {
    int device = 0;
    locgpu_loam_opts opts{};
    bool use[2] = {false, false};
    locgpu_ctx* ctx[2] = {nullptr, nullptr};
    bool borrowed = false;  // locgpu_loam_create_on: the contexts, their targets and their lifetime are the caller's
    locgpu_batch* batch[2] = {nullptr, nullptr};  // storage batches: kept between calls, grow-only, reshaped to the call's scans
    bool has_target[2] = {false, false};
    bool resident = false;  // the storage batches hold (or, after a _cloud call, point at) the scans of a single-scan call: locgpu_loam_fitness_resident
    hipStream_t stream = nullptr;  // the first enabled class's context stream: every launch of an alignment
    Event ev;                      // orders `stream` behind the other context's stream
    // joint state; h_fit, grown last, has the capacity of all eight
    DevBuf<PoseState> d_state;
    PinnedBuf<PoseState> h_state;
    DevBuf<double> d_hb;
    PinnedBuf<double> h_hb;
    DevBuf<int> d_active;
    PinnedBuf<int> h_active;
    DevBuf<double> d_fit;          // [scans][3][kFitW]: the joint score's sums — joint, surface, edge
    PinnedBuf<double> h_fit;
    // Shared-source form of the storage batches (share_scans): every entry of class c reads ONE region of n_shared[c] points — the
    // batch's own d_src, filled once through h_shared[c], or a caller's cloud through d_src_ext. src_of[c] / split_scans are what run()
    // hands to LocalStage::src_of / split_scans: nullptr / 0 in the two other forms (upload_scans, attach_scans).
    DevBuf<int> d_src_of[2];        // a zero per entry
    PinnedBuf<float4> h_shared[2];  // pinned staging of a host scan
    size_t n_shared[2] = {0, 0};
    const int* src_of[2] = {nullptr, nullptr};
    int split_scans = 0;
    // output cloud of scan_match: packed x, y, z of edge then surface points; the points of a switched-off class pass through d_off
    DevBuf<float> d_xyz;
    PinnedBuf<float> h_xyz;
    DevBuf<float4> d_off;
    PinnedBuf<float4> h_off;
    std::string err;
};

namespace {

std::string g_loam_create_err;

int lfail(locgpu_loam* l, int code, const std::string& msg) {
    if (l) l->err = msg;
    else g_loam_create_err = msg;
    return code;
}
// a failure inside one of the two contexts: its text becomes the handle's
int from_ctx(locgpu_loam* l, int c, int rc) {
    if (rc != LOCGPU_OK) l->err = std::string(c == kSurf ? "surface: " : "edge: ") + locgpu_last_error(l->ctx[c]);
    return rc;
}
bool lhip(locgpu_loam* l, hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    lfail(l, LOCGPU_ERR_NO_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
    return false;
}
#define LOAM_HIP(l, expr)                                         \
    do {                                                          \
        if (!lhip((l), (expr), #expr)) return LOCGPU_ERR_NO_DEVICE; \
    } while (0)

const locgpu_icp_opts& class_opts(const locgpu_loam* l, int c) { return c == kSurf ? l->opts.surf : l->opts.edge; }

int check_opts(const locgpu_loam_opts* o) {
    if (!o) return lfail(nullptr, LOCGPU_ERR_INVALID, "loam_create: opts is NULL");
    if (!o->use_surf_points && !o->use_edge_points) return lfail(nullptr, LOCGPU_ERR_INVALID, "loam_create: both feature classes are switched off");
    const locgpu_icp_opts* cls[2] = {&o->surf, &o->edge};
    const int32_t use[2] = {o->use_surf_points, o->use_edge_points};
    for (int c = 0; c < 2; ++c) {
        if (!use[c]) continue;
        if (cls[c]->method == LOCGPU_P2PLANE_MAP) return lfail(nullptr, LOCGPU_ERR_INVALID, "loam_create: LOCGPU_P2PLANE_MAP is not available in the LOAM matcher");
        if (cls[c]->method < LOCGPU_P2P || cls[c]->method > LOCGPU_P2PLANE) return lfail(nullptr, LOCGPU_ERR_INVALID, "loam_create: unknown method");
        if (cls[c]->search_mode != LOCGPU_SEARCH_TREE_FAITHFUL && cls[c]->search_mode != LOCGPU_SEARCH_GRID_EXACT)
            return lfail(nullptr, LOCGPU_ERR_INVALID, "loam_create: unknown search mode");
    }
    return LOCGPU_OK;
}

int reserve_joint(locgpu_loam* l, int n) {
    if ((size_t)n * 3 * kFitW <= l->h_fit.cap()) return LOCGPU_OK;
    const bool ok = lhip(l, l->d_state.alloc((size_t)n), "hipMalloc state") &&
                    lhip(l, l->h_state.alloc((size_t)n), "hipHostMalloc state") &&
                    lhip(l, l->d_hb.alloc((size_t)n * kLoamHbW), "hipMalloc hb") &&
                    lhip(l, l->h_hb.alloc((size_t)n * kLoamHbW), "hipHostMalloc hb") &&
                    lhip(l, l->d_active.alloc((size_t)n), "hipMalloc active") &&
                    lhip(l, l->h_active.alloc((size_t)n), "hipHostMalloc active") &&
                    lhip(l, l->d_fit.alloc((size_t)n * 3 * kFitW), "hipMalloc fit") &&
                    lhip(l, l->h_fit.alloc((size_t)n * 3 * kFitW), "hipHostMalloc fit");
    return ok ? LOCGPU_OK : LOCGPU_ERR_OOM;
}

// Class c's storage batch shaped as n_scans scans of at most max_n points: the one of the previous call when it has the room
// (cap_scans × cap_points — everything the kernels index goes through n_scans / max_n / pitch, so a smaller shape is the same batch as
// one created at that size), a larger one otherwise. A one-scan call gets headroom in points, as a per-scan caller's clouds vary.
int shape_batch(locgpu_loam* l, int c, int n_scans, size_t max_n) {
    locgpu_ctx* ctx = l->ctx[c];
    locgpu_batch* b = l->batch[c];
    max_n = std::max<size_t>(max_n, 1);
    if (!b || b->cap_scans < n_scans || b->cap_points < max_n) {
        const int cs = std::max(n_scans, b ? b->cap_scans : 0);
        size_t cp = std::max(max_n, b ? b->cap_points : (size_t)0);
        if (cp == max_n && n_scans == 1) cp = with_headroom(max_n);
        if (b) { (void)hipStreamSynchronize(l->stream); free_batch(b); l->batch[c] = nullptr; }
        const int slot = ctx->next_slot;
        int rc = from_ctx(l, c, alloc_batch(ctx, cs, cp, &l->batch[c]));
        ctx->next_slot = slot;  // the handle's storage does not take part in the rotation of a (borrowed) context's batches over its streams
        if (rc != LOCGPU_OK) return rc;
        b = l->batch[c];
        b->slot = 0;
        b->stream = ctx->stream;
        b->pinned = true;
        // the uploader's pinned counts are sized by the batch's scans at its first upload: give it the capacity's worth now
        if (!lhip(l, b->upl.h_counts.alloc((size_t)cs), "hipHostMalloc counts")) return LOCGPU_ERR_OOM;
    }
    if (b->n_scans != n_scans || (size_t)b->max_n != max_n) {
        if ((size_t)n_scans * max_n > b->pitch) {  // the grid search's lists were sized by the old pitch (ensure_grid_lists)
            b->d_grid_qkey.reset();
            b->d_grid_sorted.reset();
        }
        b->n_scans = b->n_total = n_scans;
        b->max_n = (int)max_n;
        b->blocks_per_scan = (int)((max_n + kBlock - 1) / kBlock);
        b->pitch = (size_t)n_scans * max_n;
        b->counts.assign(n_scans, 0);
    }
    return LOCGPU_OK;
}

// The deep copy of the feature scans (SetSource, icp_registration.cpp:252-265) into both classes' storage batches; `stream` is ordered
// behind the copies and behind whatever either context's own stream still runs (its target ingest).
int upload_scans(locgpu_loam* l, int n_scans, const void* const* srcs[2], const size_t* counts[2], size_t stride) {
    size_t max_n[2] = {0, 0};
    l->src_of[kSurf] = l->src_of[kEdge] = nullptr;  // every scan reads its own region, and the sums split by this call's shape
    l->split_scans = 0;
    for (int c = 0; c < 2; ++c) {  // every argument is checked before the first copy starts: a refused call reads nothing
        if (!l->use[c]) continue;
        if (!srcs[c] || !counts[c]) return lfail(l, LOCGPU_ERR_INVALID, "loam: the scans of an enabled feature class are NULL");
        for (int i = 0; i < n_scans; ++i) {
            if (counts[c][i] && !srcs[c][i]) return lfail(l, LOCGPU_ERR_INVALID, "loam: NULL scan pointer");
            if (counts[c][i] > 0x7FFFFF00u) return lfail(l, LOCGPU_ERR_INVALID, "loam: too many points in a scan");
            max_n[c] = std::max(max_n[c], counts[c][i]);
        }
    }
    int rc = LOCGPU_OK;
    bool started[2] = {false, false};
    for (int c = 0; c < 2 && rc == LOCGPU_OK; ++c) {
        if (!l->use[c]) continue;
        rc = shape_batch(l, c, n_scans, max_n[c]);
        if (rc == LOCGPU_OK) l->batch[c]->d_src_ext = nullptr;  // the kernels read the batch's own copy
        if (rc == LOCGPU_OK) rc = from_ctx(l, c, upload_start(l->batch[c], srcs[c], counts[c], stride));
        started[c] = rc == LOCGPU_OK;
    }
    for (int c = 0; c < 2; ++c) {  // the caller's clouds are read until the join: also on the way out of a failed call
        if (!started[c]) continue;
        const int jrc = upload_join_batch(l->batch[c]);
        if (rc == LOCGPU_OK) rc = from_ctx(l, c, jrc);
    }
    if (rc != LOCGPU_OK) return rc;
    for (int c = 0; c < 2; ++c) {
        if (!l->use[c]) continue;
        LOAM_HIP(l, upload_order_after(l->batch[c], l->stream));
        if (l->ctx[c]->stream != l->stream) {
            LOAM_HIP(l, hipEventRecord(l->ev, l->ctx[c]->stream));
            LOAM_HIP(l, hipStreamWaitEvent(l->stream, l->ev, 0));
        }
    }
    return LOCGPU_OK;
}

// The context whose stream is the handle's.
locgpu_ctx* stream_ctx(locgpu_loam* l) { return l->use[kSurf] ? l->ctx[kSurf] : l->ctx[kEdge]; }

// `c` as a read-only input of the handle (cloud_input_ready, as align_single of locgpu_api.hip): the handle's stream goes behind
// the call that produced it.
int cloud_ready(locgpu_loam* l, const locgpu_cloud* c, const char* who) {
    const hipError_t ce = cloud_input_ready(stream_ctx(l), c);
    if (ce == hipErrorInvalidDevice) return lfail(l, LOCGPU_ERR_INVALID, std::string(who) + ": a cloud belongs to a context on another GPU");
    if (ce == hipErrorInvalidValue) return lfail(l, LOCGPU_ERR_INVALID, std::string(who) + ": bad cloud");
    return lhip(l, ce, "ordering behind the cloud's context") ? LOCGPU_OK : LOCGPU_ERR_NO_DEVICE;
}

// The resident counterpart of upload_scans for one scan: both classes' storage batches get the shape of the host-pointer call on
// the same clouds (so the sums split alike and the poses are its poses, bit for bit) and read the points where the clouds hold them.
int attach_scans(locgpu_loam* l, const locgpu_cloud* const clouds[2], const char* who) {
    for (int c = 0; c < 2; ++c) {  // every argument is checked before anything is enqueued
        if (!l->use[c]) continue;
        if (!clouds[c] || !clouds[c]->ctx) return lfail(l, LOCGPU_ERR_INVALID, std::string(who) + ": the scan of an enabled feature class is NULL");
    }
    l->src_of[kSurf] = l->src_of[kEdge] = nullptr;
    l->split_scans = 0;
    for (int c = 0; c < 2; ++c) {
        if (!l->use[c]) continue;
        int rc = cloud_ready(l, clouds[c], who);
        if (rc == LOCGPU_OK) rc = shape_batch(l, c, 1, clouds[c]->n);
        if (rc != LOCGPU_OK) return rc;
        locgpu_batch* b = l->batch[c];
        const int jrc = from_ctx(l, c, upload_join_batch(b));  // a failed earlier upload stays with the batch until one replaces it: say so
        if (jrc != LOCGPU_OK) return jrc;
        b->d_src_ext = clouds[c]->n ? clouds[c]->d : nullptr;
        b->counts[0] = (int)clouds[c]->n;
        b->upl.h_counts[0] = b->counts[0];  // pinned, the uploader's (idle: every host-pointer call joins its upload before it returns)
        LOAM_HIP(l, upload_order_after(b, l->stream));
        LOAM_HIP(l, hipMemcpyAsync(b->d_counts, b->upl.h_counts, sizeof(int), hipMemcpyHostToDevice, l->stream));
        if (l->ctx[c]->stream != l->stream) {  // behind that context's target ingest
            LOAM_HIP(l, hipEventRecord(l->ev, l->ctx[c]->stream));
            LOAM_HIP(l, hipStreamWaitEvent(l->stream, l->ev, 0));
        }
    }
    return LOCGPU_OK;
}

// The fourth way to fill the storage batches: n DIFFERENT scans that are already resident, in the caller's batches. Class c's storage
// batch gets the shape locgpu_loam_align_batch gives it on the same scans — n_scans × the largest COUNT, whatever the caller's batch was
// created for (a batch filtered in place keeps its raw capacity) — so the sums split alike and the poses are that call's poses, bit
// for bit. The rows come over in ONE strided device-to-device copy (the host-pointer call copies them too, over PCIe), the device
// counts device to device; the host counts are the batch's. The caller's batches are read, never written.
int attach_batches(locgpu_loam* l, locgpu_batch* const in[2], int n_scans, const char* who) {
    l->src_of[kSurf] = l->src_of[kEdge] = nullptr;
    l->split_scans = 0;
    for (int c = 0; c < 2; ++c) {
        if (!l->use[c]) continue;
        locgpu_batch* from = in[c];
        const int urc = upload_join_batch(from);  // a pending upload of the caller's batch: its host side ends here
        if (urc != LOCGPU_OK) return lfail(l, urc, std::string(who) + ": " + locgpu_last_error(from->ctx));
        size_t max_cnt = 0;
        for (int i = 0; i < n_scans; ++i) max_cnt = std::max(max_cnt, (size_t)std::max(from->counts[i], 0));
        const int rc = shape_batch(l, c, n_scans, max_cnt);
        if (rc != LOCGPU_OK) return rc;
        locgpu_batch* b = l->batch[c];
        const int jrc = from_ctx(l, c, upload_join_batch(b));  // a failed earlier upload stays with the batch until one replaces it: say so
        if (jrc != LOCGPU_OK) return jrc;
        b->d_src_ext = nullptr;  // the kernels read the storage batch's own rows
        for (int i = 0; i < n_scans; ++i) b->counts[i] = b->upl.h_counts[i] = from->counts[i];
        LOAM_HIP(l, upload_order_after(b, l->stream));
        // behind whatever wrote the caller's batch: its upload, its context's stream (the picker, the filter), its own compute stream
        LOAM_HIP(l, upload_order_after(from, l->stream));
        hipStream_t writers[2] = {from->ctx->stream, from->stream};
        for (int k = 0; k < 2; ++k) {
            if (!writers[k] || writers[k] == l->stream || (k == 1 && writers[1] == writers[0])) continue;
            LOAM_HIP(l, hipEventRecord(l->ev, writers[k]));
            LOAM_HIP(l, hipStreamWaitEvent(l->stream, l->ev, 0));
        }
        if (max_cnt)
            LOAM_HIP(l, hipMemcpy2DAsync(b->d_src, (size_t)b->max_n * sizeof(float4), from->d_src, (size_t)from->max_n * sizeof(float4), max_cnt * sizeof(float4),
                                         (size_t)n_scans, hipMemcpyDeviceToDevice, l->stream));
        LOAM_HIP(l, hipMemcpyAsync(b->d_counts, from->d_counts, (size_t)n_scans * sizeof(int), hipMemcpyDeviceToDevice, l->stream));
        if (l->ctx[c]->stream != l->stream) {  // behind that context's target ingest
            LOAM_HIP(l, hipEventRecord(l->ev, l->ctx[c]->stream));
            LOAM_HIP(l, hipStreamWaitEvent(l->stream, l->ev, 0));
        }
    }
    return LOCGPU_OK;
}

// The third way to fill the storage batches, beside upload_scans and attach_scans: the ONE pair of scans of a score under many poses or
// of a candidate search. Class c's batch is shaped for `entries` entries of n[c] points (the largest chunk: share_entries shapes every
// chunk inside it) and its region 0 holds the scan — copied once from host[c], or read where clouds[c] holds it (clouds != nullptr).
int share_scans(locgpu_loam* l, const char* who, const void* const host[2], const locgpu_cloud* const* clouds, const size_t n[2], size_t stride, int entries) {
    for (int c = 0; c < 2; ++c) {
        if (!l->use[c]) continue;
        int rc = clouds && n[c] ? cloud_ready(l, clouds[c], who) : LOCGPU_OK;
        if (rc == LOCGPU_OK) rc = shape_batch(l, c, entries, n[c]);
        if (rc != LOCGPU_OK) return rc;
        locgpu_batch* b = l->batch[c];
        const int jrc = from_ctx(l, c, upload_join_batch(b));  // a failed earlier upload stays with the batch until one replaces it: say so
        if (jrc != LOCGPU_OK) return jrc;
        LOAM_HIP(l, upload_order_after(b, l->stream));
        if (l->d_src_of[c].cap() < (size_t)b->cap_scans) {
            if (!lhip(l, l->d_src_of[c].alloc((size_t)b->cap_scans), "hipMalloc src_of")) return LOCGPU_ERR_OOM;
            LOAM_HIP(l, hipMemsetAsync(l->d_src_of[c], 0, (size_t)b->cap_scans * sizeof(int), l->stream));
        }
        b->d_src_ext = nullptr;
        if (clouds) {
            if (n[c]) b->d_src_ext = clouds[c]->d;
        } else if (n[c]) {
            if (l->h_shared[c].cap() < n[c] && !lhip(l, l->h_shared[c].alloc(with_headroom(n[c])), "hipHostMalloc shared scan")) return LOCGPU_ERR_OOM;
            pack_points((const char*)host[c], stride, n[c], l->h_shared[c]);  // the deep copy of SetSource (icp_registration.cpp:252-265), once
            LOAM_HIP(l, hipMemcpyAsync(b->d_src, l->h_shared[c], n[c] * sizeof(float4), hipMemcpyHostToDevice, l->stream));
        }
        if (l->ctx[c]->stream != l->stream) {  // behind that context's target ingest
            LOAM_HIP(l, hipEventRecord(l->ev, l->ctx[c]->stream));
            LOAM_HIP(l, hipStreamWaitEvent(l->stream, l->ev, 0));
        }
        l->n_shared[c] = n[c];
        l->src_of[c] = l->d_src_of[c];
    }
    l->split_scans = 0;
    return LOCGPU_OK;
}

// One chunk of the shared-source form: `cnt` entries of the resident pair of scans, counts[i] = n for every entry; split > 0: the
// accumulate kernels split their sums as the plain batch of that many scans would (the m of the whole search).
int share_entries(locgpu_loam* l, int cnt, int split) {
    for (int c = 0; c < 2; ++c) {
        if (!l->use[c]) continue;
        const int rc = shape_batch(l, c, cnt, l->n_shared[c]);  // inside the capacity share_scans made: nothing is allocated
        if (rc != LOCGPU_OK) return rc;
        locgpu_batch* b = l->batch[c];
        b->counts.assign(cnt, (int)l->n_shared[c]);
        for (int i = 0; i < cnt; ++i) b->upl.h_counts[i] = (int)l->n_shared[c];  // pinned, the uploader's (idle); the previous chunk has left the stream
        LOAM_HIP(l, hipMemcpyAsync(b->d_counts, b->upl.h_counts, (size_t)cnt * sizeof(int), hipMemcpyHostToDevice, l->stream));
    }
    l->split_scans = split;
    return LOCGPU_OK;
}

// Class c has a target: the handle's own record, or — on borrowed contexts — whatever the context holds at this call.
int class_target(locgpu_loam* l, int c, const char* who) {
    if (!l->borrowed && !l->has_target[c]) return lfail(l, LOCGPU_ERR_NO_TARGET, std::string(who) + ": locgpu_loam_set_target has not been called");
    const int jrc = from_ctx(l, c, target_join(l->ctx[c]));  // an asynchronous ingest ends here at the latest
    if (jrc != LOCGPU_OK) return jrc;
    if (!l->ctx[c]->d_tree) return lfail(l, LOCGPU_ERR_NO_TARGET, std::string(who) + ": the " + (c == kSurf ? "surface" : "edge") + " class has no target");
    return from_ctx(l, c, refuse_forest(l->ctx[c], who));
}

// Both classes' requests against their current targets (check_icp: the asynchronous ingest ends here, the grid is built on first use).
int check_classes(locgpu_loam* l, AlignSpec spec[2], const char* who) {
    for (int c = 0; c < 2; ++c) {
        if (!l->use[c]) continue;
        if (!l->borrowed && !l->has_target[c]) return lfail(l, LOCGPU_ERR_NO_TARGET, std::string(who) + ": locgpu_loam_set_target has not been called");
        const int rc = from_ctx(l, c, check_icp(l->ctx[c], &class_opts(l, c), spec[c]));  // a borrowed context without a target: its LOCGPU_ERR_NO_TARGET
        if (rc != LOCGPU_OK) return rc;
    }
    return LOCGPU_OK;
}

// The alignment of the n scans resident in the storage batches (do_update = 1), or one evaluation at the poses (do_update = 0: the
// sums land in l->h_hb). Leaves the stream idle and the states in l->h_state.
int run(locgpu_loam* l, int n, const double* poses, const AlignSpec spec[2], int do_update) {
    hipStream_t s = l->stream;
    const int max_iteration = do_update ? l->opts.max_iteration : 1;
    for (int i = 0; i < n; ++i) init_state(l->h_state[i], poses + 7 * (size_t)i);
    GridSearchScratch gsc[2];
    for (int c = 0; c < 2; ++c) {
        if (!l->use[c]) continue;
        locgpu_batch* b = l->batch[c];
        const int grc = from_ctx(l, c, ensure_grid_lists(l->ctx[c], b, spec[c]));
        if (grc != LOCGPU_OK) return grc;
        gsc[c] = GridSearchScratch{b->d_grid_qkey, b->d_grid_sorted, b->d_grid_tile_count, b->d_grid_scan_temp};
        b->stage_ev.mode = 0;
        b->stage_ev.used = 0;
        b->counters_clean = false;
        LOAM_HIP(l, hipMemsetAsync(b->d_redo_count, 0, 4 * sizeof(unsigned int), s));
    }
    LOAM_HIP(l, hipMemcpyAsync(l->d_state, l->h_state, (size_t)n * sizeof(PoseState), hipMemcpyHostToDevice, s));
    LoamSolveArgs sa{};
    sa.max_iteration = max_iteration;
    sa.eps = l->opts.eps;
    sa.st = l->d_state;
    sa.do_update = do_update;
    sa.hb_out = do_update ? nullptr : l->d_hb;
    for (int c = 0; c < 2; ++c) {
        sa.partials[c] = l->use[c] ? l->batch[c]->d_partials : nullptr;
        sa.min_effective_pts[c] = class_opts(l, c).min_effective_pts;
        sa.list_counts[c] = l->use[c] ? l->batch[c]->d_redo_count : nullptr;
    }
    int launched = 0, rc = LOCGPU_OK;
    for (bool first = true; launched < max_iteration; first = false) {
        const int* active = nullptr;
        int n_active = 0;
        if (!first && n > 1) {  // later chunks run over the scans still open (enqueue_chunk, gn_driver.hip)
            for (int i = 0; i < n; ++i)
                if (!l->h_state[i].done) l->h_active[n_active++] = i;
            if (n_active < n) {
                LOAM_HIP(l, hipMemcpyAsync(l->d_active, l->h_active, (size_t)n_active * sizeof(int), hipMemcpyHostToDevice, s));
                active = l->d_active;
            }
        }
        const int todo = std::min(first ? kFirstChunk : kNextChunk, max_iteration - launched);
        for (int it = 0; it < todo && rc == LOCGPU_OK; ++it) {
            for (int c = 0; c < 2 && rc == LOCGPU_OK; ++c) {
                if (!l->use[c]) continue;
                locgpu_batch* b = l->batch[c];
                const LocalStage w{batch_src(b), l->d_state, active, active ? n_active : 0, l->src_of[c], l->split_scans, spec[c], nullptr, b->d_grid_qkey ? &gsc[c] : nullptr, false,
                                   c == kSurf ? "loam surface search" : "loam edge search"};
                const int blocks = launch_local_stage(l->ctx[c], b, w, s);
                if (blocks < 0) rc = from_ctx(l, c, LOCGPU_ERR_DEPTH);
                sa.blocks_per_scan[c] = blocks;
            }
            if (rc != LOCGPU_OK) break;
            sa.scans = active;
            launch_loam_solve(sa, active ? n_active : n, s);
            if (!lhip(l, hipGetLastError(), "kernel launch")) rc = LOCGPU_ERR_NO_DEVICE;
        }
        if (rc != LOCGPU_OK) { (void)hipStreamSynchronize(s); return rc; }  // nothing of the chunk runs on under the next upload
        launched += todo;
        LOAM_HIP(l, hipMemcpyAsync(l->h_state, l->d_state, (size_t)n * sizeof(PoseState), hipMemcpyDeviceToHost, s));
        if (!do_update) LOAM_HIP(l, hipMemcpyAsync(l->h_hb, l->d_hb, (size_t)n * kLoamHbW * sizeof(double), hipMemcpyDeviceToHost, s));
        LOAM_HIP(l, hipStreamSynchronize(s));
        bool all_done = true;
        for (int i = 0; i < n; ++i)
            if (!l->h_state[i].done) { all_done = false; break; }
        if (all_done) break;
    }
    if (launched == 0) LOAM_HIP(l, hipStreamSynchronize(s));  // max_iteration < 1: the state copy still reads the pinned poses
    for (int c = 0; c < 2; ++c)
        if (l->use[c]) l->batch[c]->counters_clean = true;  // every search was followed by its solve kernel, which zeroes them
    return LOCGPU_OK;
}

void write_stats(const PoseState& ps, locgpu_align_stats* st) {
    if (!st) return;
    st->iterations = ps.iterations; st->converged = ps.converged; st->status = ps.status; st->reserved = 0;
    st->last_effective_num = ps.last_eff; st->last_dx_norm = ps.last_dx_norm;
}

// Poses and statistics of the n scans run() left in l->h_state; a scan whose evaluation failed (status 3 / 4) hands back its init_pose.
void write_results(const locgpu_loam* l, int n, const double* init_poses, double* out_poses, locgpu_align_stats* stats) {
    for (int i = 0; i < n; ++i) {
        const PoseState& ps = l->h_state[i];
        double* o = out_poses + 7 * (size_t)i;
        if (ps.status != 0) {
            std::memcpy(o, init_poses + 7 * (size_t)i, 7 * sizeof(double));
        } else {
            for (int j = 0; j < 4; ++j) o[j] = ps.q[j];
            for (int j = 0; j < 3; ++j) o[4 + j] = ps.t[j];
        }
        write_stats(ps, stats ? stats + i : nullptr);
    }
}

void to_fitness(const double r[kFitW], locgpu_fitness* f) {
    f->inliers = (int64_t)r[1];
    f->finite_points = (int64_t)r[2];
    f->score = f->inliers > 0 ? r[0] / (double)f->inliers : HUGE_VAL;
}

// The joint score of the n entries resident in the storage batches under their poses → out[3i] joint, [3i + 1] surface, [3i + 2] edge.
// Per class the k = 1 exact search stage and the accumulate kernel of locgpu_icp_fitness (fitness_on_batch, gn_driver.hip) over the
// joint states, then ONE sum kernel for both (loam_fitness_sum_kernel, fitness.hip). Leaves the stream idle.
int score(locgpu_loam* l, int n, const double* poses, double max_range, locgpu_fitness* out) {
    hipStream_t s = l->stream;
    for (int i = 0; i < n; ++i) init_state(l->h_state[i], poses + 7 * (size_t)i);
    LOAM_HIP(l, hipMemcpyAsync(l->d_state, l->h_state, (size_t)n * sizeof(PoseState), hipMemcpyHostToDevice, s));
    const double* partials[2] = {nullptr, nullptr};
    int rows[2] = {0, 0};
    unsigned int* list_counts[2] = {nullptr, nullptr};
    for (int c = 0; c < 2; ++c) {
        if (!l->use[c]) continue;
        locgpu_batch* b = l->batch[c];
        if (!b->counters_clean) LOAM_HIP(l, hipMemsetAsync(b->d_redo_count, 0, 4 * sizeof(unsigned int), s));
        b->counters_clean = false;
        // the exact walk whatever the class's options say, skipping the points pcl::isFinite rejects (fitness_on_batch)
        SearchArgs sa = make_search_args(l->ctx[c], b, batch_src(b), l->d_state, 1, 1.0f, true);
        sa.src_of = l->src_of[c];
        if (!launch_icp_search(sa, s)) { (void)hipStreamSynchronize(s); return lfail(l, LOCGPU_ERR_DEPTH, "loam_fitness: unsupported tree depth"); }
        FitnessArgs fa{l->ctx[c]->d_tree, batch_src(b), b->d_counts, l->d_state, b->d_nn, b->max_n, b->n_scans, (float)(max_range * max_range), b->d_partials, nullptr, nullptr};
        fa.src_of = l->src_of[c];
        rows[c] = launch_icp_fitness_accum(fa, s);
        partials[c] = b->d_partials;
        list_counts[c] = b->d_redo_count;
    }
    launch_loam_fitness_sum(partials, rows, n, l->d_fit, list_counts, s);
    LOAM_HIP(l, hipGetLastError());
    LOAM_HIP(l, hipMemcpyAsync(l->h_fit, l->d_fit, (size_t)n * 3 * kFitW * sizeof(double), hipMemcpyDeviceToHost, s));
    LOAM_HIP(l, hipStreamSynchronize(s));
    for (int c = 0; c < 2; ++c)
        if (l->use[c]) l->batch[c]->counters_clean = true;  // the sum kernel zeroed them behind the searches
    for (int i = 0; i < 3 * n; ++i) to_fitness(l->h_fit + (size_t)i * kFitW, out + i);
    return LOCGPU_OK;
}

// Per-entry workspace of the shared-source form, per point: the plain storage batch's source row 16 B, neighbour lists 20 B and two
// work lists 8 B. A chunk's bound (search_chunks.hpp) is over both classes.
constexpr size_t kLoamSearchBytesPerPoint = 44;

// The arguments every shared-source entry point shares, checked before anything is copied or enqueued; n[] comes back as the points
// of the ENABLED classes (a switched-off class's scan is not read).
int check_shared(locgpu_loam* l, const char* who, const void* const host[2], const locgpu_cloud* const* clouds, size_t n[2], size_t stride, bool args_ok) {
    if (!args_ok || (!clouds && stride < 12)) return lfail(l, LOCGPU_ERR_INVALID, std::string(who) + ": bad arguments");
    for (int c = 0; c < 2; ++c) {
        if (!l->use[c]) { n[c] = 0; continue; }
        if (clouds) {
            if (!clouds[c] || !clouds[c]->ctx) return lfail(l, LOCGPU_ERR_INVALID, std::string(who) + ": the scan of an enabled feature class is NULL");
            if (clouds[c]->ctx->device != l->device) return lfail(l, LOCGPU_ERR_INVALID, std::string(who) + ": a cloud belongs to a context on another GPU");
            n[c] = clouds[c]->n;
        } else if (n[c] && !host[c]) {
            return lfail(l, LOCGPU_ERR_INVALID, std::string(who) + ": NULL scan pointer");
        }
        if (n[c] > 0x7FFFFF00u) return lfail(l, LOCGPU_ERR_INVALID, std::string(who) + ": too many points in a scan");
    }
    if (n[kSurf] + n[kEdge] == 0) return lfail(l, LOCGPU_ERR_INVALID, std::string(who) + ": both scans are empty");
    return LOCGPU_OK;
}

int shared_chunk(const size_t n[2], int m) { return search_chunk(kLoamSearchBytesPerPoint * (std::max<size_t>(n[kSurf], 1) + std::max<size_t>(n[kEdge], 1)), m); }

int fitness_shared(locgpu_loam* l, const char* who, const void* const host[2], const locgpu_cloud* const* clouds, size_t n[2], size_t stride, const double* poses,
                   int n_poses, double max_range, locgpu_fitness* out) {
    if (!l) return LOCGPU_ERR_INVALID;
    int rc = check_shared(l, who, host, clouds, n, stride, poses && out && n_poses >= 1 && !std::isnan(max_range));
    for (int c = 0; c < 2 && rc == LOCGPU_OK; ++c)
        if (l->use[c]) rc = class_target(l, c, who);
    if (rc != LOCGPU_OK) return rc;
    LOAM_HIP(l, hipSetDevice(l->device));
    const int chunk = shared_chunk(n, n_poses);
    l->resident = false;  // the storage batches take the shared-source form
    rc = reserve_joint(l, chunk);
    if (rc == LOCGPU_OK) rc = share_scans(l, who, host, clouds, n, stride, chunk);
    if (rc != LOCGPU_OK) return rc;
    return fitness_in_chunks(n_poses, chunk, [&](int off, int cnt) {
        const int erc = share_entries(l, cnt, 0);
        return erc != LOCGPU_OK ? erc : score(l, cnt, poses + 7 * (size_t)off, max_range, out + 3 * (size_t)off);
    });
}

int search_shared(locgpu_loam* l, const char* who, const void* const host[2], const locgpu_cloud* const* clouds, size_t n[2], size_t stride, const double* candidates,
                  int m, const locgpu_init_search_opts* sopts, double* out_poses, locgpu_fitness* out_fit, locgpu_align_stats* stats, int* best) {
    if (!l) return LOCGPU_ERR_INVALID;
    locgpu_init_search_opts so;
    if (sopts) so = *sopts; else locgpu_init_search_opts_default(&so);
    int rc = check_shared(l, who, host, clouds, n, stride,
                          candidates && m >= 1 && out_poses && out_fit && best && !std::isnan(so.max_range) && so.min_inlier_ratio >= 0.0);
    if (rc != LOCGPU_OK) return rc;
    AlignSpec spec[2];
    rc = check_classes(l, spec, who);
    if (rc != LOCGPU_OK) return rc;
    LOAM_HIP(l, hipSetDevice(l->device));
    const int chunk = shared_chunk(n, m);
    l->resident = false;  // the storage batches take the shared-source form
    rc = reserve_joint(l, chunk);
    if (rc == LOCGPU_OK) rc = share_scans(l, who, host, clouds, n, stride, chunk);
    if (rc != LOCGPU_OK) return rc;
    return init_search_in_chunks(m, chunk, so.min_inlier_ratio, out_fit, 3, best, [&](int off, int cnt) {
        const double* init = candidates + 7 * (size_t)off;
        double* poses = out_poses + 7 * (size_t)off;
        // every chunk sums as locgpu_loam_align_batch on all m copies would: chunking never shows in a pose
        int crc = share_entries(l, cnt, m);
        if (crc == LOCGPU_OK) crc = run(l, cnt, init, spec, 1);
        if (crc != LOCGPU_OK) return crc;
        write_results(l, cnt, init, poses, stats ? stats + off : nullptr);
        return score(l, cnt, poses, so.max_range, out_fit + 3 * (size_t)off);
    });
}

// *cloud += *edge; *cloud += *surf; pcl::transformPointCloud(*cloud, *result, pose.matrix().cast<float>()) (loam_registration.cpp:93-96):
// x, y, z of the edge points, then of the surface points, into the caller's points. An enabled class's points are in HBM from the
// alignment; a switched-off class's (when the caller hands them) are uploaded here.
int write_output(locgpu_loam* l, const void* src[2], const size_t n_pts[2], size_t stride, const double pose[7], void* out, size_t out_stride) {
    const size_t n_all = n_pts[kEdge] + n_pts[kSurf];
    if (n_all == 0) return LOCGPU_OK;
    hipStream_t s = l->stream;
    if (3 * n_all > l->h_xyz.cap()) {  // h_xyz is grown last
        const size_t cap = with_headroom(n_all);
        if (!lhip(l, l->d_xyz.alloc(cap * 3), "hipMalloc output cloud") || !lhip(l, l->h_xyz.alloc(cap * 3), "hipHostMalloc output cloud")) return LOCGPU_ERR_OOM;
    }
    double R[9];
    quat_to_R(pose, R);
    M12f m;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) m.v[4 * r + c] = (float)R[3 * r + c];
        m.v[4 * r + 3] = (float)pose[4 + r];
    }
    const int order[2] = {kEdge, kSurf};
    size_t at = 0;
    for (int k = 0; k < 2; ++k) {
        const int c = order[k];
        const size_t n = n_pts[c];
        if (n == 0) continue;
        const float4* d_pts = nullptr;
        if (l->use[c]) {
            d_pts = l->batch[c]->d_src;  // scan 0 of the one-scan shape
        } else {
            if (n > l->h_off.cap()) {  // h_off is grown last
                const size_t cap = with_headroom(n);
                if (!lhip(l, l->d_off.alloc(cap), "hipMalloc output cloud") || !lhip(l, l->h_off.alloc(cap), "hipHostMalloc output cloud")) return LOCGPU_ERR_OOM;
            }
            pack_points((const char*)src[c], stride, n, l->h_off);
            LOAM_HIP(l, hipMemcpyAsync(l->d_off, l->h_off, n * sizeof(float4), hipMemcpyHostToDevice, s));
            d_pts = l->d_off;
        }
        launch_transform_cloud(d_pts, n, m, l->d_xyz + 3 * at, s);
        at += n;
    }
    LOAM_HIP(l, hipGetLastError());
    LOAM_HIP(l, hipMemcpyAsync(l->h_xyz, l->d_xyz, n_all * 3 * sizeof(float), hipMemcpyDeviceToHost, s));
    LOAM_HIP(l, hipStreamSynchronize(s));
    char* ob = (char*)out;
    for (size_t i = 0; i < n_all; ++i) std::memcpy(ob + i * out_stride, l->h_xyz + 3 * i, 12);
    return LOCGPU_OK;
}

}  // namespace

extern "C" {

void locgpu_loam_opts_default(locgpu_loam_opts* o) {
    if (!o) return;
    locgpu_icp_opts_default(&o->surf);
    locgpu_icp_opts_default(&o->edge);
    o->surf.method = LOCGPU_P2PLANE;  // LoamOption::surf_icp_option_{IcpMethod::P2PLANE}, loam_registration.hpp:25
    o->edge.method = LOCGPU_P2LINE;   // edge_icp_option_{IcpMethod::P2LINE}, :26
    o->use_surf_points = 1;
    o->use_edge_points = 1;
    o->max_iteration = 20;
    o->eps = 1e-3;
}

int locgpu_loam_create(int device_id, const locgpu_loam_opts* opts, locgpu_loam** out) {
    if (!out) return lfail(nullptr, LOCGPU_ERR_INVALID, "loam_create: out is NULL");
    *out = nullptr;
    int rc = check_opts(opts);  // before any device call: a refusal needs no GPU
    if (rc != LOCGPU_OK) return rc;
    auto* l = new locgpu_loam();
    l->device = device_id;
    l->opts = *opts;
    l->use[kSurf] = opts->use_surf_points != 0;
    l->use[kEdge] = opts->use_edge_points != 0;
    for (int c = 0; c < 2 && rc == LOCGPU_OK; ++c) {
        if (!l->use[c]) continue;
        rc = locgpu_create(device_id, &l->ctx[c]);
        if (rc != LOCGPU_OK) g_loam_create_err = locgpu_last_error(nullptr);
        else if (!l->stream) l->stream = l->ctx[c]->stream;
    }
    if (rc == LOCGPU_OK && l->ev.ensure() != hipSuccess) rc = lfail(nullptr, LOCGPU_ERR_NO_DEVICE, "loam_create: hipEventCreate");
    if (rc != LOCGPU_OK) { locgpu_loam_destroy(l); return rc; }
    *out = l;
    return LOCGPU_OK;
}

int locgpu_loam_create_on(locgpu_ctx* surf_ctx, locgpu_ctx* edge_ctx, const locgpu_loam_opts* opts, locgpu_loam** out) {
    if (!out) return lfail(nullptr, LOCGPU_ERR_INVALID, "loam_create_on: out is NULL");
    *out = nullptr;
    if (!opts) return lfail(nullptr, LOCGPU_ERR_INVALID, "loam_create_on: opts is NULL");
    locgpu_ctx* ctx[2] = {surf_ctx, edge_ctx};
    const int32_t use[2] = {opts->use_surf_points, opts->use_edge_points};
    for (int c = 0; c < 2; ++c)
        if (use[c] && !ctx[c]) return lfail(nullptr, LOCGPU_ERR_INVALID, "loam_create_on: the context of an enabled feature class is NULL");
    int rc = check_opts(opts);  // before any device call: a refusal needs no GPU
    if (rc != LOCGPU_OK) return rc;
    if (use[kSurf] && use[kEdge] && (surf_ctx == edge_ctx || surf_ctx->device != edge_ctx->device))
        return lfail(nullptr, LOCGPU_ERR_INVALID, "loam_create_on: the two classes need two different contexts on one GPU");
    for (int c = 0; c < 2; ++c)
        if (use[c] && ctx[c]->forest_n > 0)
            return lfail(nullptr, LOCGPU_ERR_INVALID, "loam_create_on: a context holds a forest target (locgpu_icp_set_target_forest), which only the pairs calls read");
    auto* l = new locgpu_loam();
    l->borrowed = true;
    l->opts = *opts;
    for (int c = 0; c < 2; ++c) {
        l->use[c] = use[c] != 0;
        if (!l->use[c]) continue;
        l->ctx[c] = ctx[c];
        if (!l->stream) { l->stream = ctx[c]->stream; l->device = ctx[c]->device; }
    }
    if (hipSetDevice(l->device) != hipSuccess || l->ev.ensure() != hipSuccess) {
        locgpu_loam_destroy(l);
        return lfail(nullptr, LOCGPU_ERR_NO_DEVICE, "loam_create_on: hipEventCreate");
    }
    *out = l;
    return LOCGPU_OK;
}

void locgpu_loam_destroy(locgpu_loam* l) {
    if (!l) return;
    (void)hipSetDevice(l->device);
    if (l->stream) (void)hipStreamSynchronize(l->stream);
    for (int c = 0; c < 2; ++c) {
        if (l->batch[c]) free_batch(l->batch[c]);
        l->batch[c] = nullptr;
    }
    if (!l->borrowed)
        for (int c = 0; c < 2; ++c) locgpu_destroy(l->ctx[c]);  // borrowed contexts stay alive, with their targets
    delete l;
}

const char* locgpu_loam_last_error(const locgpu_loam* l) { return l ? l->err.c_str() : g_loam_create_err.c_str(); }

int locgpu_loam_set_target(locgpu_loam* l, const void* edge_pts, size_t n_edge, const void* surf_pts, size_t n_surf, size_t stride_bytes) {
    if (!l) return LOCGPU_ERR_INVALID;
    const void* pts[2] = {surf_pts, edge_pts};
    const size_t n[2] = {n_surf, n_edge};
    int rc = LOCGPU_OK;
    // like the reference (loam_registration.cpp:24-34) every enabled class is handed its cloud, whatever happened to the other
    for (int c = 0; c < 2; ++c) {
        if (!l->use[c]) continue;
        const int r = from_ctx(l, c, locgpu_icp_set_target(l->ctx[c], pts[c], n[c], stride_bytes));
        l->has_target[c] = r == LOCGPU_OK;
        if (r != LOCGPU_OK && rc == LOCGPU_OK) rc = r;
    }
    return rc;
}

static int set_target_cloud(locgpu_loam* l, const locgpu_cloud* edge_map, const locgpu_cloud* surf_map, bool async) {
    if (!l) return LOCGPU_ERR_INVALID;
    const locgpu_cloud* maps[2] = {surf_map, edge_map};
    int rc = LOCGPU_OK;
    // like locgpu_loam_set_target (loam_registration.cpp:24-34): every enabled class is handed its cloud, whatever happened to the other
    for (int c = 0; c < 2; ++c) {
        if (!l->use[c]) continue;
        int r;
        if (!maps[c] || !maps[c]->ctx) r = lfail(l, LOCGPU_ERR_INVALID, "loam_set_target_cloud: the map of an enabled feature class is NULL");
        else r = from_ctx(l, c, icp_set_target_from_cloud(l->ctx[c], maps[c], async));
        l->has_target[c] = r == LOCGPU_OK;
        if (r != LOCGPU_OK && rc == LOCGPU_OK) rc = r;
    }
    return rc;
}

int locgpu_loam_set_target_cloud(locgpu_loam* l, const locgpu_cloud* edge_map, const locgpu_cloud* surf_map) { return set_target_cloud(l, edge_map, surf_map, false); }

int locgpu_loam_set_target_cloud_async(locgpu_loam* l, const locgpu_cloud* edge_map, const locgpu_cloud* surf_map) { return set_target_cloud(l, edge_map, surf_map, true); }

int locgpu_loam_hb(locgpu_loam* l, const void* edge, size_t n_edge, const void* surf, size_t n_surf, size_t stride_bytes, const double pose[7], double H[36],
                   double B[6], int64_t eff[2], int32_t ok[2]) {
    if (!l) return LOCGPU_ERR_INVALID;
    if (!pose || !H || !B || stride_bytes < 12) return lfail(l, LOCGPU_ERR_INVALID, "loam_hb: bad arguments");
    AlignSpec spec[2];
    int rc = check_classes(l, spec, "loam_hb");
    if (rc != LOCGPU_OK) return rc;
    LOAM_HIP(l, hipSetDevice(l->device));
    const void* s1[2] = {surf, edge};
    const size_t c1[2] = {n_surf, n_edge};
    const void* const* srcs[2] = {&s1[kSurf], &s1[kEdge]};
    const size_t* counts[2] = {&c1[kSurf], &c1[kEdge]};
    l->resident = false;
    rc = reserve_joint(l, 1);
    if (rc == LOCGPU_OK) rc = upload_scans(l, 1, srcs, counts, stride_bytes);
    if (rc == LOCGPU_OK) rc = run(l, 1, pose, spec, 0);
    if (rc != LOCGPU_OK) return rc;
    l->resident = true;
    std::memcpy(H, l->h_hb, 36 * sizeof(double));
    std::memcpy(B, l->h_hb + 36, 6 * sizeof(double));
    for (int c = 0; c < 2; ++c) {
        if (eff) eff[c] = (int64_t)l->h_hb[42 + c];
        if (ok) ok[c] = l->h_hb[44 + c] != 0.0;
    }
    return LOCGPU_OK;
}

int locgpu_loam_scan_match(locgpu_loam* l, const void* edge, size_t n_edge, const void* surf, size_t n_surf, size_t stride_bytes, const double init_pose[7],
                           double result_pose[7], locgpu_align_stats* stats, void* out_cloud, size_t out_stride_bytes) {
    if (!l) return LOCGPU_ERR_INVALID;
    if (!init_pose || !result_pose || stride_bytes < 12 || (out_cloud && out_stride_bytes < 12)) return lfail(l, LOCGPU_ERR_INVALID, "loam_scan_match: bad arguments");
    AlignSpec spec[2];
    int rc = check_classes(l, spec, "loam_scan_match");
    if (rc != LOCGPU_OK) return rc;
    LOAM_HIP(l, hipSetDevice(l->device));
    const void* s1[2] = {surf, edge};
    const size_t c1[2] = {n_surf, n_edge};
    const void* const* srcs[2] = {&s1[kSurf], &s1[kEdge]};
    const size_t* counts[2] = {&c1[kSurf], &c1[kEdge]};
    l->resident = false;
    rc = reserve_joint(l, 1);
    if (rc == LOCGPU_OK) rc = upload_scans(l, 1, srcs, counts, stride_bytes);
    if (rc == LOCGPU_OK) rc = run(l, 1, init_pose, spec, 1);
    if (rc != LOCGPU_OK) return rc;
    l->resident = true;
    const PoseState& ps = l->h_state[0];
    write_stats(ps, stats);
    if (ps.status != 0) return LOCGPU_OK;  // `return false` before `result_pose = pose` (loam_registration.cpp:56-70): the caller's value and cloud stay
    for (int j = 0; j < 4; ++j) result_pose[j] = ps.q[j];
    for (int j = 0; j < 3; ++j) result_pose[4 + j] = ps.t[j];
    if (!out_cloud) return LOCGPU_OK;
    // a switched-off class takes part in the output cloud when the caller hands its points (the reference adds both, :93-95)
    const size_t n_out[2] = {(l->use[kSurf] || surf) ? n_surf : 0, (l->use[kEdge] || edge) ? n_edge : 0};
    return write_output(l, s1, n_out, stride_bytes, result_pose, out_cloud, out_stride_bytes);
}

int locgpu_loam_scan_match_cloud(locgpu_loam* l, const locgpu_cloud* edge, const locgpu_cloud* surf, const double init_pose[7], double result_pose[7],
                                 locgpu_align_stats* stats, locgpu_cloud* out) {
    if (!l) return LOCGPU_ERR_INVALID;
    if (!init_pose || !result_pose || (out && (!out->ctx || out == edge || out == surf))) return lfail(l, LOCGPU_ERR_INVALID, "loam_scan_match_cloud: bad arguments (out must be distinct from edge and surf)");
    AlignSpec spec[2];
    int rc = check_classes(l, spec, "loam_scan_match_cloud");
    if (rc != LOCGPU_OK) return rc;
    LOAM_HIP(l, hipSetDevice(l->device));
    const locgpu_cloud* clouds[2] = {surf, edge};
    // a switched-off class takes part in the output cloud when the caller hands its points (the reference adds both, :93-95)
    const size_t n_out[2] = {surf && surf->ctx ? surf->n : 0, edge && edge->ctx ? edge->n : 0};
    if (out && n_out[kSurf] + n_out[kEdge] > 0x7FFFFF00u) return lfail(l, LOCGPU_ERR_INVALID, "loam_scan_match_cloud: the output cloud exceeds 2^31 points");
    l->resident = false;
    rc = reserve_joint(l, 1);
    if (rc == LOCGPU_OK) rc = attach_scans(l, clouds, "loam_scan_match_cloud");
    if (rc == LOCGPU_OK) rc = run(l, 1, init_pose, spec, 1);
    if (rc != LOCGPU_OK) return rc;
    l->resident = true;
    const PoseState& ps = l->h_state[0];
    write_stats(ps, stats);
    if (ps.status != 0) return LOCGPU_OK;  // `return false` before `result_pose = pose` (loam_registration.cpp:56-70): the caller's value and cloud stay
    for (int j = 0; j < 4; ++j) result_pose[j] = ps.q[j];
    for (int j = 0; j < 3; ++j) result_pose[4 + j] = ps.t[j];
    if (!out) return LOCGPU_OK;
    // *cloud += *edge; *cloud += *surf; transformPointCloud(*cloud, *result, pose.matrix().cast<float>()) (:93-96), on the device
    for (int c = 0; c < 2; ++c)
        if (!l->use[c] && n_out[c]) { rc = cloud_ready(l, clouds[c], "loam_scan_match_cloud"); if (rc != LOCGPU_OK) return rc; }
    rc = cloud_ready(l, out, "loam_scan_match_cloud");  // behind whatever its owner last did with it
    if (rc != LOCGPU_OK) return rc;
    const size_t n_all = n_out[kEdge] + n_out[kSurf];
    if (!lhip(l, cloud_reserve(out, n_all, false), "loam_scan_match_cloud: hipMalloc output cloud")) return LOCGPU_ERR_OOM;
    double R[9];
    quat_to_R(result_pose, R);
    M12f m;
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) m.v[4 * r + c] = (float)R[3 * r + c];
        m.v[4 * r + 3] = (float)result_pose[4 + r];
    }
    launch_loam_join_transform(n_out[kEdge] ? edge->d : nullptr, n_out[kEdge], n_out[kSurf] ? surf->d : nullptr, n_out[kSurf], m, out->d, l->stream);
    LOAM_HIP(l, hipGetLastError());
    LOAM_HIP(l, hipStreamSynchronize(l->stream));  // the call is synchronous: the owner of `out` may use it at once
    out->n = n_all;
    out->is_dense = 1;  // operator+= ANDs the flags (a cloud that was not handed adds nothing)
    for (int c = 0; c < 2; ++c)
        if (clouds[c] && clouds[c]->ctx && !clouds[c]->is_dense) out->is_dense = 0;
    (void)cloud_mark_ready(out);
    return LOCGPU_OK;
}

int locgpu_loam_fitness_resident(locgpu_loam* l, const double pose[7], double max_range, locgpu_fitness out[2]) {
    if (!l) return LOCGPU_ERR_INVALID;
    if (!pose || !out || std::isnan(max_range)) return lfail(l, LOCGPU_ERR_INVALID, "loam_fitness_resident: bad arguments");
    if (!l->resident) return lfail(l, LOCGPU_ERR_INVALID, "loam_fitness_resident: no scans of a single-scan call are resident");
    for (int c = 0; c < 2; ++c) {
        if (!l->use[c]) continue;
        if (!l->borrowed && !l->has_target[c]) return lfail(l, LOCGPU_ERR_NO_TARGET, "loam_fitness_resident: locgpu_loam_set_target has not been called");
        const int jrc = from_ctx(l, c, target_join(l->ctx[c]));  // an asynchronous ingest ends here at the latest
        if (jrc != LOCGPU_OK) return jrc;
        if (!l->ctx[c]->d_tree) return lfail(l, LOCGPU_ERR_NO_TARGET, "loam_fitness_resident: locgpu_loam_set_target has not been called");
    }
    for (int c = 0; c < 2; ++c) {
        out[c].score = HUGE_VAL;
        out[c].inliers = out[c].finite_points = 0;
        if (!l->use[c] || l->batch[c]->counts[0] <= 0) continue;
        // the class's one-scan storage batch on its own context: locgpu_icp_fitness of that scan against that map, its bits
        const int rc = from_ctx(l, c, fitness_on_batch(l->ctx[c], l->batch[c], pose, max_range, &out[c]));
        if (rc != LOCGPU_OK) return rc;
    }
    return LOCGPU_OK;
}

int locgpu_loam_fitness(locgpu_loam* l, const void* edge, size_t n_edge, const void* surf, size_t n_surf, size_t stride_bytes, const double* poses, int n_poses,
                        double max_range, locgpu_fitness* out) {
    const void* host[2] = {surf, edge};
    size_t n[2] = {n_surf, n_edge};
    return fitness_shared(l, "loam_fitness", host, nullptr, n, stride_bytes, poses, n_poses, max_range, out);
}

int locgpu_loam_fitness_cloud(locgpu_loam* l, const locgpu_cloud* edge, const locgpu_cloud* surf, const double* poses, int n_poses, double max_range,
                              locgpu_fitness* out) {
    const locgpu_cloud* clouds[2] = {surf, edge};
    size_t n[2] = {0, 0};
    return fitness_shared(l, "loam_fitness_cloud", nullptr, clouds, n, 0, poses, n_poses, max_range, out);
}

int locgpu_loam_init_search(locgpu_loam* l, const void* edge, size_t n_edge, const void* surf, size_t n_surf, size_t stride_bytes, const double* candidates, int m,
                            const locgpu_init_search_opts* sopts, double* out_poses, locgpu_fitness* out_fit, locgpu_align_stats* stats, int* best) {
    const void* host[2] = {surf, edge};
    size_t n[2] = {n_surf, n_edge};
    return search_shared(l, "loam_init_search", host, nullptr, n, stride_bytes, candidates, m, sopts, out_poses, out_fit, stats, best);
}

int locgpu_loam_init_search_cloud(locgpu_loam* l, const locgpu_cloud* edge, const locgpu_cloud* surf, const double* candidates, int m,
                                  const locgpu_init_search_opts* sopts, double* out_poses, locgpu_fitness* out_fit, locgpu_align_stats* stats, int* best) {
    const locgpu_cloud* clouds[2] = {surf, edge};
    size_t n[2] = {0, 0};
    return search_shared(l, "loam_init_search_cloud", nullptr, clouds, n, 0, candidates, m, sopts, out_poses, out_fit, stats, best);
}

int locgpu_loam_align_batch(locgpu_loam* l, int n_scans, const void* const* edge_srcs, const size_t* edge_counts, const void* const* surf_srcs,
                            const size_t* surf_counts, size_t stride_bytes, const double* init_poses, double* out_poses, locgpu_align_stats* stats) {
    if (!l) return LOCGPU_ERR_INVALID;
    if (n_scans < 1 || n_scans > 65535 || !init_poses || !out_poses || stride_bytes < 12) return lfail(l, LOCGPU_ERR_INVALID, "loam_align_batch: bad arguments (1 <= n_scans <= 65535)");
    AlignSpec spec[2];
    int rc = check_classes(l, spec, "loam_align_batch");
    if (rc != LOCGPU_OK) return rc;
    LOAM_HIP(l, hipSetDevice(l->device));
    const void* const* srcs[2] = {surf_srcs, edge_srcs};
    const size_t* counts[2] = {surf_counts, edge_counts};
    l->resident = false;  // the storage batches take the batch's shape
    rc = reserve_joint(l, n_scans);
    if (rc == LOCGPU_OK) rc = upload_scans(l, n_scans, srcs, counts, stride_bytes);
    if (rc == LOCGPU_OK) rc = run(l, n_scans, init_poses, spec, 1);
    if (rc != LOCGPU_OK) return rc;
    write_results(l, n_scans, init_poses, out_poses, stats);
    return LOCGPU_OK;
}

int locgpu_loam_align_batches(locgpu_loam* l, locgpu_batch* edge, locgpu_batch* surf, const double* init_poses, double* out_poses, locgpu_align_stats* stats) {
    if (!l) return LOCGPU_ERR_INVALID;
    if (!init_poses || !out_poses) return lfail(l, LOCGPU_ERR_INVALID, "loam_align_batches: bad arguments");
    locgpu_batch* in[2] = {surf, edge};
    int n_scans = -1;
    for (int c = 0; c < 2; ++c) {  // every argument is checked before anything is enqueued; a switched-off class's batch is not looked at
        if (!l->use[c]) continue;
        const locgpu_batch* b = in[c];
        if (!b || !b->ctx) return lfail(l, LOCGPU_ERR_INVALID, "loam_align_batches: the batch of an enabled feature class is NULL");
        if (b->ctx->device != l->device) return lfail(l, LOCGPU_ERR_INVALID, "loam_align_batches: a batch belongs to a context on another GPU");
        if (b->sharded) return lfail(l, LOCGPU_ERR_INVALID, "loam_align_batches: sharded batches are not supported");
        if (b->shared_src) return lfail(l, LOCGPU_ERR_INVALID, "loam_align_batches: shared-source batches are not supported");
        if (b->pending.active) return lfail(l, LOCGPU_ERR_INVALID, "loam_align_batches: an alignment of a batch has been begun and not finished");
        if (n_scans >= 0 && b->n_scans != n_scans) return lfail(l, LOCGPU_ERR_INVALID, "loam_align_batches: the two batches hold different numbers of scans");
        n_scans = b->n_scans;
    }
    if (n_scans < 1 || n_scans > 65535) return lfail(l, LOCGPU_ERR_INVALID, "loam_align_batches: 1 <= n_scans <= 65535");
    AlignSpec spec[2];
    int rc = check_classes(l, spec, "loam_align_batches");
    if (rc != LOCGPU_OK) return rc;
    LOAM_HIP(l, hipSetDevice(l->device));
    l->resident = false;  // the storage batches take the batch's shape
    rc = reserve_joint(l, n_scans);
    if (rc == LOCGPU_OK) rc = attach_batches(l, in, n_scans, "loam_align_batches");
    if (rc == LOCGPU_OK) rc = run(l, n_scans, init_poses, spec, 1);
    if (rc != LOCGPU_OK) return rc;
    write_results(l, n_scans, init_poses, out_poses, stats);
    return LOCGPU_OK;
}

}  // extern "C"
