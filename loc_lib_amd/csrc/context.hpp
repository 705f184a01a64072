// loc_lib_amd/csrc/context.hpp — host-side state behind the opaque handles of include/locgpu.h.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <vector>

#include "../../include/locgpu.h"
#include "batch_upload.hpp"
#include "device_buffer.hpp"
#include "device_math.hpp"
#include "grid_kernels.hpp"
#include "icp_kernels.hpp"

#include "host_worker.hpp"

struct NdtTable;  // ndt_kernels.hpp
namespace locgpu {
struct IncNdtState;         // ndt_inc.hip
struct FilterScratch;       // cloud_filters.hpp
struct LoamScratch;         // loam_features.hip
struct BatchFilterScratch;  // batch_filters.hip
struct BatchLoamScratch;    // batch_loam.hip
struct MergeScratch;        // cloud_merge.hip
struct RangeIngestScratch;  // range_ingest.hip
struct RecordIngestScratch;  // record_ingest.hip
struct ResidentDeskewScratch;  // resident_deskew.hip
struct ForestBuildScratch;  // forest_build.hpp
}  // namespace locgpu
struct locgpu_sensor;  // range_ingest.hpp

namespace locgpu {
struct PendingTarget;
// A validated alignment request: what check_icp / check_ndt (locgpu_api.hip), its only producers, make of the caller's options, and
// the one value the Gauss–Newton driver, a batch's pending alignment, its graph-cache key and a scan pool are told it by.
struct AlignSpec {
    GnParams prm{};
    float alpha = 1.0f;  // pruning factor of the tree walk; 1.0f = exact. Always 1.0f for grid and NDT.
    bool grid = false;   // LOCGPU_SEARCH_GRID_EXACT was asked for
    bool pairs = false;  // locgpu_icp_align_pairs: scan i is searched in the tree at the batch's pair_base[i] of the context's forest; locgpu_ndt_align_pairs: it is
                         // looked up under target pair_base[i] of the context's voxel set; eager only
    bool ndt() const { return method_is_ndt(prm.method); }
    int k() const { return method_k(prm.method); }
    bool operator==(const AlignSpec& o) const { return prm == o.prm && alpha == o.alpha && grid == o.grid && pairs == o.pairs; }
};
// locgpu_ndt_opts::method and ::nearby_type (NdtMethod, NdtNearbyType of the reference), and the voxels a nearby type probes per point.
constexpr int kNdtOptDirect = 1, kNdtOptIncremental = 2;
constexpr int kNearbyCenter = 0, kNearby6 = 1;
constexpr int ndt_n_nearby(int nearby_type) { return nearby_type == kNearbyCenter ? 1 : 7; }
// Stage marks of locgpu_profile_enable (gn_driver.hip): HIP events around the stages of every Gauss–Newton iteration enqueued on one
// stream since the last collect().
struct StageEvents {
    std::vector<Event> ev;
    size_t used = 0;
    int mode = 0;  // 0: record nothing (also under stream capture); 1: search | fit + accumulate | solve; 2: the search stage's edges only
    void mark(hipStream_t s, bool search_edge = false);
    void collect(locgpu_ctx* ctx, bool ndt);  // the stream is idle: adds the elapsed times to ctx->prof_ms / prof_n
};
}  // namespace locgpu

struct locgpu_ctx {
    int device = 0;
    hipStream_t stream = nullptr;  // = slot_stream[0]: target ingest, clouds, single-scan calls
    // kSlots compute streams, so that an alignment begun on one batch (locgpu_*_align_batch_begin) runs under the tail of the one begun
    // before it: late Gauss–Newton iterations hold a handful of scans and leave most of the chip idle. Three, because that is what
    // pays (32 / 64 scans per batch: +14 % scans/s over two, nothing more with four) and because three compute streams + the copy
    // stream are the four hardware queues the runtime deals streams to in creation order.
    // Batches are dealt to them in turn when they are created, but a stream is LEASED PER ALIGNMENT (stream_lease.hpp; align_begin /
    // align_finish, gn_driver.hip): a batch keeps its stream while no other alignment in flight is on it and otherwise moves to the
    // least-loaded one. A streaming caller with three alignments in flight rotates four batches — two of them were dealt the same
    // stream and are in flight together in two steps of every four. slot_load[i]: alignments begun and not ended on slot_stream[i].
    // One caller thread per context (locgpu.h) is what guards these counters, as it guards next_slot.
    static constexpr int kSlots = 3;
    hipStream_t slot_stream[kSlots] = {};
    int next_slot = 0;
    int slot_load[kSlots] = {};
    hipStream_t copy_stream = nullptr;  // host → HBM copies of the batch uploader
    locgpu::Event foreign_ev;           // ordering behind another context's stream when one of ITS clouds is an input here (cloud_input_ready)
    hipStream_t comm_stream = nullptr;  // every collective of the context, in host order (one communicator, one stream: no two at once)
    locgpu::Uploader* up = nullptr;     // host → HBM staging shared by the context's batches (batch_upload.hpp)
    locgpu::PendingTarget* target_scratch = nullptr;  // the previous ingest's host buffers, kept for the next one (icp_target.hip)
    locgpu::PendingTarget* pending_target = nullptr;  // locgpu_icp_set_target_cloud_async: a host tree build still running (icp_target.hip)
    std::string err;

    // ICP target: packed KD-tree in HBM (kdtree_build.cpp layout)
    locgpu::DevBuf<uint2> d_tree;  // grow-only
    size_t tree_slots = 0, num_leaves = 0, num_nodes = 0, num_points = 0;
    int depth = 0;
    bool tree_bounded = true;  // PackedKdTree::bounded: the fast search kernel may be used
    unsigned long long target_epoch = 0;  // bumped by every set_target: captured graphs of older targets are never replayed

    locgpu::DevBuf<uint32_t> d_leaf_slots;  // grow-only: slot of every leaf, preorder (what the exact-search grid is built from)

    // Forest target (locgpu_icp_set_target_forest, icp_target.hip): d_tree holds forest_n > 0 trees behind one another, tree j from
    // slot forest_base[j] on; tree_slots, num_*, depth (the largest) and tree_bounded (the AND) are the whole forest's. Only the pairs
    // calls read such a target (refuse_forest); every locgpu_icp_set_target* makes the context ordinary again (forest_n = 0).
    int forest_n = 0;
    std::vector<uint32_t> forest_base;
    std::vector<size_t> forest_leaves;
    std::vector<int> forest_depth;
    locgpu::DevBuf<uint32_t> d_forest_base;  // grow-only: the device table of the bases
    locgpu::ForestBuildScratch* fbuild = nullptr;  // the device tree build's scratch, the tree it builds beside d_tree, and its report (forest_build.hip)

    // LOCGPU_P2PLANE_MAP: one plane per leaf, row slot >> 1 = four doubles, NaNs = none (map_planes.hip). Built on first use or by
    // locgpu_icp_build_map_planes, dropped (planes_ready) by every set_target; the buffers are grow-only.
    locgpu::DevBuf<double> d_planes;
    size_t planes_rows = 0;
    bool planes_ready = false;
    long long planes_valid = 0;
    locgpu::DevBuf<unsigned long long> d_planes_count;
    locgpu_batch* planes_ws = nullptr;  // one-scan search batch of the ingest's chunks

    // exact-search grid over the tree's leaves (built on the device on first use of LOCGPU_SEARCH_GRID_EXACT)
    locgpu::GridView grid;
    locgpu::GridBuffers grid_buf;

    // BfnnRegistration target (bfnn.hip)
    locgpu::DevBuf<float4> d_bfnn;
    size_t bfnn_n = 0;

    // NDT target
    NdtTable* ndt = nullptr;
    locgpu::IncNdtState* inc = nullptr;  // incremental NDT voxel set (persists across set_target calls)
    locgpu_ndt_opts ndt_opts;
    // Voxel-set target (locgpu_ndt_set_target_set, ndt_pairs.hip): `ndt` holds the grids of ndt_set_n > 0 targets under keys that carry
    // the target's index; target j has ndt_set_points[j] points and ndt_set_voxels[j] records from record ndt_set_first[j] on. Only the
    // pairs calls read such a target (refuse_ndt_set); every locgpu_ndt_set_target* makes the context ordinary again (ndt_set_n = 0).
    int ndt_set_n = 0;
    std::vector<size_t> ndt_set_points, ndt_set_voxels, ndt_set_first;

    locgpu::FilterScratch* filt = nullptr;  // workspaces of the cloud filters (cloud_filters.hip)
    locgpu::LoamScratch* loam = nullptr;    // workspaces of the LOAM feature picker (loam_features.hip)
    locgpu::BatchFilterScratch* bfilt = nullptr;  // workspaces of the batch front-end (batch_filters.hip)
    locgpu::BatchLoamScratch* bloam = nullptr;    // workspaces of the batched LOAM feature picker (batch_loam.hip)
    locgpu::MergeScratch* merge = nullptr;        // table and joined cloud of the global-map pass (cloud_merge.hip)
    locgpu::RangeIngestScratch* ringest = nullptr;  // staging and workspaces of the range-image ingest (range_ingest.hip)
    locgpu::RecordIngestScratch* recingest = nullptr;  // staging and workspaces of the point-record ingest (record_ingest.hip)
    locgpu::ResidentDeskewScratch* rdeskew = nullptr;  // motion staging and workspaces of locgpu_batch_deskew (resident_deskew.hip)
    std::vector<locgpu_sensor*> sensors;          // the sensor models created on this context and not destroyed yet (range_ingest.hip)

    // reusable one-scan batch for the single-scan entry points
    locgpu_batch* single = nullptr;
    size_t single_cap = 0;
    // the shared-source batch of locgpu_icp_fitness (several poses) and locgpu_icp_init_search: kept between calls, grow-only, at most
    // kSearchEntries entries and kSearchBytes of per-entry workspace (locgpu.h says what that retains)
    locgpu_batch* search = nullptr;
    locgpu::HostWorker* worker = nullptr;  // locgpu_*_scan_match: host copy of the output cloud's fields beside the alignment

    // multi-GPU (locgpu_comm_init): RCCL communicator of the ranks that share sharded batches
    void* comm = nullptr;  // ncclComm_t
    int comm_rank = 0, comm_world = 1;

    // measurement
    int profile = 0;  // 0 off, 1 = events around search / fit+accumulate / solve, 2 = around the search stage only
    double prof_ms[3] = {0, 0, 0};
    long long prof_n[3] = {0, 0, 0};
    bool use_graph = false;  // replay a captured hipGraph of all GN iterations instead of eager chunks
    bool count_visits = false;
    locgpu::DevBuf<unsigned long long> d_visits;  // [4]: nodes, leaves, queries, distinct tree slots read (summed over launches)
    locgpu::DevBuf<uint32_t> d_touched;      // instrumented pass: one bit per tree slot
    size_t touched_words = 0;
    locgpu::DevBuf<unsigned long long> d_search_stats;  // [2]: queries searched / queries redone by the exact kernel
};

struct locgpu_batch {
    locgpu_ctx* ctx = nullptr;
    int slot = 0;
    hipStream_t stream = nullptr;  // ctx->slot_stream[slot]: everything the batch's current (or last) alignment enqueues; align_begin may move it
    bool pinned = false;           // one-scan and workspace batches of the context: they stay on ctx->stream, where the clouds and the target ingest are ordered with them — never leased
    bool leased = false;           // an alignment begun on this batch counts in ctx->slot_load[slot]
    locgpu::Event chunk_ev;        // behind the read-back of the last chunk enqueued: what align_finish waits for (NOT the stream: another batch's alignment may be queued behind)
    int n_scans = 0, max_n = 0, blocks_per_scan = 0;  // n_scans: the scans whose points THIS rank holds
    // Sharded batch (locgpu_batch_create_sharded): the batch has n_total scans, this rank holds the points of scans
    // [first, first + n_scans) — or, point-sharded, a slice of the points of every scan (first = 0, n_scans = n_total). Poses, flags
    // and normal equations exist for all n_total scans on every rank. Unsharded: n_total = n_scans, first = 0.
    int n_total = 0, first = 0;
    bool sharded = false;
    locgpu::DevBuf<double> d_acc;  // [n_total][kAccW] per-scan sums, all-reduced over the communicator (sharded batches only)
    size_t pitch = 0;  // n_scans * max_n
    locgpu::DevBuf<float4> d_src;
    locgpu::DevBuf<int> d_counts;
    // One ring byte per point slot, [n_scans][max_n], left by locgpu_batch_upload_ranges (range_ingest.hip) and read by
    // locgpu_batch_loam_extract_resident. Allocated on first use; rings_valid is dropped by everything else that writes d_src.
    locgpu::DevBuf<unsigned char> d_rings;
    bool rings_valid = false;
    // locgpu_batch_keep_times: one float64 time key per point slot, [n_scans][max_n], left beside the ring bytes by the PLAIN ingest
    // calls (range_ingest.hip, record_ingest.hip) and read by locgpu_batch_deskew (resident_deskew.hip). Allocated on first use;
    // times_valid is dropped wherever rings_valid is, and by the ingest calls that leave no times.
    bool keep_times = false;
    locgpu::DevBuf<double> d_times;
    bool times_valid = false;
    locgpu::DevBuf<locgpu::PoseState> d_state;
    locgpu::DevBuf<uint32_t> d_nn;  // [5][pitch]
    // [n_scans][ceil(max_n / 64)] run flags of the plane fit, written by the 64-lane walk kernel (SearchArgs::run_flags);
    // run_flags_written: the search stage of the batch's last Gauss–Newton iteration wrote them (launch_local_stage)
    locgpu::DevBuf<unsigned long long> d_run_flags;
    bool run_flags_written = false;
    // Shared-source batch (locgpu_batch_create_shared): ONE region of points in d_src, read by every entry — d_src_of holds a zero per
    // entry and travels as SearchArgs / AccumArgs::src_of. The buffers are sized for cap_scans entries of cap_points points; n_scans
    // and max_n are what the current call uses of them (reshape_shared, locgpu_api.hip). split_scans > 0: the accumulate kernels
    // split their sums as a plain batch of that many scans would (AccumArgs::split_scans) — a candidate search in chunks.
    bool shared_src = false;
    locgpu::DevBuf<int> d_src_of;
    int cap_scans = 0, split_scans = 0;
    size_t cap_points = 0;
    const float4* d_src_ext = nullptr;           // one-scan batches: the points stay where the caller's cloud holds them (no copy into d_src); nullptr = d_src
    bool counters_clean = false;                 // the search stage's work-list counters are known to be zero (the last alignment ran to its end)
    int last_iterations = -1;                    // one-scan batches: iterations of the previous alignment run on this batch (-1: none yet) — sizes the next first chunk
    locgpu::DevBuf<double> d_partials;  // [n_scans][blocks_per_scan][kAccW]
    locgpu::DevBuf<double> d_hb;        // [n_scans][44]
    locgpu::DevBuf<uint32_t> d_redo_list;      // [pitch]
    locgpu::DevBuf<unsigned int> d_redo_count;  // [2]: the two lists' counters
    locgpu::DevBuf<uint32_t> d_redo_list2;      // [pitch], allocated on first use of the grid search
    locgpu::DevBuf<uint32_t> d_grid_qkey;       // [pitch] grid search: tile of each query
    locgpu::DevBuf<uint2> d_grid_sorted;        // [pitch] grid search: {query, tile} in tile order
    locgpu::DevBuf<uint32_t> d_grid_tile_count; // [occupied tiles + 1] grid search: queries per occupied tile of this batch's iteration
    locgpu::DevBuf<unsigned char> d_grid_scan_temp;  // workspace of the scan over them
    // hipGraph of {H2D state, max_iteration × (search, fit+accumulate, solve), D2H state}, keyed by the launch parameters
    hipGraphExec_t graph_exec = nullptr;       // {H2D state, first chunk of iterations, D2H state}
    hipGraphExec_t graph_exec_next = nullptr;  // {further chunk, D2H state}
    locgpu::AlignSpec graph_spec;
    const void* graph_target = nullptr;  // tree / NDT table the capture was made against
    unsigned long long graph_epoch = 0;
    locgpu::PinnedBuf<float4> h_src;       // pinned staging of the packed source (single-scan path only; reused across calls)
    locgpu::Event xyz_ev[8];               // one-scan batch: the output cloud's pieces on their way back (write_output_cloud)
    locgpu::PinnedBuf<locgpu::PoseState> h_state;
    // one-scan alignments paced from the host (gn_driver.hip, align_finish): the solve kernel posts the state here after every
    // iteration — pinned COHERENT memory: [0] a finished scan's GnPostRecord, [kPostWord] call << 32 | iterations << 1 | done, [+1] checksum
    locgpu::PinnedBuf<unsigned long long> h_post;
    static constexpr int kPostWord = 16;  // in 8-byte words: behind the record, 16-byte aligned
    unsigned int post_call = 0;
    bool paced_tail = false;       // the last alignment was paced: up to pace_ahead idle launches may still be queued on `stream`
    locgpu::Event tail_ev;         // ... behind which the next upload's copies are ordered (batch_upload.hip)
    locgpu::PinnedBuf<double> h_hb;
    // locgpu_icp_align_pairs / locgpu_icp_fitness_pairs: per scan the first slot of its target's tree, formed on the host per call
    // (pair_base[i] = forest_base[target_of[i]]) and uploaded as n_scans words; pair_skip[i]: target_of[i] == -1, the scan is not aligned.
    // locgpu_ndt_align_pairs / locgpu_ndt_fitness_pairs: pair_base[i] = target_of[i], the word the kernels shift into the voxel key
    std::vector<uint32_t> pair_base;
    std::vector<unsigned char> pair_skip;
    locgpu::DevBuf<uint32_t> d_pair_base;
    locgpu::PinnedBuf<int> h_active;       // [n_scans]: local indices of the scans still open at the last chunk boundary
    locgpu::DevBuf<int> d_active;          // its device copy (see SearchArgs::active)
    std::vector<int> counts;
    locgpu::BatchUploadState upl;          // event + pinned counts of locgpu_batch_upload_async (batch_upload.hpp)
    locgpu::StageEvents stage_ev;          // profiling events of the batch's (or the pool's) iterations (locgpu_profile_enable)
    locgpu::Event ev_ready, ev_reduced;  // sharded batches: compute stream ⇄ comm stream hand-over
    // an alignment begun with *_align_batch_begin and not yet finished
    struct Pending {
        bool active = false;
        locgpu::AlignSpec spec;
        bool graph = false;
        bool paced = false;  // one scan, eager: iterations are launched as the solve kernel posts its progress
        int launched = 0;
        std::vector<double> init_poses;
    } pending;
};

namespace locgpu {

int fail(locgpu_ctx* ctx, int code, const std::string& msg);
bool hip_ok(locgpu_ctx* ctx, hipError_t e, const char* what);

// locgpu_api.hip
void ndt_free(locgpu_ctx* ctx);
// Device buffers + pinned result staging for n_scans scans of at most max_n points each; no points yet. n_total >= 0: a sharded batch.
int alloc_batch(locgpu_ctx* ctx, int n_scans, size_t max_n, locgpu_batch** out, int first = 0, int n_total = -1, bool shared_src = false);
void free_batch(locgpu_batch* b);
// Validate the matcher's options against the context's target; fill the request of an alignment.
int check_icp(locgpu_ctx* ctx, const locgpu_icp_opts* o, AlignSpec& spec);
// pairs: the request of locgpu_ndt_align_pairs, which reads a voxel-set target and nothing else; every other request reads an ordinary one
int check_ndt(locgpu_ctx* ctx, AlignSpec& spec, bool pairs = false);
// LOCGPU_ERR_INVALID with a text when the context holds a voxel-set target: the gate of every entry point that reads the NDT target as ONE grid
int refuse_ndt_set(locgpu_ctx* ctx, const char* who);
// LOCGPU_ERR_INVALID with a text when the context holds a forest target: the gate of every entry point that reads the ICP target as ONE tree
int refuse_forest(locgpu_ctx* ctx, const char* who);
// icp_target.hip
int target_join(locgpu_ctx* ctx, bool install = true);  // finishes a pending locgpu_icp_set_target_cloud_async (no-op without one)
void free_target_scratch(locgpu_ctx* ctx);              // the ingest buffers the context keeps between SetInputTarget calls
// meta = {slots, leaves, nodes, points, depth, bounded}: waits for the readers of the old target, makes room in d_tree / d_leaf_slots
// and sets the context's description of an ORDINARY target (forest_n = 0); the caller fills the arrays
int install_tree_meta(locgpu_ctx* ctx, const long long meta[6]);
void forest_build_free(locgpu_ctx* ctx);                // forest_build.hip: the device tree build's scratch (called by locgpu_destroy)
// SetInputTarget from a resident cloud of any context on ctx's GPU; async: the host tree build runs on a worker thread
int icp_set_target_from_cloud(locgpu_ctx* ctx, const locgpu_cloud* target, bool async);
int ensure_grid(locgpu_ctx* ctx);                       // the exact-search grid of the current target (built on first use)
void free_grid(locgpu_ctx* ctx);
// comm.hip: collectives over the context's communicator, in place, on stream `s`
bool comm_all_reduce_f64(locgpu_ctx* ctx, double* buf, size_t count, hipStream_t s);
bool comm_broadcast(locgpu_ctx* ctx, void* buf, size_t bytes, int root, hipStream_t s);
bool comm_all_reduce_min_int(locgpu_ctx* ctx, int* buf, hipStream_t s);
void comm_destroy(locgpu_ctx* ctx);

}  // namespace locgpu

#define LOCGPU_HIP(ctx, expr)                                                    \
    do {                                                                         \
        if (!locgpu::hip_ok((ctx), (expr), #expr)) return LOCGPU_ERR_NO_DEVICE;  \
    } while (0)
