// loc_lib_amd/csrc/gn_driver.hpp — the Gauss–Newton driver (gn_driver.hip): the local stage of one iteration, which batches and the
// scan pool share, and what the entry points of locgpu_api.hip and scan_pool.hip call around it.
#pragma once
#include "context.hpp"
#include "launch.hpp"

namespace locgpu {

// GN iterations enqueued between two host reads of the convergence flags. Kernels of a finished scan return at once (device-side
// `done` flag), so running ahead costs ≈2 µs per empty launch while a host round trip costs tens of µs: the first chunk covers the
// typical alignment (7-8 iterations with the reference's eps), later ones are shorter. (A sharded batch has one exchange buffer per
// iteration of a chunk: alloc_batch.)
constexpr int kFirstChunk = 8, kNextChunk = 4, kLongFirstChunk = 12;

inline const float4* batch_src(const locgpu_batch* b) { return b->d_src_ext ? b->d_src_ext : b->d_src; }
// The methods whose search skips the points pcl::isFinite rejects, and the distance that gates a method's correspondences.
inline bool skips_nonfinite(int method) { return method == LOCGPU_P2P || method == LOCGPU_P2PLANE_MAP; }
inline double icp_gate(const GnParams& p) {
    return (p.method == LOCGPU_P2PLANE || p.method == LOCGPU_P2PLANE_MAP) ? p.max_plane_distance : (p.method == LOCGPU_P2LINE ? p.max_line_distance : p.max_nn_distance);
}

// The local part of one Gauss–Newton iteration over the scans of storage batch `b`: what differs between a plain batch, a sharded
// batch and a scan pool. Everything else (counts, neighbour lists, work lists, partial sums, stage marks) is the storage batch's.
struct LocalStage {
    const float4* src;            // batch_src(b), or a pool's arena of regions
    PoseState* state;             // the base the kernels index: b->d_state + b->first, or a pool's slot 0
    const int* active;            // the open scans (SearchArgs::active); nullptr = all of b->n_scans
    int n_active;
    const int* src_of;            // SearchArgs::src_of
    int split_scans;              // AccumArgs::split_scans: the batch whose split of the partial sums is reproduced (0: b's own)
    const AlignSpec& spec;
    unsigned long long* visits;   // SearchArgs::visit_totals (instrumented pass), or nullptr
    const GridSearchScratch* grid;  // the grid search's work lists when the batch has them
    bool capturing;               // inside hipStreamBeginCapture: nothing may be allocated
    const char* who;              // prefix of the error text
    const uint32_t* scan_tree_base = nullptr;  // SearchArgs::scan_tree_base: a pairs alignment over a forest target (NDT: the target words over a voxel set); nullptr = the one target
};
// Enqueues search, then fit + accumulate (ICP), or the direct / incremental NDT accumulate, on `s`, with b->stage_ev's marks around
// them. Returns the number of partial blocks per scan the solve (or launch_sum_partials) must sum; < 0 on failure (fail() was called).
int launch_local_stage(locgpu_ctx* ctx, locgpu_batch* b, const LocalStage& w, hipStream_t s);

// The grid search's work lists of `b` (no-op unless spec.grid): every caller of launch_local_stage allocates them BEFORE its launches.
int ensure_grid_lists(locgpu_ctx* ctx, locgpu_batch* b, const AlignSpec& spec);

// The owner of a scan solves it ahead of the exchange, which then runs on the communication stream. LOCGPU_SHARD_DECOUPLED=0|1
// forces either way; default: with more than one rank.
bool shard_decoupled(const locgpu_ctx* ctx, bool scan_sharded);

// The search stage's arguments over storage batch `b`: tree, depth, lists and counters are the context's and the batch's; what a
// caller varies afterwards (active, src_of, visit_totals) starts empty.
SearchArgs make_search_args(const locgpu_ctx* ctx, const locgpu_batch* b, const float4* src, const PoseState* st, int k, float alpha_eff, bool skip_nonfinite);

void init_state(PoseState& ps, const double pose[7]);
// A finished scan's pose and statistics; status 1 (direct NDT aborted: the reference leaves result_pose unassigned) hands back `init`.
void write_scan_result(const PoseState& ps, const double* init, double* out_pose, locgpu_align_stats* stats);

// An alignment in two halves, so that a caller can have two batches in flight (their streams differ): align_begin enqueues the
// first chunk of iterations and returns; align_finish waits for it, enqueues further chunks while scans are still open, and
// writes the results. run_align is begin + finish back to back.
int align_begin(locgpu_ctx* ctx, locgpu_batch* b, const double* init_poses, const AlignSpec& spec, bool blocking = false);
int align_finish(locgpu_ctx* ctx, locgpu_batch* b, double* out_poses, locgpu_align_stats* stats);
int run_align(locgpu_ctx* ctx, locgpu_batch* b, const double* init_poses, const AlignSpec& spec, double* out_poses, locgpu_align_stats* stats);
// H, B, effective_num and ok of every scan of `b` at `poses` (one iteration without the update) → hb[n_total][44].
int eval_hb_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, const AlignSpec& spec, double* hb, const char* who);
// Score of every entry of `b` under its pose: k = 1 exact search stage, then the reduction of fitness.hip.
int fitness_on_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, double max_range, locgpu_fitness* out);
// The same per scan against its own tree of the context's forest (b->pair_base / pair_skip are set): a skipped scan scores {+inf, 0, 0}.
int fitness_pairs_on_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, double max_range, locgpu_fitness* out);
// Score of every entry of `b` under its pose against the context's direct NDT table (ndt_fitness.hip).
int ndt_fitness_on_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, locgpu_fitness* out);
// The same per scan against its own target of the context's voxel set (b->pair_base / pair_skip are set): a skipped scan scores {+inf, 0, 0}.
int ndt_fitness_pairs_on_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, locgpu_fitness* out);
// The plane table of LOCGPU_P2PLANE_MAP for the current target (map_planes.hip); no-op when it is there.
int ensure_map_planes(locgpu_ctx* ctx);

}  // namespace locgpu
