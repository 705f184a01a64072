// loc_lib_amd/csrc/gn_driver.hip — the Gauss–Newton driver: one iteration's launch sequence, chunks, graphs, pacing, results.
//
// One iteration is "search → fit/accumulate → (exchange) → solve" on one HIP stream, and the convergence test lives on the device, so
// the host only reads back the small per-scan state every chunk of iterations. The local part of the iteration (launch_local_stage)
// is the same code for plain batches, sharded batches and the scan pool (scan_pool.hip); the exchange-and-solve tail is the caller's.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

#include "batch_upload.hpp"
#include "env.hpp"
#include "gn_driver.hpp"
#include "ndt_inc.hpp"
#include "ndt_kernels.hpp"
#include "stream_lease.hpp"

namespace locgpu {

namespace {
// A one-scan alignment follows its first chunk with chunks of two: there a chunk boundary (read-back, host, relaunch ≈ 35 µs) costs
// about what two idle iterations do (3 dispatches of ≈4.6 µs each), and nine iterations — the common case beyond eight — then pay
// 35 + 15 µs instead of 35 + 45 (tools/single_scan_trace.py).
inline int next_chunk(const locgpu_batch* b) { return b->n_total == 1 ? 2 : kNextChunk; }
// ... and sizes its FIRST chunk by the alignment it ran before: a front-end that matches every scan from a good prediction
// (Lio::AddCloud: 4-5 iterations per scan) used to pay three or four idle iterations, ≈15 µs each, in every call — a sixth of the
// match stage of the streaming loop (tools/stream_trace.py). One more than last time, between 3 and kFirstChunk; chunking never
// changes a result (the same kernels run on the same data in the same order), only where the host looks at the flags.
inline int first_chunk_len(const locgpu_batch* b) {
    if (b->n_total != 1 || b->sharded || b->last_iterations < 0) return kFirstChunk;
    // ... up to kLongFirstChunk when the last call needed more than eight: a chunk boundary there cost 33 µs + two idle iterations (round 5)
    return std::min(kLongFirstChunk, std::max(3, b->last_iterations + 1));
}

}  // namespace

// The search stage's arguments over storage batch `b`: tree, depth, lists and counters are the context's and the batch's; what a
// caller varies afterwards (active, src_of, visit_totals) starts empty.
SearchArgs make_search_args(const locgpu_ctx* ctx, const locgpu_batch* b, const float4* src, const PoseState* st, int k, float alpha_eff, bool skip_nonfinite) {
    SearchArgs sa{ctx->d_tree, ctx->tree_slots * sizeof(uint64_t), ctx->depth, src, b->d_counts, st, b->d_nn, b->pitch, b->max_n, b->n_scans, k, alpha_eff,
                  skip_nonfinite ? 1 : 0, nullptr, b->d_redo_list, b->d_redo_count, b->d_redo_list2, b->d_redo_count + 1, ctx->d_search_stats};
    if (!ctx->tree_bounded) sa.redo_list = nullptr;  // huge / non-finite map coordinates: exact tree kernel only
    return sa;
}

// LOCGPU_PLANE_RUNFLAGS (read once): 1 (default) = the 64-lane walk kernel of a P2Plane search marks the runs of equal neighbour sets
// for the plane kernel (SearchArgs::run_flags → AccumArgs::run_flags); 0 = it writes none and the plane kernel finds the runs itself
// (measurement hook: the two give the same bits).
static bool plane_run_flags() {
    static const bool on = env_int("LOCGPU_PLANE_RUNFLAGS", 1) != 0;
    return on;
}

void init_state(PoseState& ps, const double pose[7]) {
    std::memset(&ps, 0, sizeof(ps));
    for (int i = 0; i < 4; ++i) ps.q[i] = pose[i];
    for (int i = 0; i < 3; ++i) ps.t[i] = pose[4 + i];
    quat_to_R(ps.q, ps.R);
}

static void init_states(locgpu_batch* b, const double* poses) {
    for (int s = 0; s < b->n_total; ++s) init_state(b->h_state[s], poses + 7 * (size_t)s);  // an empty scan still runs the loop: effective_num < min ⇒ no-op iterations
}

void write_scan_result(const PoseState& ps, const double* init, double* out_pose, locgpu_align_stats* stats) {
    if (ps.status == 1) {
        for (int j = 0; j < 7; ++j) out_pose[j] = init[j];
    } else {
        for (int j = 0; j < 4; ++j) out_pose[j] = ps.q[j];
        for (int j = 0; j < 3; ++j) out_pose[4 + j] = ps.t[j];
    }
    if (!stats) return;
    stats->iterations = ps.iterations; stats->converged = ps.converged; stats->status = ps.status; stats->reserved = 0;
    stats->last_effective_num = ps.last_eff; stats->last_dx_norm = ps.last_dx_norm;
}

bool shard_decoupled(const locgpu_ctx* ctx, bool scan_sharded) {
    static const int env = env_int("LOCGPU_SHARD_DECOUPLED", -1);
    return ctx->comm && scan_sharded && (env >= 0 ? env != 0 : ctx->comm_world > 1);
}

void StageEvents::mark(hipStream_t s, bool search_edge) {
    if (!mode || (mode == 2 && !search_edge)) return;
    if (ev.size() <= used) {
        Event e;
        if (e.ensure(hipEventDefault) != hipSuccess) return;
        ev.push_back(std::move(e));
    }
    (void)hipEventRecord(ev[used++], s);
}

void StageEvents::collect(locgpu_ctx* ctx, bool ndt) {
    // mode 1: four marks per iteration — [0,1] search, [1,2] fit + accumulate, [2,3] solve (and exchange); mode 2: two — [0,1] search
    const size_t per = mode == 2 ? 2 : 4;
    for (size_t i = 0; i + per - 1 < used; i += per)
        for (size_t j = 0; j + 1 < per; ++j) {
            if (ndt && j == 0) continue;  // NDT has no search kernel: the slot stays empty
            float ms = 0.f;
            if (hipEventElapsedTime(&ms, ev[i + j], ev[i + j + 1]) == hipSuccess) { ctx->prof_ms[j] += ms; ctx->prof_n[j] += 1; }
        }
    used = 0;
}

int launch_local_stage(locgpu_ctx* ctx, locgpu_batch* b, const LocalStage& w, hipStream_t s) {
    StageEvents& ev = b->stage_ev;
    int n_partial_blocks = b->blocks_per_scan;
    ev.mark(s, true);
    if (b->n_scans == 0 || (w.active && w.n_active == 0)) {
        ev.mark(s, true);  // nothing local: this rank only takes part in the exchange that follows
    } else if (!w.spec.ndt()) {
        const GnParams& prm = w.spec.prm;
        SearchArgs sa = make_search_args(ctx, b, w.src, w.state, w.spec.k(), w.spec.alpha, skips_nonfinite(prm.method));
        const bool grid_mode = w.spec.grid && ctx->tree_bounded;
        if (grid_mode && !w.grid) { fail(ctx, LOCGPU_ERR_INVALID, "grid search: work list missing (ensure_grid_lists was not called)"); return -1; }
        sa.visit_totals = w.visits;
        sa.active = w.active; sa.n_active = w.n_active;
        sa.src_of = w.src_of;
        sa.scan_tree_base = w.scan_tree_base;
        if (sa.visit_totals && !w.capturing) {  // instrumented pass: which tree slots does this launch read at all? (bench.py: compulsory bytes)
            const size_t words = (ctx->tree_slots + 2 + 31) / 32;
            if (words > ctx->touched_words) {
                ctx->touched_words = 0;
                if (ctx->d_touched.alloc(words) == hipSuccess && hipMemsetAsync(ctx->d_touched, 0, words * sizeof(uint32_t), s) == hipSuccess)
                    ctx->touched_words = words;
            }
            sa.touched = ctx->touched_words ? ctx->d_touched.get() : nullptr;
        }
        // only the plane kernel reads run flags (the line kernel's search has k = 5 too); the grid search writes none
        if (prm.method == LOCGPU_P2PLANE && plane_run_flags()) sa.run_flags = b->d_run_flags;
        bool wrote_flags = false;
        const bool ok_search = (grid_mode && !sa.visit_totals) ? launch_icp_search_grid(ctx->grid, sa, *w.grid, s) : launch_icp_search(sa, s, &wrote_flags);
        b->run_flags_written = wrote_flags;
        if (!ok_search) { fail(ctx, LOCGPU_ERR_DEPTH, std::string(w.who) + ": unsupported k/depth"); return -1; }
        if (sa.touched) launch_count_touched(sa.touched, (ctx->tree_slots + 2 + 31) / 32, sa.visit_totals, s);
        ev.mark(s, true);
        AccumArgs aa{ctx->d_tree, w.src, b->d_counts, w.state, b->d_nn, b->pitch, b->max_n, b->n_scans, icp_gate(prm), b->d_partials};
        aa.planes = ctx->d_planes;
        aa.active = w.active; aa.n_active = w.n_active;
        aa.src_of = w.src_of;
        aa.split_scans = w.split_scans;
        if (wrote_flags && prm.method == LOCGPU_P2PLANE) aa.run_flags = b->d_run_flags;
        n_partial_blocks = launch_icp_accum(prm.method, aa, s);
    } else {
        ev.mark(s, true);  // NDT has no separate search kernel: the search slot stays empty
        if (w.spec.prm.method == kMethodNdtInc)
            launch_inc_accum(ctx->inc, ctx->ndt_opts.res_outlier_th, ndt_n_nearby(ctx->ndt_opts.nearby_type), w.src, b->d_counts, w.state, b->max_n, b->n_scans, b->d_partials, s,
                             w.active, w.n_active, w.src_of);
        else
            n_partial_blocks = launch_ndt_accum(ctx->ndt, w.src, b->d_counts, w.state, b->max_n, b->n_scans, b->d_partials, s, w.active, w.n_active, w.split_scans, w.src_of,
                                                w.spec.pairs ? w.scan_tree_base : nullptr);
    }
    ev.mark(s);
    return n_partial_blocks;
}

struct IterLauncher {
    locgpu_ctx* ctx;
    locgpu_batch* b;
    const AlignSpec& spec;
    bool capturing = false;  // inside hipStreamBeginCapture: no event records
    int slot = 0;            // sharded batches: which of the chunk's exchange buffers this iteration uses
    bool replicated_on_comm_stream = false;  // the chunk's read-back must wait for the communication stream as well
    const int* active = nullptr;  // later chunks: the local scans still open (SearchArgs::active); nullptr = all
    int n_active = 0;
    const GnPost* post = nullptr;  // paced one-scan alignment: the solve kernel posts the state to the host
    // One GN iteration = search + accumulate + solve. Returns false on a launch error.
    bool launch(int do_update);
};

bool IterLauncher::launch(int do_update) {
    hipStream_t s = b->stream;
    const GnParams& prm = spec.prm;
    const bool ndt = spec.ndt();
    StageEvents& ev = b->stage_ev;
    ev.mode = capturing ? 0 : ctx->profile;
    const GridSearchScratch gsc{b->d_grid_qkey, b->d_grid_sorted, b->d_grid_tile_count, b->d_grid_scan_temp};
    // Kernels index the scans this rank holds, 0..n_scans-1. A candidate search in chunks sums as the plain batch of all candidates,
    // and a rank of a scan-sharded batch splits the partial sums as the WHOLE batch would (points per thread follow the batch's size):
    // the order of a scan's additions — hence its bits — must not depend on how many ranks share the batch (found by the eight-rank
    // loopback run of round 6: 32 of 256 scans per rank summed one point per thread where the plain batch sums four)
    const LocalStage w{batch_src(b), b->d_state + b->first, active, n_active, b->d_src_of, b->sharded ? b->n_total : b->split_scans, spec,
                       ctx->count_visits ? ctx->d_visits : nullptr, b->d_grid_qkey ? &gsc : nullptr, capturing, "search", spec.pairs ? b->d_pair_base.get() : nullptr};
    const int n_partial_blocks = launch_local_stage(ctx, b, w, s);
    if (n_partial_blocks < 0) return false;
    // The exchange-and-solve tail. Against the pool's (scan_pool.hip): contiguous ranges [first, first + n_scans) instead of two slot
    // lists, LOCGPU_COMM_DIRECT, one exchange buffer per iteration of the first chunk.
    if (b->sharded) {
        // The exchange step of the sharded mode: per scan 28 sums (21 H + 6 B + effective_num), zeros from the
        // ranks that do not hold the scan, summed over xGMI on this stream; then every rank solves every scan, so all ranks see the
        // same convergence flags and stay in lock-step.
        double* acc = b->d_acc + (size_t)(slot % kFirstChunk) * b->n_total * kAccW;
        slot++;
        launch_sum_partials(b->d_partials, n_partial_blocks, b->d_state, b->first, b->n_scans, b->n_total, acc, s);
        // Scan-sharded over several ranks: a scan's sums are complete on the rank that holds it (everybody else adds zeros), so the
        // OWNER solves its scans at once and goes on to the next search, while the all-reduce — on the context's communication
        // stream — only replicates: behind it every rank solves the scans it does not hold, from the reduced sums, and ends up with
        // the same poses and flags as their owners. The network is off the Gauss–Newton loop's critical path; the host looks at the
        // flags of ALL scans only between chunks (both streams joined), which keeps the ranks' collective counts in lock-step.
        // Point-sharded batches (every rank holds a slice of every scan) and H/B evaluations need the sum itself: they wait.
        if (do_update && shard_decoupled(ctx, b->n_scans != b->n_total)) {
            hipStream_t cs = ctx->comm_stream;
            if (b->n_scans > 0)
                launch_gn_solve(acc + (size_t)b->first * kAccW, 1, b->d_state + b->first, b->n_scans, prm, do_update, b->d_hb + (size_t)b->first * 44,
                                ndt ? nullptr : b->d_redo_count, s);
            if (!hip_ok(ctx, hipEventRecord(b->ev_ready, s), "sharded: hipEventRecord") || !hip_ok(ctx, hipStreamWaitEvent(cs, b->ev_ready, 0), "sharded: hipStreamWaitEvent")) return false;
            if (!comm_all_reduce_f64(ctx, acc, (size_t)b->n_total * kAccW, cs)) return false;
            const int after = b->first + b->n_scans;
            if (b->first > 0) launch_gn_solve(acc, 1, b->d_state, b->first, prm, do_update, b->d_hb, nullptr, cs);
            if (after < b->n_total)
                launch_gn_solve(acc + (size_t)after * kAccW, 1, b->d_state + after, b->n_total - after, prm, do_update, b->d_hb + (size_t)after * 44, nullptr, cs);
            replicated_on_comm_stream = true;
            ev.mark(s);
            return hip_ok(ctx, hipGetLastError(), "kernel launch");
        }
        if (ctx->comm) {
            // Every collective of the context goes through ONE stream in host order — the order is the same on every rank because
            // every rank sees the same convergence flags — so two batches in flight never have two collectives of the one
            // communicator racing each other.
            // (A one-rank communicator has nobody to disagree with about the order: its collective stays on the batch's own stream —
            // 32 scans per step, two in flight: 8500 scans/s against 5700 through the comm stream, whose in-order queue makes the
            // second batch's first exchange wait for the first batch's whole chunk. LOCGPU_COMM_DIRECT=0/1 forces either way.)
            static const int force = env_int("LOCGPU_COMM_DIRECT", -1);
            const bool direct = force >= 0 ? force != 0 : ctx->comm_world == 1;
            hipStream_t cs = direct ? s : ctx->comm_stream;
            if (!direct && (!hip_ok(ctx, hipEventRecord(b->ev_ready, s), "sharded: hipEventRecord") || !hip_ok(ctx, hipStreamWaitEvent(cs, b->ev_ready, 0), "sharded: hipStreamWaitEvent"))) return false;
            if (!comm_all_reduce_f64(ctx, acc, (size_t)b->n_total * kAccW, cs)) return false;
            if (!direct && (!hip_ok(ctx, hipEventRecord(b->ev_reduced, cs), "sharded: hipEventRecord") || !hip_ok(ctx, hipStreamWaitEvent(s, b->ev_reduced, 0), "sharded: hipStreamWaitEvent"))) return false;
        }
        launch_gn_solve(acc, 1, b->d_state, b->n_total, prm, do_update, b->d_hb, ndt ? nullptr : b->d_redo_count, s);
    } else {
        launch_gn_solve(b->d_partials, n_partial_blocks, b->d_state, b->n_scans, prm, do_update, b->d_hb, ndt ? nullptr : b->d_redo_count, s, nullptr, post);
    }
    ev.mark(s);
    return hip_ok(ctx, hipGetLastError(), "kernel launch");
}

// A pending locgpu_batch_upload_async of `b`: wait until the host side is through, then order the compute stream behind the copies.
static int batch_ready(locgpu_ctx* ctx, locgpu_batch* b) {
    const int rc = upload_join_batch(b);
    if (rc != LOCGPU_OK) return rc;
    LOCGPU_HIP(ctx, upload_order_after(b, b->stream));
    return LOCGPU_OK;
}

// The grid search hands its leftovers through a second work list. It is allocated here, by every entry point that may run the
// grid search on `b`, BEFORE any launch: launch() can run under hipStreamBeginCapture, where hipMalloc is not allowed.
int ensure_grid_lists(locgpu_ctx* ctx, locgpu_batch* b, const AlignSpec& spec) {
    if (!spec.grid) return LOCGPU_OK;
    if (!b->d_grid_qkey) {
        LOCGPU_HIP(ctx, b->d_grid_qkey.alloc(b->pitch));
        LOCGPU_HIP(ctx, b->d_grid_sorted.alloc(b->pitch));
    }
    // the binning's per-tile counts and scan workspace are the batch's own as well (several alignments run at once); sized by the
    // current target's grid — a new target may have more occupied tiles
    const size_t tocc = ctx->grid.n_tocc, scan = std::max<size_t>(ctx->grid.scan_temp_bytes, 1);
    if (b->d_grid_tile_count.cap() < tocc + 1) {
        LOCGPU_HIP(ctx, hipStreamSynchronize(b->stream));
        LOCGPU_HIP(ctx, b->d_grid_tile_count.alloc(tocc + 1));
    }
    if (b->d_grid_scan_temp.cap() < scan) {
        LOCGPU_HIP(ctx, hipStreamSynchronize(b->stream));
        LOCGPU_HIP(ctx, b->d_grid_scan_temp.alloc(scan));
    }
    return LOCGPU_OK;
}

// hipGraph path (BASELINE config 5): the Gauss–Newton iterations are captured once — the kernels early-out per scan on the
// device-side `done` flag, so a fixed node sequence gives the same result as the data-dependent eager loop — and replayed per call.
// Two graphs mirror the eager loop's chunks: graph 0 = {H2D state, kFirstChunk iterations, D2H state} covers the typical alignment
// with one launch and one host synchronisation; graph 1 = {kNextChunk iterations, D2H state} is replayed while scans are still
// open (capturing all max_iteration iterations in one graph made every call pay a dozen empty iterations).
static int capture_chunk(locgpu_ctx* ctx, locgpu_batch* b, const AlignSpec& spec, int iters, bool with_h2d, hipGraphExec_t* out) {
    hipStream_t s = b->stream;
    hipGraph_t graph = nullptr;
    LOCGPU_HIP(ctx, hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
    bool ok = !with_h2d || hip_ok(ctx, hipMemcpyAsync(b->d_state, b->h_state, b->n_total * sizeof(PoseState), hipMemcpyHostToDevice, s), "capture H2D");
    IterLauncher it{ctx, b, spec};
    it.capturing = true;
    for (int i = 0; ok && i < iters; ++i) ok = it.launch(1);
    ok = ok && hip_ok(ctx, hipMemcpyAsync(b->h_state, b->d_state, b->n_total * sizeof(PoseState), hipMemcpyDeviceToHost, s), "capture D2H");
    const hipError_t e = hipStreamEndCapture(s, &graph);
    if (!ok || !hip_ok(ctx, e, "hipStreamEndCapture")) { if (graph) (void)hipGraphDestroy(graph); return LOCGPU_ERR_NO_DEVICE; }
    const bool inst = hip_ok(ctx, hipGraphInstantiate(out, graph, nullptr, nullptr, 0), "hipGraphInstantiate");
    (void)hipGraphDestroy(graph);
    if (!inst) { *out = nullptr; return LOCGPU_ERR_NO_DEVICE; }
    return LOCGPU_OK;
}

static int ensure_graphs(locgpu_ctx* ctx, locgpu_batch* b, const AlignSpec& spec) {
    const void* target = !spec.ndt() ? (const void*)ctx->d_tree : (spec.prm.method == kMethodNdtInc ? inc_ndt_table_ptr(ctx->inc) : (const void*)ctx->ndt->d_rec);
    if (b->graph_exec && b->graph_spec == spec && b->graph_target == target && b->graph_epoch == ctx->target_epoch) return LOCGPU_OK;
    const int first = std::min(kFirstChunk, spec.prm.max_iteration);
    if (b->graph_exec) { (void)hipGraphExecDestroy(b->graph_exec); b->graph_exec = nullptr; }
    if (b->graph_exec_next) { (void)hipGraphExecDestroy(b->graph_exec_next); b->graph_exec_next = nullptr; }
    int rc = capture_chunk(ctx, b, spec, first, true, &b->graph_exec);
    if (rc == LOCGPU_OK && spec.prm.max_iteration > first) rc = capture_chunk(ctx, b, spec, next_chunk(b), false, &b->graph_exec_next);
    if (rc != LOCGPU_OK) return rc;
    b->graph_spec = spec; b->graph_target = target;
    b->graph_epoch = ctx->target_epoch;
    return LOCGPU_OK;
}

// One chunk of iterations + the read-back of the per-scan states behind it, on the batch's stream, and the batch's event behind that.
static int enqueue_chunk(locgpu_ctx* ctx, locgpu_batch* b, bool first_chunk) {
    locgpu_batch::Pending& P = b->pending;
    const GnParams& prm = P.spec.prm;
    hipStream_t s = b->stream;
    if (P.graph) {
        // kernels of a finished scan return at once and the solve kernel stops at max_iteration, so a whole chunk is always safe
        LOCGPU_HIP(ctx, hipGraphLaunch(first_chunk ? b->graph_exec : b->graph_exec_next, s));  // on whatever stream the batch holds now: a graph's nodes keep nothing of the capture stream
        P.launched += first_chunk ? std::min(kFirstChunk, prm.max_iteration) : next_chunk(b);
        LOCGPU_HIP(ctx, hipEventRecord(b->chunk_ev, s));
        return LOCGPU_OK;
    }
    if (first_chunk) LOCGPU_HIP(ctx, hipMemcpyAsync(b->d_state, b->h_state, b->n_total * sizeof(PoseState), hipMemcpyHostToDevice, s));
    IterLauncher it{ctx, b, P.spec};
    if (!first_chunk && !P.spec.ndt() && b->n_scans > 1) {
        // The host has just read every scan's flags (align_finish): launch the search and accumulate kernels of this chunk over the
        // local scans still open only. A 256-scan step's second and third chunk hold ≈60 and ≈5 scans; the rest used to be 1800
        // early-exit workgroups per scan and kernel (≈96 µs per search launch for nothing). Results are the same bits: a scan's
        // blocks do the same work wherever blockIdx.y finds it, and the accumulate kernels' split does not depend on the list.
        int na = 0;
        for (int i = 0; i < b->n_scans; ++i)
            if (!b->h_state[b->first + i].done) b->h_active[na++] = i;
        if (na > 0 && na < b->n_scans) {
            LOCGPU_HIP(ctx, hipMemcpyAsync(b->d_active, b->h_active, (size_t)na * sizeof(int), hipMemcpyHostToDevice, s));
            it.active = b->d_active;
            it.n_active = na;
        }
    }
    const int todo = std::min(first_chunk ? first_chunk_len(b) : next_chunk(b), prm.max_iteration - P.launched);
    for (int c = 0; c < todo; ++c)
        if (!it.launch(1)) return LOCGPU_ERR_NO_DEVICE;
    P.launched += todo;
    if (it.replicated_on_comm_stream) {  // the states of the scans other ranks hold are written on the communication stream
        LOCGPU_HIP(ctx, hipEventRecord(b->ev_reduced, ctx->comm_stream));
        LOCGPU_HIP(ctx, hipStreamWaitEvent(s, b->ev_reduced, 0));
    }
    LOCGPU_HIP(ctx, hipMemcpyAsync(b->h_state, b->d_state, b->n_total * sizeof(PoseState), hipMemcpyDeviceToHost, s));
    LOCGPU_HIP(ctx, hipEventRecord(b->chunk_ev, s));  // what align_finish waits for
    return LOCGPU_OK;
}

// A ONE-SCAN alignment is paced from the host instead of chunked: the solve kernel posts the scan's state and an iteration word to
// pinned host memory (GnPost, icp_fit.hip); the host keeps `ahead` iterations queued behind the one that is running and launches
// the next when a post arrives. Against chunks (first_chunk_len / next_chunk above, still what graphs and batches use) a call no
// longer pays the idle iterations of a chunk that was sized by the previous call (≈14 µs each: three dispatches that find `done`),
// nor a chunk boundary (read-back + host + relaunch ≈ 33 µs) when the guess was short, nor the copy and the stream synchronisation
// at the end: the result is in host memory when the done bit arrives. At most `ahead` idle iterations stay queued behind a finished
// call; they return on the `done` flag before they read anything (an upload or the next call's state copy may follow at once).
// Same kernels on the same data in the same order: results are the chunked path's bits. LOCGPU_PACE_AHEAD=0 switches it off.
inline int pace_ahead() {
    static const int v = std::max(0, std::min(8, env_int("LOCGPU_PACE_AHEAD", 1)));
    return v;
}

static int paced_launch(locgpu_ctx* ctx, locgpu_batch* b, int upto) {
    locgpu_batch::Pending& P = b->pending;
    IterLauncher it{ctx, b, P.spec};
    const GnPost post{reinterpret_cast<GnPostRecord*>(b->h_post.get()), b->h_post + locgpu_batch::kPostWord, b->post_call};
    it.post = &post;
    while (P.launched < upto) {
        if (!it.launch(1)) return LOCGPU_ERR_NO_DEVICE;
        P.launched++;
    }
    return LOCGPU_OK;
}

// Wait for a post of this call that is newer than iteration `seen`; returns the word. A post with the done bit is taken only when the
// state behind it is complete (its checksum matches what this thread reads: the kernel's stores carry no fence).
constexpr int kPacedTimeoutS = 30;  // an iteration of the largest alignment this path takes (one scan) lasts well under a millisecond
static int paced_wait(locgpu_ctx* ctx, locgpu_batch* b, int seen, unsigned long long* out) {
    auto fresh = [&](unsigned long long* w_out) {
        unsigned long long w;
        GnPostRecord r;
        if (!gn_post_take(b->h_post, locgpu_batch::kPostWord, b->post_call, seen, &w, &r)) return false;
        if (w & 1ull) {
            PoseState& ps = b->h_state[0];
            for (int i = 0; i < 4; ++i) std::memcpy(&ps.q[i], &r.w[i], 8);
            for (int i = 0; i < 3; ++i) std::memcpy(&ps.t[i], &r.w[4 + i], 8);
            quat_to_R(ps.q, ps.R);
            std::memcpy(&ps.last_dx_norm, &r.w[7], 8);
            ps.last_eff = (long long)r.w[8];
            ps.iterations = (int)((w & 0xffffffffull) >> 1);
            ps.converged = (int)(r.w[9] >> 32);
            ps.status = (int)(r.w[9] & 0xffffffffull);
            ps.done = 1;
        }
        *w_out = w;
        return true;
    };
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned long spins = 1;; ++spins) {
        if (fresh(out)) return LOCGPU_OK;
#if defined(__x86_64__)
        __builtin_ia32_pause();  // a polite spin: the sibling hyper-thread (the uploader, the helper thread) gets the core's issue slots
#endif
        if ((spins & 0xffff) == 0 && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(200)) {
            // nothing for a long time: is the stream still working? An idle stream with no post means a kernel died or the posts do
            // not reach the host. (Not earlier: a stream query is a runtime call on the latency path.)
            const hipError_t q = hipStreamQuery(b->stream);
            if (q == hipErrorNotReady) {
                // a stream that stays busy without ever posting (a hung kernel) must not spin a core for ever: give up after kPacedTimeoutS
                if (std::chrono::steady_clock::now() - t0 > std::chrono::seconds(kPacedTimeoutS))
                    return fail(ctx, LOCGPU_ERR_NO_DEVICE, "paced alignment: no post from the solve kernel within the time-out (the stream is still busy)");
                std::this_thread::yield();
                continue;
            }
            if (q != hipSuccess) { hip_ok(ctx, q, "paced alignment"); return LOCGPU_ERR_NO_DEVICE; }
            if (fresh(out)) return LOCGPU_OK;
            return fail(ctx, LOCGPU_ERR_NO_DEVICE, "paced alignment: the stream is idle and the solve kernel's post has not arrived");
        }
    }
}

// The compute stream of the alignment about to begin on `b` (stream_lease.hpp): the batch's own while no other alignment in flight
// is on it, else the least-loaded one — b->slot and b->stream follow. Nothing of the batch is queued on the stream it leaves: every
// entry point that works on a batch waits for that work on the host before it returns, an ended alignment included (align_finish)
// — except the idle launches of a paced one-scan alignment (paced_tail), behind which the new stream is ordered. (NOT behind the old
// stream as a whole: the alignment in flight there is the reason for the move, and waiting for it is what the move avoids.)
static int lease_take(locgpu_ctx* ctx, locgpu_batch* b) {
    if (b->pinned) return LOCGPU_OK;
    const int to = lease_choose(ctx->slot_load, locgpu_ctx::kSlots, b->slot);
    if (to != b->slot) {
        if (b->paced_tail) {
            LOCGPU_HIP(ctx, b->tail_ev.ensure());
            LOCGPU_HIP(ctx, hipEventRecord(b->tail_ev, b->stream));
            LOCGPU_HIP(ctx, hipStreamWaitEvent(ctx->slot_stream[to], b->tail_ev, 0));
        }
        b->slot = to;
        b->stream = ctx->slot_stream[to];
    }
    ctx->slot_load[to]++;
    b->leased = true;
    return LOCGPU_OK;
}

static void lease_release(locgpu_ctx* ctx, locgpu_batch* b) {
    if (!b->leased) return;
    ctx->slot_load[b->slot]--;
    b->leased = false;
}

// The per-scan words of a pairs call (b->pair_base, formed by the entry point: ICP tree bases, NDT target indices) → b->d_pair_base, on
// the batch's stream.
static int upload_pair_base(locgpu_ctx* ctx, locgpu_batch* b) {
    if (b->d_pair_base.cap() < (size_t)b->n_scans) {
        LOCGPU_HIP(ctx, hipStreamSynchronize(b->stream));
        LOCGPU_HIP(ctx, b->d_pair_base.alloc((size_t)b->n_scans));
    }
    // pageable source: the copy has left the host array when the call returns
    LOCGPU_HIP(ctx, hipMemcpyAsync(b->d_pair_base, b->pair_base.data(), (size_t)b->n_scans * sizeof(uint32_t), hipMemcpyHostToDevice, b->stream));
    return LOCGPU_OK;
}

static int begin_on_stream(locgpu_ctx* ctx, locgpu_batch* b, const double* init_poses, const AlignSpec& spec, bool blocking) {
    const GnParams& prm = spec.prm;
    const bool ndt = spec.ndt();
    locgpu_batch::Pending& P = b->pending;
    LOCGPU_HIP(ctx, b->chunk_ev.ensure());
    if (!ndt) { const int grc = ensure_grid_lists(ctx, b, spec); if (grc != LOCGPU_OK) return grc; }
    { const int urc = batch_ready(ctx, b); if (urc != LOCGPU_OK) return urc; }
    P.spec = spec;
    P.graph = ctx->use_graph && !ctx->count_visits && !b->sharded && prm.max_iteration > 0 && !spec.pairs;  // a pairs alignment is eager whatever locgpu_graph_enable was told
    P.launched = 0;
    b->stage_ev.used = 0;
    P.init_poses.assign(init_poses, init_poses + 7 * (size_t)b->n_total);
    init_states(b, init_poses);
    if (spec.pairs) {
        // a scan without a target is done before the first iteration: no kernel touches it, its pose stays its init
        for (int i = 0; i < b->n_scans; ++i)
            if (b->pair_skip[i]) { b->h_state[i].done = 1; b->h_state[i].status = LOCGPU_STATUS_NO_PAIR_TARGET; }
        const int prc = upload_pair_base(ctx, b);
        if (prc != LOCGPU_OK) return prc;
    }
    // the search stage's work-list counters: zero once per alignment, whatever an earlier call that failed between a search and
    // its solve kernel left behind (the solve kernel re-zeroes them after every search)
    if (!ndt && !b->counters_clean) LOCGPU_HIP(ctx, hipMemsetAsync(b->d_redo_count, 0, 4 * sizeof(unsigned int), b->stream));
    b->counters_clean = false;  // until this alignment has run to its end
    if (P.graph) { const int rc = ensure_graphs(ctx, b, spec); if (rc != LOCGPU_OK) return rc; }
    // (a blocking call only: between a begin and its end the host is elsewhere, and a chunk keeps the GPU busy meanwhile)
    P.paced = blocking && !P.graph && b->n_total == 1 && !b->sharded && !ctx->profile && !ctx->count_visits && prm.max_iteration > 0 && pace_ahead() > 0 && !spec.grid &&
              !spec.pairs;  // a scan without a target is done from the start: its solve kernel would never post
    if (P.paced) {
        if (!b->h_post) {
            LOCGPU_HIP(ctx, b->h_post.alloc(256 / sizeof(unsigned long long), hipHostMallocCoherent));
            std::memset(b->h_post, 0, 256);
        }
        b->post_call++;  // posts carry the call's number: a word left by the previous call is not this call's
        LOCGPU_HIP(ctx, hipMemcpyAsync(b->d_state, b->h_state, sizeof(PoseState), hipMemcpyHostToDevice, b->stream));
        const int rc = paced_launch(ctx, b, std::min(prm.max_iteration, 1 + pace_ahead()));
        if (rc != LOCGPU_OK) { (void)hipStreamSynchronize(b->stream); return rc; }
    } else if (prm.max_iteration > 0) {
        const int rc = enqueue_chunk(ctx, b, true);
        if (rc != LOCGPU_OK) return rc;
    }
    P.active = true;
    return LOCGPU_OK;
}

int align_begin(locgpu_ctx* ctx, locgpu_batch* b, const double* init_poses, const AlignSpec& spec, bool blocking) {
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "align: an alignment of this batch has been begun and not finished");
    // the stream first: batch_ready orders it behind the batch's upload
    { const int lrc = lease_take(ctx, b); if (lrc != LOCGPU_OK) return lrc; }
    const int rc = begin_on_stream(ctx, b, init_poses, spec, blocking);
    if (rc != LOCGPU_OK) {
        // nothing of a failed begin may run on under the batch's next upload, or on a stream the batch no longer holds
        (void)hipStreamSynchronize(b->stream);
        lease_release(ctx, b);
    }
    return rc;
}

static int finish_on_stream(locgpu_ctx* ctx, locgpu_batch* b, double* out_poses, locgpu_align_stats* stats) {
    locgpu_batch::Pending& P = b->pending;
    const int max_iteration = P.spec.prm.max_iteration;
    if (P.paced) {
        int seen = 0;
        for (;;) {
            unsigned long long w = 0;
            int rc = paced_wait(ctx, b, seen, &w);
            if (rc == LOCGPU_OK) {
                seen = (int)((w & 0xffffffffull) >> 1);
                if ((w & 1ull) || seen >= max_iteration) break;
                rc = paced_launch(ctx, b, std::min(max_iteration, seen + 1 + pace_ahead()));
            }
            if (rc != LOCGPU_OK) { (void)hipStreamSynchronize(b->stream); return rc; }
        }
        b->paced_tail = true;
    }
    while (!P.paced && max_iteration > 0) {
        // the batch's own event where the stream carries another alignment as well (more in flight than streams, or a one-scan call
        // beside a batch on the context's stream): that one's chunks may be queued behind this one's, and ending this alignment must
        // not wait for them. Alone on its stream, the stream's own wait is the same thing and returns sooner: with two alignments in
        // flight the host's wake-up is on the critical path, and waiting for the event there cost 0.2-1.7 ms per 256-scan step
        // (profiles/stream_lease.md).
        const bool shared = ctx->slot_load[b->slot] > (b->leased ? 1 : 0);
        if (const hipError_t e = shared ? hipEventSynchronize(b->chunk_ev) : hipStreamSynchronize(b->stream); e != hipSuccess) {
            (void)hipStreamSynchronize(b->stream);
            hip_ok(ctx, e, "align: waiting for the chunk");
            return LOCGPU_ERR_NO_DEVICE;
        }
        b->stage_ev.collect(ctx, P.spec.ndt());
        bool all_done = true;
        for (int i = 0; i < b->n_total; ++i)
            if (!b->h_state[i].done) { all_done = false; break; }
        if (all_done || P.launched >= max_iteration) break;
        const int rc = enqueue_chunk(ctx, b, false);
        if (rc != LOCGPU_OK) {
            // whatever of the chunk was enqueued must not run on under the batch's next upload (which relies on an ended alignment
            // leaving nothing of the batch queued, batch_upload.hip)
            (void)hipStreamSynchronize(b->stream);
            return rc;
        }
    }
    for (int i = 0; i < b->n_total; ++i) write_scan_result(b->h_state[i], P.init_poses.data() + 7 * (size_t)i, out_poses + 7 * (size_t)i, stats ? stats + i : nullptr);
    b->counters_clean = !P.spec.ndt() && !ctx->count_visits && !P.spec.grid && !b->sharded;  // every search was followed by its solve kernel, which zeroes them (a one-scan front-end saves a fill launch per call)
    if (b->n_total == 1 && max_iteration > 0) b->last_iterations = b->h_state[0].iterations;
    return LOCGPU_OK;
}

int align_finish(locgpu_ctx* ctx, locgpu_batch* b, double* out_poses, locgpu_align_stats* stats) {
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    if (!b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "align: no alignment of this batch has been begun");
    b->pending.active = false;
    const int rc = finish_on_stream(ctx, b, out_poses, stats);
    lease_release(ctx, b);  // on every way out
    return rc;
}

int run_align(locgpu_ctx* ctx, locgpu_batch* b, const double* init_poses, const AlignSpec& spec, double* out_poses, locgpu_align_stats* stats) {
    const int rc = align_begin(ctx, b, init_poses, spec, /*blocking*/ true);
    return rc != LOCGPU_OK ? rc : align_finish(ctx, b, out_poses, stats);
}

// The plane table of LOCGPU_P2PLANE_MAP for the current target (map_planes.hip), on the context's stream; no-op when it is there.
// Leaves go through the existing search stage in chunks of at most kPlaneChunk, as the points of a one-scan batch under the
// identity pose (k = 5, exact). The table and the chunk workspace are kept: nothing is allocated after the first call unless the map grew.
// The workspace is a whole one-scan batch (alloc_batch also makes partials, H/B and pinned state the ingest never touches: a few KB
// beside the 44 MB of points, lists and work lists at 2^20 leaves); like ctx->search it stays resident until locgpu_destroy, even
// if the table is never built again.
constexpr size_t kPlaneChunk = (size_t)1 << 20;
int ensure_map_planes(locgpu_ctx* ctx) {
    if (ctx->planes_ready) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    hipStream_t s = ctx->stream;
    const size_t rows = ctx->tree_slots / 2 + 2;  // slot >> 1 of every slot, the sentinel leaf behind the tree included
    if (rows * 4 > ctx->d_planes.cap() && !hip_ok(ctx, ctx->d_planes.alloc(with_headroom(rows) * 4), "hipMalloc map planes")) return LOCGPU_ERR_OOM;
    if (!hip_ok(ctx, ctx->d_planes_count.reserve(1), "hipMalloc map planes")) return LOCGPU_ERR_OOM;
    LOCGPU_HIP(ctx, hipMemsetAsync(ctx->d_planes, 0xFF, rows * 4 * sizeof(double), s));  // all-ones doubles are NaNs: no plane
    LOCGPU_HIP(ctx, hipMemsetAsync(ctx->d_planes_count, 0, sizeof(unsigned long long), s));
    unsigned long long n_valid = 0;
    if (ctx->num_leaves >= 5) {  // k > size_: GetClosestPoint returns nothing (kdtree.cpp:149-153) ⇒ no plane at all
        const size_t chunk = std::min(ctx->num_leaves, kPlaneChunk);
        locgpu_batch* w = ctx->planes_ws;
        if (!w || (size_t)w->max_n < chunk) {
            if (w) { free_batch(w); ctx->planes_ws = nullptr; }
            const int next_slot = ctx->next_slot;  // the workspace must not shift the streams the caller's batches are dealt
            const int rc = alloc_batch(ctx, 1, chunk, &ctx->planes_ws);
            ctx->next_slot = next_slot;
            if (rc != LOCGPU_OK) return rc;
            w = ctx->planes_ws;
            w->slot = 0;
            w->stream = s;
            w->pinned = true;
        }
        const double identity[7] = {0, 0, 0, 1, 0, 0, 0};
        init_states(w, identity);
        LOCGPU_HIP(ctx, hipMemsetAsync(w->d_redo_count, 0, 4 * sizeof(unsigned int), s));
        LOCGPU_HIP(ctx, hipMemcpyAsync(w->d_state, w->h_state, sizeof(PoseState), hipMemcpyHostToDevice, s));
        for (size_t first = 0; first < ctx->num_leaves; first += chunk) {
            const int cnt = (int)std::min(chunk, ctx->num_leaves - first);
            launch_map_plane_queries(ctx->d_tree, ctx->d_leaf_slots, first, cnt, w->d_src, w->d_counts, s);
            SearchArgs sa = make_search_args(ctx, w, w->d_src, w->d_state, 5, 1.0f, false);
            sa.search_stats = nullptr;  // the ingest's queries are not the matcher's
            if (!launch_icp_search(sa, s)) return fail(ctx, LOCGPU_ERR_DEPTH, "icp_build_map_planes: unsupported tree depth");
            LOCGPU_HIP(ctx, hipMemsetAsync(w->d_redo_count, 0, 4 * sizeof(unsigned int), s));  // the work lists are consumed
            launch_map_plane_fit(ctx->d_tree, ctx->d_leaf_slots, first, cnt, w->d_nn, w->pitch, ctx->d_planes, ctx->d_planes_count, s);
        }
        LOCGPU_HIP(ctx, hipGetLastError());
        LOCGPU_HIP(ctx, hipMemcpyAsync(&n_valid, ctx->d_planes_count, sizeof(n_valid), hipMemcpyDeviceToHost, s));
    }
    LOCGPU_HIP(ctx, hipStreamSynchronize(s));  // batches run on other streams: the table is complete before anyone reads it
    ctx->planes_rows = ctx->num_leaves;
    ctx->planes_valid = (long long)n_valid;
    ctx->planes_ready = true;
    return LOCGPU_OK;
}

// Score of every entry of `b` under its pose: k = 1 exact search stage, then the reduction of fitness.hip. pairs: per scan against
// its own tree of the forest (b->pair_base), a scan without a target (b->pair_skip) is `done` for the search and scores {+inf, 0, 0}.
static int fitness_on_batch_impl(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, double max_range, locgpu_fitness* out, bool pairs) {
    if (b->sharded) return fail(ctx, LOCGPU_ERR_INVALID, "icp_fitness: sharded batches are not scored");
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "icp_fitness: an alignment of this batch has been begun and not finished");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    { const int urc = batch_ready(ctx, b); if (urc != LOCGPU_OK) return urc; }
    init_states(b, poses);
    hipStream_t s = b->stream;
    if (pairs) {
        // The search skips a `done` scan; the score kernel does not look at the flag and would follow whatever the scan's list rows
        // hold: they are set to "no neighbour" (all-ones bytes = kInvalidSlot) first, which makes every point of the scan a non-query.
        for (int i = 0; i < b->n_scans; ++i)
            if (b->pair_skip[i]) {
                b->h_state[i].done = 1;
                LOCGPU_HIP(ctx, hipMemsetAsync(b->d_nn + (size_t)i * b->max_n, 0xFF, (size_t)b->max_n * sizeof(uint32_t), s));
            }
        const int prc = upload_pair_base(ctx, b);
        if (prc != LOCGPU_OK) return prc;
    }
    if (!b->counters_clean) LOCGPU_HIP(ctx, hipMemsetAsync(b->d_redo_count, 0, 4 * sizeof(unsigned int), s));
    b->counters_clean = false;
    LOCGPU_HIP(ctx, hipMemcpyAsync(b->d_state, b->h_state, b->n_total * sizeof(PoseState), hipMemcpyHostToDevice, s));
    // the exact walk whatever the matcher's options say: a score must not depend on a pruning knob (alpha_eff = 1), and it skips the
    // points pcl::isFinite rejects
    SearchArgs sa = make_search_args(ctx, b, batch_src(b), b->d_state, 1, 1.0f, true);
    sa.src_of = b->d_src_of;
    if (pairs) sa.scan_tree_base = b->d_pair_base;
    if (!launch_icp_search(sa, s)) return fail(ctx, LOCGPU_ERR_DEPTH, "icp_fitness: unsupported tree depth");
    FitnessArgs fa{ctx->d_tree, batch_src(b), b->d_counts, b->d_state, b->d_nn, b->max_n, b->n_scans, (float)(max_range * max_range), b->d_partials, b->d_hb, b->d_redo_count};
    fa.src_of = b->d_src_of;
    launch_icp_fitness(fa, s);
    LOCGPU_HIP(ctx, hipGetLastError());
    LOCGPU_HIP(ctx, hipMemcpyAsync(b->h_hb, b->d_hb, (size_t)b->n_scans * kFitW * sizeof(double), hipMemcpyDeviceToHost, s));
    LOCGPU_HIP(ctx, hipStreamSynchronize(s));
    b->counters_clean = true;  // the sum kernel zeroed them behind the search
    for (int i = 0; i < b->n_scans; ++i) {
        const double* r = b->h_hb + (size_t)i * kFitW;
        out[i].inliers = (int64_t)r[1];
        out[i].finite_points = (int64_t)r[2];
        out[i].score = out[i].inliers > 0 ? r[0] / (double)out[i].inliers : HUGE_VAL;
        if (pairs && b->pair_skip[i]) out[i] = locgpu_fitness{HUGE_VAL, 0, 0};  // never searched: its list rows are stale
    }
    return LOCGPU_OK;
}

int fitness_on_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, double max_range, locgpu_fitness* out) {
    return fitness_on_batch_impl(ctx, b, poses, max_range, out, false);
}
int fitness_pairs_on_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, double max_range, locgpu_fitness* out) {
    return fitness_on_batch_impl(ctx, b, poses, max_range, out, true);
}

// Score of every entry of `b` under its pose against the direct NDT table: the probe-and-reduce kernel of ndt_fitness.hip, then the
// ICP score's fixed-order sum. Touches nothing of the search stage (no neighbour lists, no work-list counters). pairs: per scan under
// its own target of the voxel set (b->pair_base); a scan without a target (b->pair_skip) is scored against target 0 and reported as
// {+inf, 0, 0}.
static int ndt_fitness_on_batch_impl(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, locgpu_fitness* out, bool pairs) {
    if (b->sharded) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_fitness: sharded batches are not scored");
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "ndt_fitness: an alignment of this batch has been begun and not finished");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    { const int urc = batch_ready(ctx, b); if (urc != LOCGPU_OK) return urc; }
    init_states(b, poses);
    hipStream_t s = b->stream;
    LOCGPU_HIP(ctx, hipMemcpyAsync(b->d_state, b->h_state, b->n_total * sizeof(PoseState), hipMemcpyHostToDevice, s));
    if (pairs) {
        const int prc = upload_pair_base(ctx, b);
        if (prc != LOCGPU_OK) return prc;
    }
    launch_ndt_fitness(ctx->ndt, batch_src(b), b->d_counts, b->d_state, b->max_n, b->n_scans, b->d_partials, b->d_hb, s, b->d_src_of, pairs ? b->d_pair_base.get() : nullptr);
    LOCGPU_HIP(ctx, hipGetLastError());
    LOCGPU_HIP(ctx, hipMemcpyAsync(b->h_hb, b->d_hb, (size_t)b->n_scans * kFitW * sizeof(double), hipMemcpyDeviceToHost, s));
    LOCGPU_HIP(ctx, hipStreamSynchronize(s));
    for (int i = 0; i < b->n_scans; ++i) {
        const double* r = b->h_hb + (size_t)i * kFitW;
        out[i].inliers = (int64_t)r[1];
        out[i].finite_points = (int64_t)r[2];
        out[i].score = out[i].inliers > 0 ? r[0] / (double)out[i].inliers : HUGE_VAL;
        if (pairs && b->pair_skip[i]) out[i] = locgpu_fitness{HUGE_VAL, 0, 0};
    }
    return LOCGPU_OK;
}

int ndt_fitness_on_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, locgpu_fitness* out) { return ndt_fitness_on_batch_impl(ctx, b, poses, out, false); }
int ndt_fitness_pairs_on_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, locgpu_fitness* out) { return ndt_fitness_on_batch_impl(ctx, b, poses, out, true); }

int eval_hb_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, const AlignSpec& spec, double* hb, const char* who) {
    const bool ndt = spec.ndt();
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": an alignment of this batch has been begun and not finished");
    if (!ndt) { const int grc = ensure_grid_lists(ctx, b, spec); if (grc != LOCGPU_OK) return grc; }
    { const int urc = batch_ready(ctx, b); if (urc != LOCGPU_OK) return urc; }
    init_states(b, poses);
    // NDT has no search stage: its evaluation leaves the work-list counters, and what the batch knows about them, as they are
    if (!ndt) {
        b->counters_clean = false;
        LOCGPU_HIP(ctx, hipMemsetAsync(b->d_redo_count, 0, 4 * sizeof(unsigned int), b->stream));
    }
    LOCGPU_HIP(ctx, hipMemcpyAsync(b->d_state, b->h_state, b->n_total * sizeof(PoseState), hipMemcpyHostToDevice, b->stream));
    b->stage_ev.used = 0;
    IterLauncher it{ctx, b, spec};
    if (!it.launch(0)) return LOCGPU_ERR_NO_DEVICE;
    LOCGPU_HIP(ctx, hipMemcpyAsync(b->h_hb, b->d_hb, (size_t)b->n_total * 44 * sizeof(double), hipMemcpyDeviceToHost, b->stream));
    LOCGPU_HIP(ctx, hipStreamSynchronize(b->stream));
    b->stage_ev.collect(ctx, ndt);
    std::memcpy(hb, b->h_hb, (size_t)b->n_total * 44 * sizeof(double));
    return LOCGPU_OK;
}

}  // namespace locgpu
