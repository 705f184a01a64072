// loc_lib_amd/csrc/resident_deskew.hip — a resident batch motion-compensated where it lies (include/locgpu.h, "Deskew of a resident
// batch").
//
// The deskewed ingest forms (range_ingest.hip, record_ingest.hip) need the sweep motion BEFORE the scan is uploaded, and the caller
// has it only after the alignment of that same scan: the reference forms it from the last two results, predict_pos = result_pos *
// last_pose.inverse() * result_pos (loc.cpp:232, lio.cpp:465). So the standard two-pass — align the skewed scan, derive the motion,
// deskew, re-align or merge — sent the raw bytes over PCIe twice. With locgpu_batch_keep_times on, the plain ingest calls leave the one
// thing the raw survivors lack, 8 B per point: the time key (rec_scatter_kernel<false, true>, ri_scatter_times_kernel). This file is
// the pass that uses it, and the host helper that makes a locgpu_sweep_motion of a pose sequence.
//
//   check    block (tile of 1024 points, scan): 8 B per point in; tp = key (+ time_offsets[s]); survivors whose tp is     rsd_check_kernel
//            not finite, lies before the scan's first knot or more than 0.5 s behind its last → the tile's count
//   offsets  ri_offsets_kernel: the scan's sum of its tile counts (ingest_launch_offsets, one row)
//   verdict  ri_verdict_kernel with room for 0: 1 when no scan has a bad survivor (ingest_launch_verdict)
//   move     block (tile, scan): the scan's knots staged in LDS, the reference pose once per block by thread 0 (the same       rsd_move_kernel
//            inputs through the same function in every block: the same bits), then per point 16 B + 8 B in, rd_move_point —
//            the device function of rec_scatter_kernel<true> — 16 B out; dst != src: + the ring byte and the count
//
// A point keeps its place: no compaction, no atomics, so the bits depend neither on n_scans nor on a scan's place. Nothing is
// written when the verdict is 0 — the mechanism of the ingest's refusals — so dst is exactly as it was, also in place.
//
// Scratch, grow-only on the context (resident_deskew_free): 8 B per knot value and scan (+ pinned), 8 B per tile, 4 B per scan
// (+ pinned).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "cloud_filters.hpp"
#include "context.hpp"
#include "pose_interp.hpp"
#include "range_ingest.hpp"

namespace locgpu {

namespace {

constexpr int kRsdPer = 4;                 // points per lane
constexpr int kRsdTile = kRI * kRsdPer;    // points per block: the knots and the reference pose are staged once per 1024 points

// motion = times [n_scans][K] | poses [n_scans][K][7] | ref_times [n_scans] | time_offsets [n_scans] (the last row only with add_offset)
__device__ __forceinline__ double rsd_time(const double* __restrict__ times, size_t at, const double* __restrict__ motion, int n_scans, int K, uint32_t s, int add_offset) {
    const double key = times[at];
    if (!add_offset) return key;  // time_offsets == NULL: nothing is added
    double tp;
    {
#pragma clang fp contract(off)
        tp = key + motion[(size_t)n_scans * (8 * K + 1) + s];  // the second IEEE operation of the header's "Point time" rule
    }
    return tp;
}

// The points scan s holds, never more than either batch has rows for (the host has checked the counts it knows).
__device__ __forceinline__ uint32_t rsd_count(const int* __restrict__ counts, uint32_t s, uint32_t max_n) {
    const int n = counts[s];
    return n < 0 ? 0u : min((uint32_t)n, max_n);
}

// tile_cnt [n_scans][n_tiles]: the tile's survivors with a refused time.
__global__ __launch_bounds__(kRI) void rsd_check_kernel(const double* __restrict__ times, const int* __restrict__ counts, uint32_t max_n, uint32_t n_tiles,
                                                        const double* __restrict__ motion, int n_scans, int K, int add_offset, uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t s_wave[kRI / 64];
    const uint32_t s = blockIdx.y, tile = blockIdx.x;
    const uint32_t n = rsd_count(counts, s, max_n);
    const double* t = motion + (size_t)s * K;
    const double t_first = t[0], t_last = t[K - 1];
    uint32_t bad = 0;
#pragma unroll
    for (int k = 0; k < kRsdPer; ++k) {
        const uint32_t i = tile * kRsdTile + k * kRI + threadIdx.x;
        if (i < n) {  // i < max_n: inside scan s's rows of the times
            const double tp = rsd_time(times, (size_t)s * max_n + i, motion, n_scans, K, s, add_offset);
            if (!isfinite(tp) || tp < t_first || tp - t_last > kInterpTimeTh) ++bad;
        }
    }
    uint32_t total;
    (void)block_exclusive(bad, s_wave, total);
    if (threadIdx.x == 0) tile_cnt[(size_t)s * n_tiles + tile] = total;
}

// Tile (blockIdx.x, scan blockIdx.y): point i of src's scan → point i of dst's scan, moved by the matrix of its own time. dst may be
// src (every lane reads its point before it writes it, and no other lane touches it). dst_ring / dst_counts: NULL in place.
__global__ __launch_bounds__(kRI) void rsd_move_kernel(const float4* src, const double* __restrict__ times, const unsigned char* src_ring, const int* __restrict__ counts,
                                                       uint32_t max_n, const int32_t* __restrict__ res, const double* __restrict__ motion, int n_scans, int K, int add_offset,
                                                       float4* dst, unsigned char* dst_ring, int* __restrict__ dst_counts, uint32_t dst_max_n) {
    if (res[n_scans] == 0) return;  // the same for every thread of the grid
    __shared__ double s_t[kMaxKnots];
    __shared__ double s_p[kMaxKnots * 7];
    __shared__ double s_ref[12];  // R_r, t_r
    const uint32_t s = blockIdx.y, tile = blockIdx.x;
    const uint32_t n = rsd_count(counts, s, min(max_n, dst_max_n));
    if (tile == 0 && threadIdx.x == 0 && dst_counts) dst_counts[s] = (int)n;
    if (tile * kRsdTile >= n) return;  // the same for every thread of the block
    const double* g_t = motion + (size_t)s * K;
    const double* g_p = motion + (size_t)n_scans * K + (size_t)s * K * 7;
    for (int i = threadIdx.x; i < K; i += kRI) s_t[i] = g_t[i];
    for (int i = threadIdx.x; i < 7 * K; i += kRI) s_p[i] = g_p[i];
    __syncthreads();
    if (threadIdx.x == 0) rd_ref_pose(s_t, s_p, K, motion[(size_t)n_scans * K * 8 + s], s_ref);
    __syncthreads();
#pragma unroll 1
    for (int k = 0; k < kRsdPer; ++k) {
        const uint32_t i = tile * kRsdTile + k * kRI + threadIdx.x;
        if (i >= n) break;  // i < n <= max_n and dst_max_n: inside scan s's rows of both batches
        const size_t from = (size_t)s * max_n + i, to = (size_t)s * dst_max_n + i;
        const double tp = rsd_time(times, from, motion, n_scans, K, s, add_offset);
        double m[12];
        dst[to] = rd_move_point(s_t, s_p, K, s_ref, tp, src[from], m);
        if (dst_ring) dst_ring[to] = src_ring[from];
    }
}

int hip_fail(locgpu_ctx* ctx, hipError_t e, const char* what) {
    hip_ok(ctx, e, what);
    return e == hipErrorOutOfMemory ? LOCGPU_ERR_OOM : LOCGPU_ERR_NO_DEVICE;
}

}  // namespace

struct ResidentDeskewScratch {
    PinnedBuf<double> h_motion;  // times [n_scans][K] | poses [n_scans][K][7] | ref_times [n_scans] | time_offsets [n_scans]
    DevBuf<double> d_motion;
    DevBuf<uint32_t> tile_cnt, tile_off;  // [n_scans][n_tiles]
    DevBuf<int32_t> res;                  // bad survivors [n_scans] | verdict | the largest of them
    PinnedBuf<int32_t> h_res;
    PinnedBuf<double> h_times;            // locgpu_batch_download_times
    // locgpu_profile_enable: [0,1] round the check kernel, [2,3] round the move kernel, on the compute stream
    Event prof[4];
    bool prof_valid = false;
    double prof_ms[2] = {0, 0};
};

namespace {

ResidentDeskewScratch* scratch(locgpu_ctx* ctx) {
    if (!ctx->rdeskew) ctx->rdeskew = new ResidentDeskewScratch();
    return ctx->rdeskew;
}

template <typename B>
hipError_t grow(B& buf, size_t n) {
    return n <= buf.cap() ? hipSuccess : buf.alloc(with_headroom(n));
}

// The pass on ctx->stream; the bad-survivor counts and the verdict are on their way to S->h_res when it returns.
hipError_t deskew_dev(locgpu_ctx* ctx, locgpu_batch* src, locgpu_batch* dst, const double* time_offsets, const locgpu_sweep_motion& m) {
    ResidentDeskewScratch* S = scratch(ctx);
    const int n_scans = src->n_scans, K = m.n_knots;
    int longest = 0;
    for (int s = 0; s < n_scans; ++s) longest = std::max(longest, src->counts[s]);
    const uint32_t n_tiles = (uint32_t)std::max(1, (longest + kRsdTile - 1) / kRsdTile);
    const size_t tiles = (size_t)n_scans * n_tiles, nk = (size_t)n_scans * K, n_motion = 8 * nk + 2 * (size_t)n_scans, n_res = (size_t)n_scans + 2;
    LOCGPU_TRY(grow(S->h_motion, n_motion));
    LOCGPU_TRY(grow(S->d_motion, n_motion));
    LOCGPU_TRY(grow(S->tile_cnt, tiles));
    LOCGPU_TRY(grow(S->tile_off, tiles));
    LOCGPU_TRY(grow(S->res, n_res));
    LOCGPU_TRY(grow(S->h_res, n_res));
    const bool prof = ctx->profile != 0;
    S->prof_valid = false;
    if (prof)
        for (Event& e : S->prof) LOCGPU_TRY(e.ensure(hipEventDefault));
    std::memcpy(S->h_motion, m.knot_times, nk * sizeof(double));
    std::memcpy(S->h_motion + nk, m.knot_poses, 7 * nk * sizeof(double));
    std::memcpy(S->h_motion + 8 * nk, m.ref_times, (size_t)n_scans * sizeof(double));
    if (time_offsets) std::memcpy(S->h_motion + 8 * nk + n_scans, time_offsets, (size_t)n_scans * sizeof(double));
    else std::fill(S->h_motion + 8 * nk + n_scans, S->h_motion + n_motion, 0.0);
    hipStream_t s = ctx->stream;
    // the call is blocking: the staging is free again when it returns
    LOCGPU_TRY(hipMemcpyAsync(S->d_motion, S->h_motion, n_motion * sizeof(double), hipMemcpyHostToDevice, s));
    const bool in_place = src == dst;
    const int add_offset = time_offsets ? 1 : 0;
    const dim3 grid(n_tiles, n_scans);
    if (prof) LOCGPU_TRY(hipEventRecord(S->prof[0], s));
    hipLaunchKernelGGL(rsd_check_kernel, grid, dim3(kRI), 0, s, src->d_times.get(), src->d_counts.get(), (uint32_t)src->max_n, n_tiles, S->d_motion.get(), n_scans, K, add_offset,
                       S->tile_cnt.get());
    LOCGPU_TRY(hipGetLastError());
    if (prof) LOCGPU_TRY(hipEventRecord(S->prof[1], s));
    ingest_launch_offsets(s, S->tile_cnt.get(), n_tiles, S->tile_off.get(), S->res.get(), n_scans, 1);
    ingest_launch_verdict(s, S->res.get(), n_scans, 0u, 1);  // room for 0 bad survivors
    LOCGPU_TRY(hipGetLastError());
    if (prof) LOCGPU_TRY(hipEventRecord(S->prof[2], s));
    const unsigned char* src_ring = src->rings_valid ? src->d_rings.get() : nullptr;
    hipLaunchKernelGGL(rsd_move_kernel, grid, dim3(kRI), 0, s, src->d_src.get(), src->d_times.get(), src_ring, src->d_counts.get(), (uint32_t)src->max_n, S->res.get(),
                       S->d_motion.get(), n_scans, K, add_offset, dst->d_src.get(), in_place || !src_ring ? (unsigned char*)nullptr : dst->d_rings.get(),
                       in_place ? (int*)nullptr : dst->d_counts.get(), (uint32_t)dst->max_n);
    LOCGPU_TRY(hipGetLastError());
    if (prof) {
        LOCGPU_TRY(hipEventRecord(S->prof[3], s));
        S->prof_valid = true;
    }
    return hipMemcpyAsync(S->h_res, S->res, n_res * sizeof(int32_t), hipMemcpyDeviceToHost, s);
}

// The stream has been waited for: the elapsed times of the pass that just ran.
void collect_times(locgpu_ctx* ctx) {
    ResidentDeskewScratch* S = ctx->rdeskew;
    if (!S->prof_valid) return;
    float check_ms = 0.f, move_ms = 0.f;
    if (hipEventElapsedTime(&check_ms, S->prof[0], S->prof[1]) == hipSuccess && hipEventElapsedTime(&move_ms, S->prof[2], S->prof[3]) == hipSuccess) {
        S->prof_ms[0] = check_ms;
        S->prof_ms[1] = move_ms;
    }
}

// ---- locgpu_motion_from_poses: SE(3) on the host, FP64, one IEEE operation per written operation, nothing normalised ----------------
struct Pose {
    double q[4], t[3];  // quaternion xyzw, translation
};

// q1 ⊗ q2, Eigen's product order
void quat_mul(const double* a, const double* b, double* o) {
    o[3] = ((a[3] * b[3] - a[0] * b[0]) - a[1] * b[1]) - a[2] * b[2];
    o[0] = ((a[3] * b[0] + a[0] * b[3]) + a[1] * b[2]) - a[2] * b[1];
    o[1] = ((a[3] * b[1] + a[1] * b[3]) + a[2] * b[0]) - a[0] * b[2];
    o[2] = ((a[3] * b[2] + a[2] * b[3]) + a[0] * b[1]) - a[1] * b[0];
}

// R(q) · v, every dot product summed left to right
void rotate(const double* q, const double* v, double* o) {
    double R[9];
    quat_to_R(q, R);
    for (int r = 0; r < 3; ++r) o[r] = (R[3 * r] * v[0] + R[3 * r + 1] * v[1]) + R[3 * r + 2] * v[2];
}

// (q, t)⁻¹ = (conj q, −R(conj q) · t)
Pose inverse(const Pose& a) {
    Pose o;
    o.q[0] = -a.q[0], o.q[1] = -a.q[1], o.q[2] = -a.q[2], o.q[3] = a.q[3];
    double rt[3];
    rotate(o.q, a.t, rt);
    for (int r = 0; r < 3; ++r) o.t[r] = -rt[r];
    return o;
}

// (q₁, t₁) · (q₂, t₂) = (q₁ ⊗ q₂, t₁ + R(q₁) · t₂)
Pose compose(const Pose& a, const Pose& b) {
    Pose o;
    quat_mul(a.q, b.q, o.q);
    double rt[3];
    rotate(a.q, b.t, rt);
    for (int r = 0; r < 3; ++r) o.t[r] = a.t[r] + rt[r];
    return o;
}

// (T_a · T_b⁻¹) · T_a: one more step of the motion that led from b to a (loc.cpp:232)
Pose extrapolate(const Pose& a, const Pose& b) { return compose(compose(a, inverse(b)), a); }

}  // namespace

void resident_deskew_free(locgpu_ctx* ctx) {
    delete ctx->rdeskew;
    ctx->rdeskew = nullptr;
}

}  // namespace locgpu

using namespace locgpu;

extern "C" {

int locgpu_batch_keep_times(locgpu_batch* b, int on) {
    if (!b) return fail(nullptr, LOCGPU_ERR_INVALID, "batch_keep_times: NULL batch");
    locgpu_ctx* ctx = b->ctx;
    if (b->shared_src || b->sharded) return fail(ctx, LOCGPU_ERR_INVALID, "batch_keep_times: sharded and shared-source batches are not supported");
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "batch_keep_times: an alignment of this batch has been begun and not finished");
    b->keep_times = on != 0;
    if (!b->keep_times && b->d_times) {  // off: nothing is kept
        b->times_valid = false;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);  // every call that reads or writes the times is blocking on this stream
        b->d_times.reset();
    }
    return LOCGPU_OK;
}

int locgpu_batch_download_times(locgpu_batch* b, int scan, double* out, size_t capacity, size_t* n) {
    if (!b) return fail(nullptr, LOCGPU_ERR_INVALID, "batch_download_times: NULL batch");
    locgpu_ctx* ctx = b->ctx;
    if (!b->times_valid) return fail(ctx, LOCGPU_ERR_INVALID, "batch_download_times: the batch holds no resident times (locgpu_batch_keep_times, then a plain ingest of scans that carry times)");
    if (scan < 0 || scan >= b->n_scans) return fail(ctx, LOCGPU_ERR_INVALID, "batch_download_times: scan index out of range");
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "batch_download_times: an alignment of this batch has been begun and not finished");
    const size_t cnt = (size_t)b->counts[scan];
    if (n) *n = cnt;
    if (!out) return LOCGPU_OK;
    if (cnt > capacity) return fail(ctx, LOCGPU_ERR_INVALID, "batch_download_times: capacity < the scan's size");
    if (cnt == 0) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    ResidentDeskewScratch* S = scratch(ctx);
    hipError_t e = S->h_times.reserve(cnt);
    if (e == hipSuccess) e = hipMemcpyAsync(S->h_times, b->d_times + (size_t)scan * b->max_n, cnt * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "batch_download_times: D2H");
    std::memcpy(out, S->h_times, cnt * sizeof(double));
    return LOCGPU_OK;
}

int locgpu_batch_deskew(locgpu_batch* src, locgpu_batch* dst, const double* time_offsets, const locgpu_sweep_motion* motion, int32_t* out_status) {
    const std::string who = "batch_deskew";
    if (!src || !dst) return fail(src ? src->ctx : (dst ? dst->ctx : nullptr), LOCGPU_ERR_INVALID, who + ": NULL batch");
    locgpu_ctx* ctx = src->ctx;
    if (dst->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, who + ": the batches belong to different contexts");
    if (src->sharded || dst->sharded) return fail(ctx, LOCGPU_ERR_INVALID, who + ": sharded batches are not supported");
    if (src->shared_src || dst->shared_src) return fail(ctx, LOCGPU_ERR_INVALID, who + ": shared-source batches are not supported");
    if (src->pending.active || dst->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, who + ": an alignment of the batch has been begun and not finished");
    if (!src->times_valid)
        return fail(ctx, LOCGPU_ERR_INVALID, who + ": src holds no resident times (they are left by a plain ingest after locgpu_batch_keep_times, and dropped by every later "
                                                   "upload, preprocess or deskew into the batch: compensated points are not compensated again)");
    const int n_scans = src->n_scans;
    if (dst->n_scans != n_scans) return fail(ctx, LOCGPU_ERR_INVALID, who + ": src and dst hold different numbers of scans");
    int rc = check_sweep_motion(ctx, who, motion, n_scans, false, 0.0, 0.0);
    if (rc != LOCGPU_OK) return rc;
    if (time_offsets)
        for (int i = 0; i < n_scans; ++i)
            if (!std::isfinite(time_offsets[i])) return fail(ctx, LOCGPU_ERR_INVALID, who + ": time_offsets[" + std::to_string(i) + "] is not finite");
    for (int i = 0; i < n_scans; ++i)
        if (src->counts[i] > dst->max_n)
            return fail(ctx, LOCGPU_ERR_INVALID, who + ": scan " + std::to_string(i) + " has " + std::to_string(src->counts[i]) + " points, dst was created for " +
                                                     std::to_string(dst->max_n) + " per scan (dst is unchanged)");
    if (out_status) std::fill(out_status, out_status + n_scans, 0);
    if (n_scans == 0) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    rc = order_behind_batch(ctx, src, (who + ": ordering behind src").c_str());
    if (rc == LOCGPU_OK && dst != src) rc = order_behind_batch(ctx, dst, (who + ": ordering behind dst").c_str());
    if (rc != LOCGPU_OK) return rc;
    hipError_t e = dst == src || !src->rings_valid || dst->d_rings ? hipSuccess : dst->d_rings.alloc(std::max<size_t>(dst->pitch, 1));
    if (e != hipSuccess) return hip_fail(ctx, e, (who + ": ring bytes").c_str());
    e = deskew_dev(ctx, src, dst, time_offsets, *motion);
    // the one read-back: when it is there the whole pass has run, and whatever uses dst next — on any stream — finds it complete
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->stream);
        return hip_fail(ctx, e, who.c_str());
    }
    src->paced_tail = dst->paced_tail = false;
    collect_times(ctx);
    const int32_t* res = ctx->rdeskew->h_res;
    if (!res[n_scans]) {
        int first = 0;
        while (first < n_scans && res[first] == 0) ++first;
        if (out_status)
            for (int i = 0; i < n_scans; ++i) out_status[i] = res[i] != 0;
        return fail(ctx, LOCGPU_ERR_INVALID, who + ": scan " + std::to_string(first) + " has " + std::to_string(first < n_scans ? res[first] : 0) +
                                                 " survivors whose time is not finite, lies before the first knot or more than 0.5 s behind the last knot (dst is unchanged)");
    }
    if (dst != src) {
        set_host_counts(dst, src->counts.data());
        dst->rings_valid = src->rings_valid;
    }
    dst->times_valid = false;  // compensated points are no longer raw; src (when it is another batch) keeps its points and times
    return LOCGPU_OK;
}

int locgpu_batch_deskew_times(locgpu_ctx* ctx, double out_ms[2]) {
    if (!ctx || !out_ms) return fail(ctx, LOCGPU_ERR_INVALID, "batch_deskew_times: NULL argument");
    out_ms[0] = ctx->rdeskew ? ctx->rdeskew->prof_ms[0] : 0.0;
    out_ms[1] = ctx->rdeskew ? ctx->rdeskew->prof_ms[1] : 0.0;
    return LOCGPU_OK;
}

int locgpu_motion_from_poses(const double* poses, const double* stamps, int n, double* knot_times, double* knot_poses) {
    if (!poses || !stamps || !knot_times || !knot_poses) return fail(nullptr, LOCGPU_ERR_INVALID, "motion_from_poses: NULL array");
    if (n < 2) return fail(nullptr, LOCGPU_ERR_INVALID, "motion_from_poses: at least two poses are needed (n < 2)");
    for (int i = 0; i < n; ++i)
        if (!std::isfinite(stamps[i]) || (i && !(stamps[i] > stamps[i - 1])))
            return fail(nullptr, LOCGPU_ERR_INVALID, "motion_from_poses: stamps must be finite and strictly increasing (stamps[" + std::to_string(i) + "])");
    auto pose = [&](int i) {
        Pose p;
        std::memcpy(p.q, poses + 7 * (size_t)i, 4 * sizeof(double));
        std::memcpy(p.t, poses + 7 * (size_t)i + 4, 3 * sizeof(double));
        return p;
    };
    const Pose before = extrapolate(pose(0), pose(1)), after = extrapolate(pose(n - 1), pose(n - 2));
    const double t_before = 2.0 * stamps[0] - stamps[1], t_after = 2.0 * stamps[n - 1] - stamps[n - 2];
    for (int i = 0; i < n; ++i) {
        for (int k = 0; k < 3; ++k) {
            const int j = i - 1 + k;
            const Pose p = j < 0 ? before : j >= n ? after : pose(j);
            knot_times[3 * (size_t)i + k] = j < 0 ? t_before : j >= n ? t_after : stamps[j];
            double* o = knot_poses + 7 * (3 * (size_t)i + k);
            std::memcpy(o, p.q, 4 * sizeof(double));
            std::memcpy(o + 4, p.t, 3 * sizeof(double));
        }
    }
    return LOCGPU_OK;
}

}  // extern "C"
