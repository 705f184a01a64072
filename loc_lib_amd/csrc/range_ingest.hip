// loc_lib_amd/csrc/range_ingest.hip — range images decoded in HBM (include/locgpu.h, "Range-image ingest"; range_ingest.hpp).
//
// The reference's step from the driver's cloud to the library's cloud is CloudConver::Conver (LocUtils/src/subscriber/
// cloud_subscriber.cpp:7-29): drop non-finite points, drop points with PointDistance(p) < 4.0 (common/point_cloud_utils.h:41-44), keep
// the survivors in input order. A spinning LiDAR delivers that cloud as a range image — n_rings × n_cols 16-bit counts, 2 B per cell,
// ring and azimuth implicit in the position — and the raw float4 points are what bounds the batch pipelines (472 MB over PCIe for
// 256 × 115 200 points; the images are 59 MB). This file takes the images on the host, decodes them on the device, applies Conver's
// two rules there and leaves an ordinary batch (or a resident cloud) plus one ring byte per survivor.
//
// One pass for all scans of a call, images staged [n_scans][cells_pad] (cells_pad = cells rounded up to 8, so that every scan starts
// on a 16-byte boundary and every lane's eight cells are ONE 16-byte load that stays inside the allocation; cells ≥ n_rings · n_cols
// are treated as "no return", whatever the padding holds):
//
//   count    block (tile, scan): 256 lanes × 8 cells, decode + the two rules → survivors of the tile                ri_count_kernel
//   offsets  one workgroup per scan: exclusive sum of its tile counts in tile order, the scan's total               ri_offsets_kernel
//   verdict  one workgroup: does every scan fit the destination; the largest count                                  ri_verdict_kernel
//   scatter  block (tile, scan): decode again, compact the tile in LDS in cell order, then coalesced float4 stores   ri_scatter_kernel
//            and one ring-byte store per survivor at scan base + tile offset; the device counts
//
// A survivor's position is the number of survivors before it in cell order (ring-ascending, then column-ascending): integer sums in
// a fixed order, no atomics anywhere, so counts, order and bits do not depend on n_scans, on the scan's position or on the run.
// Nothing is written when the verdict is 0: the call fails and the destination is exactly as it was. The second decode re-reads
// 2 B per cell (L2-resident at scan size) to save 17 B per cell of staging between the two kernels.
//
// Scratch, grow-only on the context (freed by range_ingest_free): 2 B per cell pinned + 2 B per cell in HBM, 8 B per tile, 4 B per
// scan (+ pinned), and for the cloud form 1 B per cell of ring bytes (+ pinned).
//
// Motion compensation at decode (include/locgpu.h, "Range-image ingest, motion-compensated"): the *_deskew entry points
// run the same pass with one kernel ahead of it and another scatter —
//
//   matrices one block per scan: the knots staged in LDS, math::PoseInterp (math_utils.h:470-517) at the reference         rd_pose_kernel
//            time once and at every column's time, M = [R_rᵀ·R_c | R_rᵀ·(t_c − t_r)] → 12 doubles per column
//   scatter  ri_scatter_kernel with the survivor's column carried through the compaction; the final store loop applies     rd_scatter_kernel
//            the column's matrix (transform_point_f64), so only survivors are transformed
//
// — so survivors, order, counts and ring bytes are the plain call's. Scratch: 96 B per column and scan for the matrices, 8 B per knot
// value (+ pinned). The plain entry points launch the four kernels above and nothing else — with locgpu_batch_keep_times on and a
// sensor that has column times, ri_scatter_times_kernel in ri_scatter_kernel's place: the same bytes, and col_time[column] of every
// survivor beside its ring byte, for locgpu_batch_deskew (resident_deskew.hip).
//
// Shared with the point-record ingest (record_ingest.hip): Conver's keep rule and block_exclusive (range_ingest.hpp), rd_pose_at and the
// matrix product (pose_interp.hpp), the offsets and verdict kernels (ingest_launch_*; a second row of sums that this file leaves
// off) and the motion's host-side refusals (check_sweep_motion).
#include "range_ingest.hpp"

#include <algorithm>
#include <atomic>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "batch_upload.hpp"
#include "cloud_filters.hpp"
#include "context.hpp"
#include "pose_interp.hpp"

namespace locgpu {

namespace {

constexpr int kCellsPerLane = 8;               // one 16-byte load
constexpr int kTile = kRI * kCellsPerLane;     // cells per block
constexpr int kMaxRings = 256, kMaxCols = 12288;  // the LOAM picker's limits: a ring byte, rings of at most 6 × 2048 points

struct SensorView {
    const float* __restrict__ cos_el;
    const float* __restrict__ sin_el;
    const float* __restrict__ cos_az;
    const float* __restrict__ sin_az;
    uint32_t n_cols, cells, cells_pad, az_per_ring;
    float range_scale, min_range;
};

// The eight cells base .. base + 7 of scan s: bit j of the result = cell base + j yields a point, pts[j] / ring[j] are then valid.
// base is a multiple of 8 below cells_pad.
__device__ __forceinline__ uint32_t decode8(const SensorView& v, const uint16_t* __restrict__ img, uint32_t s, uint32_t base, float4 (&pts)[kCellsPerLane],
                                            uint32_t (&ring)[kCellsPerLane]) {
    const uint4 w = *reinterpret_cast<const uint4*>(img + (size_t)s * v.cells_pad + base);
    const uint32_t word[4] = {w.x, w.y, w.z, w.w};
    uint32_t g = base / v.n_cols, c = base - g * v.n_cols;
    uint32_t mask = 0;
#pragma unroll
    for (int j = 0; j < kCellsPerLane; ++j) {
        const uint32_t k = (word[j >> 1] >> ((j & 1) * 16)) & 0xFFFFu;
        if (base + j < v.cells) {
            const uint32_t a = v.az_per_ring ? g * v.n_cols + c : c;
            if (range_decode_cell(k, v.range_scale, v.min_range, v.cos_el[g], v.sin_el[g], v.cos_az[a], v.sin_az[a], pts[j])) mask |= 1u << j;
            ring[j] = g;
        }
        if (++c == v.n_cols) { c = 0; ++g; }
    }
    return mask;
}

__global__ __launch_bounds__(kRI) void ri_count_kernel(SensorView v, const uint16_t* __restrict__ img, uint32_t n_tiles, uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t s_wave[kRI / 64];
    const uint32_t s = blockIdx.y, tile = blockIdx.x;
    const uint32_t base = tile * kTile + threadIdx.x * kCellsPerLane;
    uint32_t cnt = 0;
    if (base < v.cells) {
        float4 pts[kCellsPerLane];
        uint32_t ring[kCellsPerLane];
        cnt = __popc(decode8(v, img, s, base, pts, ring));
    }
    uint32_t total;
    (void)block_exclusive(cnt, s_wave, total);
    if (threadIdx.x == 0) tile_cnt[(size_t)s * n_tiles + tile] = total;
}

// Row blockIdx.y of scan blockIdx.x (range_ingest.hpp): row 0 — tile_off = exclusive sums of the scan's tile counts in tile order,
// res[s] = its survivors; row 1 (the record ingest's refused times) — res[n_scans + 2 + s] = the sum alone.
__global__ __launch_bounds__(kRI) void ri_offsets_kernel(const uint32_t* __restrict__ tile_cnt, uint32_t n_tiles, uint32_t* __restrict__ tile_off, int32_t* __restrict__ res,
                                                         int n_scans) {
    __shared__ uint32_t s_wave[kRI / 64];
    const uint32_t s = blockIdx.x, r = blockIdx.y;
    const size_t row = (size_t)s * n_tiles;
    const uint32_t* cnt = tile_cnt + (size_t)r * n_scans * n_tiles;
    uint32_t carry = 0;
    for (uint32_t t0 = 0; t0 < n_tiles; t0 += kRI) {  // n_tiles is the same for every thread: the barriers inside are uniform
        const uint32_t t = t0 + threadIdx.x;
        const uint32_t x = t < n_tiles ? cnt[row + t] : 0u;
        uint32_t total;
        const uint32_t ex = block_exclusive(x, s_wave, total);
        if (r == 0 && t < n_tiles) tile_off[row + t] = carry + ex;
        carry += total;
    }
    if (threadIdx.x == 0) res[r == 0 ? s : n_scans + 2 + s] = (int32_t)carry;
}

// res[n_scans] = 1 when every scan fits dst_max_n points (and, rows == 2, no scan has a positive row-1 sum), res[n_scans + 1] = the
// largest count.
__global__ __launch_bounds__(kRI) void ri_verdict_kernel(int32_t* __restrict__ res, int n_scans, uint32_t dst_max_n, int rows) {
    __shared__ int s_max[kRI / 64], s_bad[kRI / 64];
    int m = 0, bad = 0;
    for (int s = threadIdx.x; s < n_scans; s += kRI) {
        m = max(m, res[s]);
        if (rows == 2) bad = max(bad, res[n_scans + 2 + s]);
    }
    for (int off = 32; off > 0; off >>= 1) {
        m = max(m, __shfl_xor(m, off, 64));
        bad = max(bad, __shfl_xor(bad, off, 64));
    }
    if ((threadIdx.x & 63) == 0) s_max[threadIdx.x >> 6] = m, s_bad[threadIdx.x >> 6] = bad;
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int w = 1; w < kRI / 64; ++w) m = max(m, s_max[w]), bad = max(bad, s_bad[w]);
        res[n_scans] = (uint32_t)m <= dst_max_n && bad == 0 ? 1 : 0;
        res[n_scans + 1] = m;
    }
}

// Tile (blockIdx.x, scan blockIdx.y) → dst + s · dst_max_n + tile offset, {x, y, z, +0}, and the ring bytes beside it: the body of both
// scatter kernels. kDeskew: the survivor's column is carried through the compaction beside its ring byte and the final store loop
// applies the column's matrix (mats [n_scans][n_cols][12], rd_pose_kernel), so only survivors are transformed. kTimes (plain form only,
// a batch with locgpu_batch_keep_times on): the column is carried the same way and the store loop leaves col_time[column] in dst_time.
template <bool kDeskew, bool kTimes = false>
__device__ __forceinline__ void scatter_tile(const SensorView& v, const uint16_t* __restrict__ img, uint32_t n_tiles, const uint32_t* __restrict__ tile_off,
                                             const int32_t* __restrict__ res, int n_scans, uint32_t dst_max_n, const double* __restrict__ mats, float4* __restrict__ dst,
                                             unsigned char* __restrict__ dst_ring, int* __restrict__ dst_counts, const double* __restrict__ col_time = nullptr,
                                             double* __restrict__ dst_time = nullptr) {
    static_assert(!(kDeskew && kTimes), "deskewed points are no longer raw: they leave no times");
    if (res[n_scans] == 0) return;  // the same for every thread of the grid
    __shared__ float4 s_pts[kTile];
    __shared__ uint16_t s_col[kDeskew || kTimes ? kTile : 1];  // n_cols <= 12 288
    __shared__ unsigned char s_ring[kTile];
    __shared__ uint32_t s_wave[kRI / 64];
    const uint32_t s = blockIdx.y, tile = blockIdx.x;
    if (tile == 0 && threadIdx.x == 0 && dst_counts) dst_counts[s] = res[s];
    const uint32_t base = tile * kTile + threadIdx.x * kCellsPerLane;
    float4 pts[kCellsPerLane];
    uint32_t ring[kCellsPerLane];
    uint32_t mask = 0;
    if (base < v.cells) mask = decode8(v, img, s, base, pts, ring);
    uint32_t total;
    uint32_t at = block_exclusive(__popc(mask), s_wave, total);  // total <= kTile, at + popc(mask) <= total
#pragma unroll
    for (int j = 0; j < kCellsPerLane; ++j) {
        if (mask & (1u << j)) {
            s_pts[at] = pts[j];
            if constexpr (kDeskew || kTimes) s_col[at] = (uint16_t)(base + j - ring[j] * v.n_cols);  // cell = ring · n_cols + column
            s_ring[at] = (unsigned char)ring[j];
            ++at;
        }
    }
    __syncthreads();
    // tile_off + total <= res[s] <= dst_max_n (the verdict): every store below is inside scan s's rows
    const size_t out = (size_t)s * dst_max_n + tile_off[(size_t)s * n_tiles + tile];
    for (uint32_t i = threadIdx.x; i < total; i += kRI) {
        if constexpr (kDeskew)
            dst[out + i] = transform_point_f64(s_pts[i], mats + ((size_t)s * v.n_cols + s_col[i]) * 12, true);  // every survivor is finite
        else
            dst[out + i] = s_pts[i];
        dst_ring[out + i] = s_ring[i];
        if constexpr (kTimes) dst_time[out + i] = col_time[s_col[i]];  // s_col < n_cols, the table's length; [n_scans][dst_max_n], the layout of dst
    }
}

__global__ __launch_bounds__(kRI) void ri_scatter_kernel(SensorView v, const uint16_t* __restrict__ img, uint32_t n_tiles, const uint32_t* __restrict__ tile_off,
                                                         const int32_t* __restrict__ res, int n_scans, uint32_t dst_max_n, float4* __restrict__ dst,
                                                         unsigned char* __restrict__ dst_ring, int* __restrict__ dst_counts) {
    scatter_tile<false>(v, img, n_tiles, tile_off, res, n_scans, dst_max_n, nullptr, dst, dst_ring, dst_counts);
}

// ri_scatter_kernel that also leaves every survivor's time key — its column's firing time — in dst_time (locgpu_batch_keep_times).
__global__ __launch_bounds__(kRI) void ri_scatter_times_kernel(SensorView v, const uint16_t* __restrict__ img, uint32_t n_tiles, const uint32_t* __restrict__ tile_off,
                                                               const int32_t* __restrict__ res, int n_scans, uint32_t dst_max_n, const double* __restrict__ col_time,
                                                               float4* __restrict__ dst, unsigned char* __restrict__ dst_ring, int* __restrict__ dst_counts,
                                                               double* __restrict__ dst_time) {
    scatter_tile<false, true>(v, img, n_tiles, tile_off, res, n_scans, dst_max_n, nullptr, dst, dst_ring, dst_counts, col_time, dst_time);
}

// ---- Motion compensation at decode (include/locgpu.h, "Range-image ingest, motion-compensated") ------------------------------------
// Scan blockIdx.x: M[c] = [ R_rᵀ·R_c | R_rᵀ·(t_c − t_r) ] for each of its columns, row-major 3×4, every dot product summed left to
// right. motion = times [n_scans][K] | poses [n_scans][K][7] | ref_times [n_scans]. One block per scan, so that the knots are staged
// and the reference-time pose is computed once per scan; its threads walk the columns.
__global__ __launch_bounds__(kRI) void rd_pose_kernel(const double* __restrict__ motion, int n_scans, int K, const double* __restrict__ col_time, uint32_t n_cols,
                                                      double* __restrict__ mats) {
    __shared__ double s_t[kMaxKnots];
    __shared__ double s_p[kMaxKnots * 7];
    __shared__ double s_ref[12];  // R_r, t_r
    const uint32_t s = blockIdx.x;
    const double* g_t = motion + (size_t)s * K;
    const double* g_p = motion + (size_t)n_scans * K + (size_t)s * K * 7;
    for (int i = threadIdx.x; i < K; i += kRI) s_t[i] = g_t[i];
    for (int i = threadIdx.x; i < 7 * K; i += kRI) s_p[i] = g_p[i];
    __syncthreads();
    if (threadIdx.x == 0) rd_ref_pose(s_t, s_p, K, motion[(size_t)n_scans * K * 8 + s], s_ref);
    __syncthreads();
    for (uint32_t c = threadIdx.x; c < n_cols; c += kRI) {
        double pc[7];
        rd_pose_at(s_t, s_p, K, col_time[c], pc);
        rd_matrix(s_ref, pc, mats + ((size_t)s * n_cols + c) * 12);  // inside the table: ensure_deskew sized it for n_scans · n_cols matrices
    }
}

// ri_scatter_kernel with every survivor moved by its column's matrix; positions, counts and ring bytes are ri_scatter_kernel's.
__global__ __launch_bounds__(kRI) void rd_scatter_kernel(SensorView v, const uint16_t* __restrict__ img, uint32_t n_tiles, const uint32_t* __restrict__ tile_off,
                                                         const int32_t* __restrict__ res, int n_scans, uint32_t dst_max_n, const double* __restrict__ mats,
                                                         float4* __restrict__ dst, unsigned char* __restrict__ dst_ring, int* __restrict__ dst_counts) {
    scatter_tile<true>(v, img, n_tiles, tile_off, res, n_scans, dst_max_n, mats, dst, dst_ring, dst_counts);
}

int hip_fail(locgpu_ctx* ctx, hipError_t e, const char* what) {
    hip_ok(ctx, e, what);
    return e == hipErrorOutOfMemory ? LOCGPU_ERR_OOM : LOCGPU_ERR_NO_DEVICE;
}

}  // namespace

struct RangeIngestScratch {
    PinnedBuf<uint16_t> h_img;  // [n_scans][cells_pad]
    DevBuf<uint16_t> d_img;
    DevBuf<uint32_t> tile_cnt, tile_off;  // [n_scans][n_tiles]
    DevBuf<int32_t> res;                  // [n_scans + 2]
    PinnedBuf<int32_t> h_res;
    DevBuf<unsigned char> d_ring;         // the cloud form's ring bytes
    PinnedBuf<unsigned char> h_ring;
    Event staged;                         // behind the last H2D of the images on the copy stream
    // locgpu_profile_enable: timing events round the copies (copy stream) and round the four kernels (compute stream) of the most
    // recent pass, read by locgpu_range_ingest_times
    Event prof[4];
    bool prof_valid = false;
    double prof_ms[2] = {0, 0};
    // The deskewed calls: the motion of a call, times [n_scans][K] | poses [n_scans][K][7] | ref_times [n_scans], and the matrices
    // rd_pose_kernel made of it, [mats_scans][mats_cols][12], kept for locgpu_range_deskew_matrices. Events of their own, so that
    // locgpu_range_ingest_times goes on reporting the most recent PLAIN call: copies [0,1] on the copy stream; the matrix kernel
    // [2,3] and the four decode kernels [3,4] on the compute stream.
    PinnedBuf<double> h_motion;
    DevBuf<double> d_motion, d_mats;
    int mats_scans = 0;
    uint32_t mats_cols = 0;
    Event dprof[5];
    bool dprof_valid = false;
    double dprof_ms[3] = {0, 0, 0};
};

namespace {

RangeIngestScratch* scratch(locgpu_ctx* ctx) {
    if (!ctx->ringest) ctx->ringest = new RangeIngestScratch();
    return ctx->ringest;
}

hipError_t ensure(locgpu_ctx* ctx, size_t n_scans, size_t cells_pad, size_t n_tiles) {
    RangeIngestScratch* S = scratch(ctx);
    const size_t img = n_scans * cells_pad, tiles = n_scans * n_tiles;
    if (img > S->d_img.cap()) {
        const size_t cap = with_headroom(img);
        LOCGPU_TRY(S->h_img.alloc(cap));
        LOCGPU_TRY(S->d_img.alloc(cap));
    }
    if (tiles > S->tile_off.cap()) {
        const size_t cap = with_headroom(tiles);
        LOCGPU_TRY(S->tile_cnt.alloc(cap));
        LOCGPU_TRY(S->tile_off.alloc(cap));
    }
    if (n_scans + 2 > S->h_res.cap()) {
        const size_t cap = n_scans + 18;
        LOCGPU_TRY(S->res.alloc(cap));
        LOCGPU_TRY(S->h_res.alloc(cap));
    }
    return S->staged.ensure();
}

hipError_t ensure_deskew(locgpu_ctx* ctx, size_t n_scans, size_t K, size_t n_cols) {
    RangeIngestScratch* S = scratch(ctx);
    const size_t motion = n_scans * (8 * K + 1), mats = n_scans * n_cols * 12;
    if (motion > S->d_motion.cap()) {
        const size_t cap = with_headroom(motion);
        LOCGPU_TRY(S->h_motion.alloc(cap));
        LOCGPU_TRY(S->d_motion.alloc(cap));
    }
    if (mats > S->d_mats.cap()) {
        S->mats_scans = 0;
        LOCGPU_TRY(S->d_mats.alloc(with_headroom(mats)));
    }
    return hipSuccess;
}

// The call's knots and reference times → pinned staging → HBM on the copy stream, ahead of the images: `staged` covers them too.
hipError_t stage_motion(locgpu_ctx* ctx, const locgpu_sweep_motion& m, int n_scans) {
    RangeIngestScratch* S = ctx->ringest;
    const size_t nk = (size_t)n_scans * m.n_knots;
    std::memcpy(S->h_motion, m.knot_times, nk * sizeof(double));
    std::memcpy(S->h_motion + nk, m.knot_poses, 7 * nk * sizeof(double));
    std::memcpy(S->h_motion + 8 * nk, m.ref_times, (size_t)n_scans * sizeof(double));
    return hipMemcpyAsync(S->d_motion, S->h_motion, (8 * nk + n_scans) * sizeof(double), hipMemcpyHostToDevice, ctx->copy_stream);
}

// The images → pinned staging → HBM on the context's copy stream, in groups of scans of about 4 MB: a few host threads copy groups
// into the staging buffer and enqueue each group's H2D as soon as it is there, so the copies of the first groups run under the
// host copies of the later ones. ctx->stream then waits for the last of them.
hipError_t stage_images(locgpu_ctx* ctx, const uint16_t* const* images, int n_scans, size_t cells, size_t cells_pad) {
    RangeIngestScratch* S = ctx->ringest;
    const size_t scan_bytes = cells_pad * sizeof(uint16_t);
    const int per_group = (int)std::max<size_t>(1, (4u << 20) / scan_bytes);
    const int n_groups = (n_scans + per_group - 1) / per_group;
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int nt = std::min<int>(n_groups, (int)std::min<unsigned>(8u, std::max(2u, hw / 4)));  // the batch uploader's thread count
    std::atomic<int> next{0};
    std::atomic<int> err{(int)hipSuccess};
    auto worker = [&]() {
        (void)hipSetDevice(ctx->device);
        for (int g = next.fetch_add(1); g < n_groups && err.load() == (int)hipSuccess; g = next.fetch_add(1)) {
            const int s0 = g * per_group, s1 = std::min(n_scans, s0 + per_group);
            for (int s = s0; s < s1; ++s) std::memcpy(S->h_img + (size_t)s * cells_pad, images[s], cells * sizeof(uint16_t));
            const hipError_t e = hipMemcpyAsync(S->d_img + (size_t)s0 * cells_pad, S->h_img + (size_t)s0 * cells_pad, (size_t)(s1 - s0) * scan_bytes,
                                                hipMemcpyHostToDevice, ctx->copy_stream);
            if (e != hipSuccess) err = (int)e;
        }
    };
    std::vector<std::thread> th;
    for (int t = 1; t < nt; ++t) th.emplace_back(worker);
    worker();
    for (auto& t : th) t.join();
    LOCGPU_TRY((hipError_t)err.load());
    LOCGPU_TRY(hipEventRecord(S->staged, ctx->copy_stream));
    return hipStreamWaitEvent(ctx->stream, S->staged, 0);
}

// dk: the checked motion of a deskewed call (check_sweep_motion), or NULL.
// The pass for n_scans images into dst [n_scans][dst_max_n] (+ ring bytes, + device counts unless dst_counts is NULL), on
// ctx->stream; the counts and the verdict are on their way to S->h_res when it returns. dst_time (plain form of a sensor with column
// times only, else NULL): the survivors' time keys, [n_scans][dst_max_n].
hipError_t ingest_dev(locgpu_ctx* ctx, const locgpu_sensor* sn, const uint16_t* const* images, int n_scans, float4* dst, unsigned char* dst_ring, int* dst_counts,
                      uint32_t dst_max_n, const locgpu_sweep_motion* dk = nullptr, double* dst_time = nullptr) {
    const size_t cells = sn->cells(), cells_pad = (cells + kCellsPerLane - 1) / kCellsPerLane * kCellsPerLane;
    const uint32_t n_tiles = (uint32_t)((cells + kTile - 1) / kTile);
    LOCGPU_TRY(ensure(ctx, (size_t)n_scans, cells_pad, n_tiles));
    if (dk) LOCGPU_TRY(ensure_deskew(ctx, (size_t)n_scans, (size_t)dk->n_knots, sn->n_cols));
    RangeIngestScratch* S = ctx->ringest;
    const bool prof = ctx->profile != 0;
    // a deskewed call keeps its times apart: ev[0..1] round the copies, ev[2] ahead of the kernels, ev[3] behind them, and
    // dprof[3] doubles as the mark between the matrix kernel and the decode
    Event* ev[4] = {&S->prof[0], &S->prof[1], &S->prof[2], &S->prof[3]};
    if (dk) {
        ev[0] = &S->dprof[0], ev[1] = &S->dprof[1], ev[2] = &S->dprof[2], ev[3] = &S->dprof[4];
        S->dprof_valid = false;
        S->mats_scans = 0;
    } else {
        S->prof_valid = false;
    }
    if (prof) {
        for (Event& e : S->prof) LOCGPU_TRY(e.ensure(hipEventDefault));
        if (dk)
            for (Event& e : S->dprof) LOCGPU_TRY(e.ensure(hipEventDefault));
        LOCGPU_TRY(hipEventRecord(*ev[0], ctx->copy_stream));
    }
    if (dk) LOCGPU_TRY(stage_motion(ctx, *dk, n_scans));
    LOCGPU_TRY(stage_images(ctx, images, n_scans, cells, cells_pad));
    if (prof) {
        LOCGPU_TRY(hipEventRecord(*ev[1], ctx->copy_stream));
        LOCGPU_TRY(hipEventRecord(*ev[2], ctx->stream));
    }
    const float* t = sn->d_tables;
    SensorView v;
    v.cos_el = t;
    v.sin_el = t + sn->n_rings;
    v.cos_az = t + 2 * (size_t)sn->n_rings;
    v.sin_az = v.cos_az + sn->n_az();
    v.n_cols = sn->n_cols;
    v.cells = (uint32_t)cells;
    v.cells_pad = (uint32_t)cells_pad;
    v.az_per_ring = sn->az_per_ring;
    v.range_scale = sn->range_scale;
    v.min_range = sn->min_range;
    hipStream_t s = ctx->stream;
    if (dk) {
        hipLaunchKernelGGL(rd_pose_kernel, dim3(n_scans), dim3(kRI), 0, s, S->d_motion.get(), n_scans, dk->n_knots, sn->d_col_time.get(), sn->n_cols, S->d_mats.get());
        LOCGPU_TRY(hipGetLastError());
        S->mats_scans = n_scans;
        S->mats_cols = sn->n_cols;
        if (prof) LOCGPU_TRY(hipEventRecord(S->dprof[3], s));
    }
    hipLaunchKernelGGL(ri_count_kernel, dim3(n_tiles, n_scans), dim3(kRI), 0, s, v, S->d_img.get(), n_tiles, S->tile_cnt.get());
    ingest_launch_offsets(s, S->tile_cnt.get(), n_tiles, S->tile_off.get(), S->res.get(), n_scans, 1);
    ingest_launch_verdict(s, S->res.get(), n_scans, dst_max_n, 1);
    if (dk)
        hipLaunchKernelGGL(rd_scatter_kernel, dim3(n_tiles, n_scans), dim3(kRI), 0, s, v, S->d_img.get(), n_tiles, S->tile_off.get(), S->res.get(), n_scans, dst_max_n,
                           S->d_mats.get(), dst, dst_ring, dst_counts);
    else if (dst_time)
        hipLaunchKernelGGL(ri_scatter_times_kernel, dim3(n_tiles, n_scans), dim3(kRI), 0, s, v, S->d_img.get(), n_tiles, S->tile_off.get(), S->res.get(), n_scans, dst_max_n,
                           sn->d_col_time.get(), dst, dst_ring, dst_counts, dst_time);
    else
        hipLaunchKernelGGL(ri_scatter_kernel, dim3(n_tiles, n_scans), dim3(kRI), 0, s, v, S->d_img.get(), n_tiles, S->tile_off.get(), S->res.get(), n_scans, dst_max_n, dst,
                           dst_ring, dst_counts);
    LOCGPU_TRY(hipGetLastError());
    if (prof) {
        LOCGPU_TRY(hipEventRecord(*ev[3], s));
        (dk ? S->dprof_valid : S->prof_valid) = true;
    }
    return hipMemcpyAsync(S->h_res, S->res, ((size_t)n_scans + 2) * sizeof(int32_t), hipMemcpyDeviceToHost, s);
}

// Both streams have been waited for: the elapsed times of the pass that just ran.
void collect_times(locgpu_ctx* ctx) {
    RangeIngestScratch* S = ctx->ringest;
    if (!S->prof_valid) return;
    float copy_ms = 0.f, kernel_ms = 0.f;
    // the compute stream waited for `staged`, which is recorded just before prof[1] on the copy stream
    if (hipEventSynchronize(S->prof[1]) == hipSuccess && hipEventElapsedTime(&copy_ms, S->prof[0], S->prof[1]) == hipSuccess && hipEventElapsedTime(&kernel_ms, S->prof[2], S->prof[3]) == hipSuccess) {
        S->prof_ms[0] = copy_ms;
        S->prof_ms[1] = kernel_ms;
    }
}

void collect_deskew_times(locgpu_ctx* ctx) {
    RangeIngestScratch* S = ctx->ringest;
    if (!S->dprof_valid) return;
    float copy_ms = 0.f, pose_ms = 0.f, decode_ms = 0.f;
    if (hipEventSynchronize(S->dprof[1]) == hipSuccess && hipEventElapsedTime(&copy_ms, S->dprof[0], S->dprof[1]) == hipSuccess &&
        hipEventElapsedTime(&pose_ms, S->dprof[2], S->dprof[3]) == hipSuccess && hipEventElapsedTime(&decode_ms, S->dprof[3], S->dprof[4]) == hipSuccess) {
        S->dprof_ms[0] = copy_ms;
        S->dprof_ms[1] = pose_ms;
        S->dprof_ms[2] = decode_ms;
    }
}

bool bad_scalar(float x, bool allow_zero) { return !std::isfinite(x) || x < 0.f || (!allow_zero && x == 0.f); }

}  // namespace

void ingest_launch_offsets(hipStream_t s, const uint32_t* tile_cnt, uint32_t n_tiles, uint32_t* tile_off, int32_t* res, int n_scans, int rows) {
    hipLaunchKernelGGL(ri_offsets_kernel, dim3(n_scans, rows), dim3(kRI), 0, s, tile_cnt, n_tiles, tile_off, res, n_scans);
}

void ingest_launch_verdict(hipStream_t s, int32_t* res, int n_scans, uint32_t dst_max_n, int rows) {
    hipLaunchKernelGGL(ri_verdict_kernel, dim3(1), dim3(kRI), 0, s, res, n_scans, dst_max_n, rows);
}

int check_sweep_motion(locgpu_ctx* ctx, const std::string& who, const locgpu_sweep_motion* m, int n_scans, bool cols, double q_min, double q_max) {
    if (!m) return fail(ctx, LOCGPU_ERR_INVALID, who + ": motion is NULL");
    if (!m->knot_times || !m->knot_poses || !m->ref_times) return fail(ctx, LOCGPU_ERR_INVALID, who + ": a NULL array in the motion");
    const int K = m->n_knots;
    if (K < 2 || K > kMaxKnots) return fail(ctx, LOCGPU_ERR_INVALID, who + ": n_knots must be in 2..256");
    const std::string what = cols ? ": a column time or the reference time lies " : ": the reference time lies ";
    for (int i = 0; i < n_scans; ++i) {
        const double* t = m->knot_times + (size_t)i * K;
        const std::string scan = " (scan " + std::to_string(i) + ")";
        for (int k = 0; k < K; ++k)
            if (!std::isfinite(t[k]) || (k && !(t[k] > t[k - 1]))) return fail(ctx, LOCGPU_ERR_INVALID, who + ": knot times must be finite and strictly increasing" + scan);
        const double r = m->ref_times[i];
        if (!std::isfinite(r)) return fail(ctx, LOCGPU_ERR_INVALID, who + ": a reference time is not finite" + scan);
        if ((cols && q_min < t[0]) || r < t[0]) return fail(ctx, LOCGPU_ERR_INVALID, who + what + "before the first knot" + scan + "; nothing is extrapolated");
        if ((cols && q_max - t[K - 1] > kInterpTimeTh) || r - t[K - 1] > kInterpTimeTh)
            return fail(ctx, LOCGPU_ERR_INVALID, who + what + "more than 0.5 s behind the last knot" + scan);
    }
    return LOCGPU_OK;
}

void range_ingest_free(locgpu_ctx* ctx) {
    delete ctx->ringest;
    ctx->ringest = nullptr;
    for (locgpu_sensor* s : ctx->sensors) delete s;
    ctx->sensors.clear();
}

}  // namespace locgpu

using namespace locgpu;

extern "C" {

int locgpu_sensor_create(locgpu_ctx* ctx, const locgpu_sensor_model* m, locgpu_sensor** out) {
    if (!ctx) return fail(nullptr, LOCGPU_ERR_INVALID, "sensor_create: NULL context");
    if (out) *out = nullptr;
    if (!m || !out) return fail(ctx, LOCGPU_ERR_INVALID, "sensor_create: NULL model or out");
    if (m->n_rings < 1 || m->n_rings > kMaxRings) return fail(ctx, LOCGPU_ERR_INVALID, "sensor_create: n_rings must be in 1..256");
    if (m->n_cols < 1 || m->n_cols > kMaxCols) return fail(ctx, LOCGPU_ERR_INVALID, "sensor_create: n_cols must be in 1..12288");
    if (bad_scalar(m->range_scale, false)) return fail(ctx, LOCGPU_ERR_INVALID, "sensor_create: range_scale must be finite and positive");
    if (bad_scalar(m->min_range, true)) return fail(ctx, LOCGPU_ERR_INVALID, "sensor_create: min_range must be finite and not negative");
    if (m->az_per_ring != 0 && m->az_per_ring != 1) return fail(ctx, LOCGPU_ERR_INVALID, "sensor_create: az_per_ring must be 0 or 1");
    if (!m->cos_el || !m->sin_el || !m->cos_az || !m->sin_az) return fail(ctx, LOCGPU_ERR_INVALID, "sensor_create: NULL table");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    auto* s = new locgpu_sensor();
    s->ctx = ctx;
    s->n_rings = (uint32_t)m->n_rings;
    s->n_cols = (uint32_t)m->n_cols;
    s->az_per_ring = (uint32_t)m->az_per_ring;
    s->range_scale = m->range_scale;
    s->min_range = m->min_range;
    const size_t n_el = s->n_rings, n_az = s->n_az();
    std::vector<float> host(2 * n_el + 2 * n_az);
    std::memcpy(host.data(), m->cos_el, n_el * sizeof(float));
    std::memcpy(host.data() + n_el, m->sin_el, n_el * sizeof(float));
    std::memcpy(host.data() + 2 * n_el, m->cos_az, n_az * sizeof(float));
    std::memcpy(host.data() + 2 * n_el + n_az, m->sin_az, n_az * sizeof(float));
    hipError_t e = s->d_tables.alloc(host.size());
    // once per sensor, from pageable memory: the copy is complete when the stream has been waited for
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_tables, host.data(), host.size() * sizeof(float), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        delete s;
        return hip_fail(ctx, e, "sensor_create: tables");
    }
    ctx->sensors.push_back(s);
    *out = s;
    return LOCGPU_OK;
}

void locgpu_sensor_destroy(locgpu_sensor* s) {
    if (!s) return;
    locgpu_ctx* ctx = s->ctx;
    (void)hipSetDevice(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    ctx->sensors.erase(std::remove(ctx->sensors.begin(), ctx->sensors.end(), s), ctx->sensors.end());
    delete s;
}

int locgpu_sensor_set_col_times(locgpu_sensor* s, const double* col_time) {
    if (!s) return fail(nullptr, LOCGPU_ERR_INVALID, "sensor_set_col_times: NULL sensor");
    locgpu_ctx* ctx = s->ctx;
    if (!col_time) return fail(ctx, LOCGPU_ERR_INVALID, "sensor_set_col_times: col_time is NULL");
    double lo = col_time[0], hi = col_time[0];
    for (uint32_t c = 0; c < s->n_cols; ++c) {
        if (!std::isfinite(col_time[c])) return fail(ctx, LOCGPU_ERR_INVALID, "sensor_set_col_times: col_time[" + std::to_string(c) + "] is not finite");
        lo = std::min(lo, col_time[c]);
        hi = std::max(hi, col_time[c]);
    }
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    // a call that reads the previous table has ended (every ingest is blocking); once per table, from pageable memory, as the model's tables
    hipError_t e = s->d_col_time ? hipSuccess : s->d_col_time.alloc(s->n_cols);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_col_time, col_time, (size_t)s->n_cols * sizeof(double), hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        s->has_col_times = false;
        return hip_fail(ctx, e, "sensor_set_col_times: table");
    }
    s->has_col_times = true;
    s->col_time_min = lo;
    s->col_time_max = hi;
    return LOCGPU_OK;
}

}  // extern "C"

namespace {

// locgpu_batch_upload_ranges (motion == NULL and !deskew) and locgpu_batch_upload_ranges_deskew: the same refusals in the same order,
// then the motion's; nothing on the device is written before the last of them.
int batch_upload_ranges(locgpu_batch* b, const locgpu_sensor* s, const uint16_t* const* images, bool deskew, const locgpu_sweep_motion* motion, int32_t* out_counts) {
    const std::string who = deskew ? "batch_upload_ranges_deskew" : "batch_upload_ranges";
    if (!b) return fail(nullptr, LOCGPU_ERR_INVALID, who + ": NULL batch");
    locgpu_ctx* ctx = b->ctx;
    if (!s) return fail(ctx, LOCGPU_ERR_INVALID, who + ": NULL sensor");
    if (s->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, who + ": the sensor belongs to another context");
    if (b->shared_src) return fail(ctx, LOCGPU_ERR_INVALID, "batch upload: a shared-source batch takes its cloud when it is created");
    if (b->sharded) return fail(ctx, LOCGPU_ERR_INVALID, who + ": sharded batches are not supported");
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "batch upload: an alignment of this batch has been begun and not finished");
    if (!images) return fail(ctx, LOCGPU_ERR_INVALID, who + ": images is NULL");
    const int n_scans = b->n_scans;
    for (int i = 0; i < n_scans; ++i)
        if (!images[i]) return fail(ctx, LOCGPU_ERR_INVALID, who + ": images[" + std::to_string(i) + "] is NULL");
    if (deskew) {
        if (!s->has_col_times) return fail(ctx, LOCGPU_ERR_INVALID, who + ": the sensor has no column times (locgpu_sensor_set_col_times)");
        const int rc = check_sweep_motion(ctx, who, motion, n_scans, true, s->col_time_min, s->col_time_max);
        if (rc != LOCGPU_OK) return rc;
    }
    if (n_scans == 0) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    const int rc = order_behind_batch(ctx, b, (who + ": ordering behind the batch").c_str());
    if (rc != LOCGPU_OK) return rc;
    hipError_t e = b->d_rings ? hipSuccess : b->d_rings.alloc(std::max<size_t>(b->pitch, 1));
    if (e != hipSuccess) return hip_fail(ctx, e, (who + ": ring bytes").c_str());
    // locgpu_batch_keep_times: the plain form of a sensor with column times leaves the survivors' time keys; the deskewed form never does
    const bool times = !deskew && b->keep_times && s->has_col_times;
    if (e == hipSuccess && times && !b->d_times) e = b->d_times.alloc(std::max<size_t>(b->pitch, 1));
    if (e != hipSuccess) return hip_fail(ctx, e, (who + ": point times").c_str());
    e = ingest_dev(ctx, s, images, n_scans, b->d_src, b->d_rings, b->d_counts, (uint32_t)b->max_n, deskew ? motion : nullptr, times ? b->d_times.get() : nullptr);
    // the one read-back: when it is there the whole pass has run, and whatever uses the batch next — on any stream — finds it complete
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamSynchronize(ctx->stream);
        return hip_fail(ctx, e, who.c_str());
    }
    b->paced_tail = false;
    if (deskew) collect_deskew_times(ctx); else collect_times(ctx);
    const int32_t* res = ctx->ringest->h_res;
    if (out_counts) std::memcpy(out_counts, res, (size_t)n_scans * sizeof(int32_t));
    if (!res[n_scans])
        return fail(ctx, LOCGPU_ERR_INVALID, who + ": a decoded scan has " + std::to_string(res[n_scans + 1]) + " points, the batch was created for " +
                                                 std::to_string(b->max_n) + " per scan (the batch is unchanged)");
    set_host_counts(b, res);
    b->rings_valid = true;
    b->times_valid = times;
    return LOCGPU_OK;
}

}  // namespace

extern "C" {

int locgpu_batch_upload_ranges(locgpu_batch* b, const locgpu_sensor* s, const uint16_t* const* images, int32_t* out_counts) {
    return batch_upload_ranges(b, s, images, false, nullptr, out_counts);
}

int locgpu_batch_upload_ranges_deskew(locgpu_batch* b, const locgpu_sensor* s, const uint16_t* const* images, const locgpu_sweep_motion* motion, int32_t* out_counts) {
    return batch_upload_ranges(b, s, images, true, motion, out_counts);
}

int locgpu_range_deskew_matrices(locgpu_ctx* ctx, int scan, double* out, size_t capacity, size_t* n_cols_out) {
    if (!ctx) return fail(nullptr, LOCGPU_ERR_INVALID, "range_deskew_matrices: NULL context");
    RangeIngestScratch* S = ctx->ringest;
    if (!S || S->mats_scans == 0) return fail(ctx, LOCGPU_ERR_INVALID, "range_deskew_matrices: no deskewed ingest has run on this context");
    if (scan < 0 || scan >= S->mats_scans) return fail(ctx, LOCGPU_ERR_INVALID, "range_deskew_matrices: scan index out of range");
    if (n_cols_out) *n_cols_out = S->mats_cols;
    if (!out) return LOCGPU_OK;
    const size_t n = (size_t)S->mats_cols * 12;
    if (capacity < n) return fail(ctx, LOCGPU_ERR_INVALID, "range_deskew_matrices: capacity < 12 doubles per column");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipMemcpyAsync(out, S->d_mats + (size_t)scan * n, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "range_deskew_matrices: D2H");
    return LOCGPU_OK;
}

int locgpu_range_deskew_times(locgpu_ctx* ctx, double out_ms[3]) {
    if (!ctx || !out_ms) return fail(ctx, LOCGPU_ERR_INVALID, "range_deskew_times: NULL argument");
    for (int i = 0; i < 3; ++i) out_ms[i] = ctx->ringest ? ctx->ringest->dprof_ms[i] : 0.0;
    return LOCGPU_OK;
}

int locgpu_range_ingest_times(locgpu_ctx* ctx, double out_ms[2]) {
    if (!ctx || !out_ms) return fail(ctx, LOCGPU_ERR_INVALID, "range_ingest_times: NULL argument");
    out_ms[0] = ctx->ringest ? ctx->ringest->prof_ms[0] : 0.0;
    out_ms[1] = ctx->ringest ? ctx->ringest->prof_ms[1] : 0.0;
    return LOCGPU_OK;
}

int locgpu_batch_download_rings(locgpu_batch* b, int scan, uint8_t* out, size_t capacity, size_t* n) {
    if (!b) return fail(nullptr, LOCGPU_ERR_INVALID, "batch_download_rings: NULL batch");
    locgpu_ctx* ctx = b->ctx;
    if (!b->rings_valid) return fail(ctx, LOCGPU_ERR_INVALID, "batch_download_rings: the batch holds no resident rings");
    if (scan < 0 || scan >= b->n_scans) return fail(ctx, LOCGPU_ERR_INVALID, "batch_download_rings: scan index out of range");
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "batch_download_rings: an alignment of this batch has been begun and not finished");
    const size_t cnt = (size_t)b->counts[scan];
    if (n) *n = cnt;
    if (!out) return LOCGPU_OK;
    if (cnt > capacity) return fail(ctx, LOCGPU_ERR_INVALID, "batch_download_rings: capacity < the scan's size");
    if (cnt == 0) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    RangeIngestScratch* S = scratch(ctx);  // rings_valid: an ingest has run on this context, the range-image or the point-record one
    hipError_t e = S->h_ring.reserve(cnt);
    if (e == hipSuccess) e = hipMemcpyAsync(S->h_ring, b->d_rings + (size_t)scan * b->max_n, cnt, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "batch_download_rings: D2H");
    std::memcpy(out, S->h_ring, cnt);
    return LOCGPU_OK;
}

}  // extern "C"

namespace {

// locgpu_cloud_upload_ranges and locgpu_cloud_upload_ranges_deskew: as batch_upload_ranges above, for one image into a resident cloud.
int cloud_upload_ranges(locgpu_cloud* c, const locgpu_sensor* s, const uint16_t* image, bool deskew, const locgpu_sweep_motion* motion, uint8_t* ring_out, size_t* n) {
    const std::string who = deskew ? "cloud_upload_ranges_deskew" : "cloud_upload_ranges";
    if (!c) return fail(nullptr, LOCGPU_ERR_INVALID, who + ": NULL cloud");
    locgpu_ctx* ctx = c->ctx;
    if (!s) return fail(ctx, LOCGPU_ERR_INVALID, who + ": NULL sensor");
    if (s->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, who + ": the sensor belongs to another context");
    if (!image) return fail(ctx, LOCGPU_ERR_INVALID, who + ": image is NULL");
    if (deskew) {  // before the cloud is touched: a refusal leaves it as it was
        if (!s->has_col_times) return fail(ctx, LOCGPU_ERR_INVALID, who + ": the sensor has no column times (locgpu_sensor_set_col_times)");
        const int rc = check_sweep_motion(ctx, who, motion, 1, true, s->col_time_min, s->col_time_max);
        if (rc != LOCGPU_OK) return rc;
    }
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    const size_t cells = s->cells();
    hipError_t e = cloud_reserve(c, cells, false);  // room for every cell: this form has no capacity refusal
    RangeIngestScratch* S = scratch(ctx);
    if (e == hipSuccess && cells > S->d_ring.cap()) {
        const size_t cap = with_headroom(cells);
        e = S->d_ring.alloc(cap);
    }
    if (e == hipSuccess && ring_out) e = S->h_ring.reserve(with_headroom(cells));
    if (e != hipSuccess) return hip_fail(ctx, e, (who + ": buffers").c_str());
    e = ingest_dev(ctx, s, &image, 1, c->d, S->d_ring, nullptr, (uint32_t)cells, deskew ? motion : nullptr);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamSynchronize(ctx->stream);
        c->n = 0;
        return hip_fail(ctx, e, who.c_str());
    }
    if (deskew) collect_deskew_times(ctx); else collect_times(ctx);
    const size_t cnt = (size_t)S->h_res[0];
    if (ring_out && cnt) {
        e = hipMemcpyAsync(S->h_ring, S->d_ring, cnt, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, (who + ": ring bytes").c_str());
        std::memcpy(ring_out, S->h_ring, cnt);
    }
    c->n = cnt;
    c->is_dense = 1;  // every survivor is finite
    if (n) *n = cnt;
    (void)cloud_mark_ready(c);
    return LOCGPU_OK;
}

}  // namespace

extern "C" {

int locgpu_cloud_upload_ranges(locgpu_cloud* c, const locgpu_sensor* s, const uint16_t* image, uint8_t* ring_out, size_t* n) {
    return cloud_upload_ranges(c, s, image, false, nullptr, ring_out, n);
}

int locgpu_cloud_upload_ranges_deskew(locgpu_cloud* c, const locgpu_sensor* s, const uint16_t* image, const locgpu_sweep_motion* motion, uint8_t* ring_out, size_t* n) {
    return cloud_upload_ranges(c, s, image, true, motion, ring_out, n);
}

}  // extern "C"
