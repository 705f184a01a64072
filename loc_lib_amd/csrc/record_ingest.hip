// loc_lib_amd/csrc/record_ingest.hip — point records decoded in HBM (include/locgpu.h, "Point-record ingest").
//
// The reference's scans arrive as sensor_msgs::PointCloud2 blobs of driver-specific records (velodyne_ros::Point, ouster_ros::Point,
// rslidar_ros::Point — LocUtils/include/LocUtils/common/point_types.h:99-169) and CloudConver::Conver (LocUtils/src/subscriber/
// cloud_subscriber.cpp:7-29 and :31-58) makes the library's clouds of them: non-finite points and points nearer than 4.0 are dropped,
// the rest kept in input order, ring carried as one byte. This file takes the raw blobs — the host copies each once into pinned
// staging and never reads a field — and does that on the device for all scans of a call; the *_deskew forms also move every survivor
// into the sensor frame of a reference instant by math::PoseInterp (math_utils.h:470-517) at the point's OWN time.
//
// One pass, the shape of range_ingest.hip's; the blobs staged back to back, each scan's rows starting on a 16-byte boundary and padded
// by at least 4 bytes, so that the aligned dwords that cover the last record's last field are inside the allocation:
//
//   count    block (tile, scan): 256 lanes × 1 record, fields picked out of the covering dwords, Conver's two rules   rec_count_kernel
//            (conver_keep, range_ingest.hpp) → survivors of the tile; deskew form: and survivors with a refused time
//   offsets  per scan: exclusive sum of its tile counts in tile order, its total, its refused-time total (row 1)      ri_offsets_kernel
//   verdict  does every scan fit the destination, and is no survivor's time refused; the largest count               ri_verdict_kernel
//   scatter  block (tile, scan): pick again, compact the tile in LDS in input order (point with the intensity in     rec_scatter_kernel
//            lane w, ring byte, the time in the deskew form), then a store loop over survivors — deskew form:            <kDeskew>
//            rd_pose_at at the survivor's time on the scan's knots staged in LDS, the matrix against the scan's
//            reference pose (computed once per block by thread 0), transform_point_f64 — coalesced float4 stores;     <., kTimes>
//            plain form into a batch with locgpu_batch_keep_times on: the time KEY (double)field * time_scale goes
//            through the compaction instead and is stored beside the ring byte, for locgpu_batch_deskew (resident_deskew.hip)
//
// Scans have different lengths: the grid is (tiles of the longest scan, n_scans) and a tile past its scan's end counts 0. A
// survivor's position is the number of survivors before it in input order: no atomics, so counts, order and bits do not depend on
// n_scans, on the scan's place or on the run. Nothing is written when the verdict is 0.
//
// Reading a field at any byte offset: the aligned dwords that cover it are loaded and funnel-shifted (rec_words) — never a misaligned
// or a wide global load; neighbouring lanes read neighbouring records, so the dwords of one load instruction lie within
// 64 × stride bytes and every byte of a cache line is used by some lane.
//
// Scratch, grow-only on the context (record_ingest_free): the raw bytes pinned + in HBM, 8 B per scan of offsets and lengths, 4 B
// (8 B deskewed) per tile, 4 B (8 B) per scan of results (+ pinned), 8 B per knot value; with locgpu_records_deskew_debug on, 96 B per
// point slot of the destination; for the cloud form 1 B per record of ring bytes (+ pinned).
#include "record_ingest.hpp"

#include <algorithm>
#include <atomic>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "batch_upload.hpp"
#include "cloud_filters.hpp"
#include "context.hpp"
#include "pose_interp.hpp"
#include "range_ingest.hpp"

namespace locgpu {

namespace {

constexpr int kRecTile = kRI;  // records per block: one per lane
constexpr uint32_t kMinStride = 12, kMaxStride = 64;

// What the kernels know of a call: the staged bytes as dwords, per scan its first 16-byte unit and its length, and the layout.
struct RecView {
    const uint32_t* __restrict__ words;
    const uint32_t* __restrict__ n_pts;  // [n_scans]
    const uint32_t* __restrict__ off16;  // [n_scans]
    uint32_t stride, xyz_off, time_off, time_kind, ring_off, ring_kind, int_off, int_kind;
    float min_range;
    double time_scale;
};

// The NW dwords that start at byte address `byte` of the staging, as memcpy would read them: NW + 1 aligned dword loads, funnel-shifted.
// The last load is at most 4 bytes behind the field's end: inside the scan's padding.
template <int NW>
__device__ __forceinline__ void rec_words(const uint32_t* __restrict__ w, uint64_t byte, uint32_t (&out)[NW]) {
    const uint32_t* p = w + (byte >> 2);
    const uint32_t sh = ((uint32_t)byte & 3u) * 8u;
    uint32_t lo = p[0];
#pragma unroll
    for (int i = 0; i < NW; ++i) {
        const uint32_t hi = p[i + 1];
        out[i] = (uint32_t)((((uint64_t)hi << 32) | lo) >> sh);
        lo = hi;
    }
}

__device__ __forceinline__ uint32_t rec_byte(const uint32_t* __restrict__ w, uint64_t byte) { return (w[byte >> 2] >> (((uint32_t)byte & 3u) * 8u)) & 0xFFu; }

// Record at byte address `rec`: the raw point and whether Conver keeps it.
__device__ __forceinline__ bool rec_point(const RecView& v, uint64_t rec, float& x, float& y, float& z) {
    uint32_t q[3];
    rec_words<3>(v.words, rec + v.xyz_off, q);
    x = __uint_as_float(q[0]);
    y = __uint_as_float(q[1]);
    z = __uint_as_float(q[2]);
    return conver_keep(x, y, z, v.min_range);
}

// The point's time key: (double)field * time_scale, the first of the two IEEE double operations of the point's time — what a batch that
// keeps times (locgpu_batch_keep_times) stores per survivor.
__device__ __forceinline__ double rec_time_key(const RecView& v, uint64_t rec) {
    double f;
    if (v.time_kind == LOCGPU_TIME_F64) {
        uint32_t q[2];
        rec_words<2>(v.words, rec + v.time_off, q);
        f = __longlong_as_double((long long)(((uint64_t)q[1] << 32) | q[0]));
    } else {
        uint32_t q[1];
        rec_words<1>(v.words, rec + v.time_off, q);
        f = v.time_kind == LOCGPU_TIME_F32 ? (double)__uint_as_float(q[0]) : (double)q[0];
    }
    double key;
    {
#pragma clang fp contract(off)
        key = f * v.time_scale;
    }
    return key;
}

// The point's time: (double)field * time_scale + offset, two IEEE double operations.
__device__ __forceinline__ double rec_time(const RecView& v, uint64_t rec, double offset) {
    const double scaled = rec_time_key(v, rec);
    double tp;
    {
#pragma clang fp contract(off)
        tp = scaled + offset;
    }
    return tp;
}

__device__ __forceinline__ uint32_t rec_ring(const RecView& v, uint64_t rec) {
    return v.ring_kind == LOCGPU_RING_NONE ? 0u : rec_byte(v.words, rec + v.ring_off);  // U16, little-endian: (uint8_t)ring is its first byte
}

__device__ __forceinline__ float rec_intensity(const RecView& v, uint64_t rec) {
    if (v.int_kind == LOCGPU_INTENSITY_F32) {
        uint32_t q[1];
        rec_words<1>(v.words, rec + v.int_off, q);
        return __uint_as_float(q[0]);
    }
    if (v.int_kind == LOCGPU_INTENSITY_U8) return (float)rec_byte(v.words, rec + v.int_off);
    return 0.f;
}

// motion = times [n_scans][K] | poses [n_scans][K][7] | ref_times [n_scans] | time_offsets [n_scans]
__device__ __forceinline__ double motion_time_offset(const double* __restrict__ motion, int n_scans, int K, uint32_t s) { return motion[(size_t)n_scans * (8 * K + 1) + s]; }

// tile_cnt [rows][n_scans][n_tiles]: row 0 the tile's survivors, row 1 (motion != NULL) its survivors with a refused time.
__global__ __launch_bounds__(kRI) void rec_count_kernel(RecView v, uint32_t n_tiles, int n_scans, const double* __restrict__ motion, int K, uint32_t* __restrict__ tile_cnt) {
    __shared__ uint32_t s_wave[kRI / 64];
    const uint32_t s = blockIdx.y, tile = blockIdx.x;
    const uint32_t i = tile * kRecTile + threadIdx.x;
    uint32_t x = 0;  // survivor | refused << 16: both sums are at most 256
    if (i < v.n_pts[s]) {
        const uint64_t rec = (uint64_t)v.off16[s] * 16u + (uint64_t)i * v.stride;
        float px, py, pz;
        if (rec_point(v, rec, px, py, pz)) {
            x = 1;
            if (motion) {
                const double* t = motion + (size_t)s * K;
                const double tp = rec_time(v, rec, motion_time_offset(motion, n_scans, K, s));
                if (!isfinite(tp) || tp < t[0] || tp - t[K - 1] > kInterpTimeTh) x |= 1u << 16;
            }
        }
    }
    uint32_t total;
    (void)block_exclusive(x, s_wave, total);
    if (threadIdx.x == 0) {
        const size_t at = (size_t)s * n_tiles + tile;
        tile_cnt[at] = total & 0xFFFFu;
        if (motion) tile_cnt[(size_t)n_scans * n_tiles + at] = total >> 16;
    }
}

// Tile (blockIdx.x, scan blockIdx.y) → dst + s · dst_max_n + tile offset, {x, y, z, intensity or +0}, and the ring bytes beside it.
// kDeskew: each survivor is moved by the matrix of its own time; dbg (NULL unless locgpu_records_deskew_debug is on) receives it.
// kTimes (plain form only, a batch with locgpu_batch_keep_times on): the survivor's time key rec_time_key goes through the compaction
// and into dst_time beside the ring byte.
template <bool kDeskew, bool kTimes = false>
__global__ __launch_bounds__(kRI) void rec_scatter_kernel(RecView v, uint32_t n_tiles, const uint32_t* __restrict__ tile_off, const int32_t* __restrict__ res, int n_scans,
                                                          uint32_t dst_max_n, const double* __restrict__ motion, int K, double* __restrict__ dbg, float4* __restrict__ dst,
                                                          unsigned char* __restrict__ dst_ring, int* __restrict__ dst_counts, double* __restrict__ dst_time) {
    static_assert(!(kDeskew && kTimes), "deskewed points are no longer raw: they leave no times");
    if (res[n_scans] == 0) return;  // the same for every thread of the grid
    __shared__ float4 s_pts[kRecTile];
    __shared__ double s_tp[kDeskew || kTimes ? kRecTile : 1];
    __shared__ unsigned char s_ring[kRecTile];
    __shared__ uint32_t s_wave[kRI / 64];
    __shared__ double s_t[kDeskew ? kMaxKnots : 1];
    __shared__ double s_p[kDeskew ? kMaxKnots * 7 : 1];
    __shared__ double s_ref[12];  // R_r, t_r
    const uint32_t s = blockIdx.y, tile = blockIdx.x;
    if (tile == 0 && threadIdx.x == 0 && dst_counts) dst_counts[s] = res[s];
    const uint32_t n = v.n_pts[s];
    if (tile * kRecTile >= n) return;  // the same for every thread of the block
    if constexpr (kDeskew) {
        const double* g_t = motion + (size_t)s * K;
        const double* g_p = motion + (size_t)n_scans * K + (size_t)s * K * 7;
        for (int i = threadIdx.x; i < K; i += kRI) s_t[i] = g_t[i];
        for (int i = threadIdx.x; i < 7 * K; i += kRI) s_p[i] = g_p[i];
        __syncthreads();
        // the same inputs through the same function in every block of the scan: the same bits; the barriers below publish it
        if (threadIdx.x == 0) rd_ref_pose(s_t, s_p, K, motion[(size_t)n_scans * K * 8 + s], s_ref);
    }
    const uint32_t i = tile * kRecTile + threadIdx.x;
    const uint64_t rec = (uint64_t)v.off16[s] * 16u + (uint64_t)i * v.stride;
    float px = 0.f, py = 0.f, pz = 0.f;
    const bool keep = i < n && rec_point(v, rec, px, py, pz);
    uint32_t total;
    const uint32_t at = block_exclusive(keep ? 1u : 0u, s_wave, total);  // total <= kRecTile, at < total for a survivor
    if (keep) {
        s_pts[at] = float4{px, py, pz, rec_intensity(v, rec)};
        s_ring[at] = (unsigned char)rec_ring(v, rec);
        if constexpr (kDeskew) s_tp[at] = rec_time(v, rec, motion_time_offset(motion, n_scans, K, s));
        if constexpr (kTimes) s_tp[at] = rec_time_key(v, rec);
    }
    __syncthreads();
    // tile_off + total <= res[s] <= dst_max_n (the verdict): every store below is inside scan s's rows
    const size_t out = (size_t)s * dst_max_n + tile_off[(size_t)s * n_tiles + tile];
    for (uint32_t j = threadIdx.x; j < total; j += kRI) {
        if constexpr (kDeskew) {
            double m[12];
            const float4 moved = rd_move_point(s_t, s_p, K, s_ref, s_tp[j], s_pts[j], m);
            if (dbg) {  // the same for every thread of the grid; sized n_scans · dst_max_n matrices (ensure_debug)
#pragma unroll
                for (int k = 0; k < 12; ++k) dbg[(out + j) * 12 + k] = m[k];
            }
            dst[out + j] = moved;
        } else {
            dst[out + j] = s_pts[j];
        }
        if constexpr (kTimes) dst_time[out + j] = s_tp[j];  // [n_scans][dst_max_n], the layout of dst
        if (dst_ring) dst_ring[out + j] = s_ring[j];
    }
}

int hip_fail(locgpu_ctx* ctx, hipError_t e, const char* what) {
    hip_ok(ctx, e, what);
    return e == hipErrorOutOfMemory ? LOCGPU_ERR_OOM : LOCGPU_ERR_NO_DEVICE;
}

}  // namespace

struct RecordIngestScratch {
    PinnedBuf<unsigned char> h_bytes;  // the blobs back to back, each scan on a 16-byte boundary
    DevBuf<unsigned char> d_bytes;
    PinnedBuf<uint32_t> h_meta;        // n_pts [n_scans] | off16 [n_scans]
    DevBuf<uint32_t> d_meta;
    DevBuf<uint32_t> tile_cnt, tile_off;  // [2][n_scans][n_tiles], [n_scans][n_tiles]
    DevBuf<int32_t> res;                  // counts [n_scans] | verdict | largest | refused times [n_scans]
    PinnedBuf<int32_t> h_res;
    PinnedBuf<double> h_motion;  // times [n_scans][K] | poses [n_scans][K][7] | ref_times [n_scans] | time_offsets [n_scans]
    DevBuf<double> d_motion;
    DevBuf<unsigned char> d_ring;  // the cloud form's ring bytes
    PinnedBuf<unsigned char> h_ring;
    Event staged;  // behind the last H2D on the copy stream
    // locgpu_records_deskew_debug: the matrices of the most recent deskewed call that ran with it on, [dbg_scans][dbg_pitch][12]
    bool debug = false;
    DevBuf<double> d_dbg;
    int dbg_scans = 0;
    size_t dbg_pitch = 0;
    std::vector<int32_t> dbg_counts;
    // locgpu_profile_enable: copies [0,1] on the copy stream, kernels [2,3] on the compute stream
    Event prof[4];
    bool prof_valid = false;
    double prof_ms[2] = {0, 0};
};

namespace {

RecordIngestScratch* scratch(locgpu_ctx* ctx) {
    if (!ctx->recingest) ctx->recingest = new RecordIngestScratch();
    return ctx->recingest;
}

template <typename B>
hipError_t grow(B& buf, size_t n) {
    return n <= buf.cap() ? hipSuccess : buf.alloc(with_headroom(n));
}

// One call: the checked arguments of an entry point.
struct RecCall {
    const locgpu_point_layout* layout;
    const void* const* records;
    const int64_t* n_points;
    int n_scans;
    const double* time_offsets;        // deskew forms
    const locgpu_sweep_motion* motion;  // deskew forms, else NULL
    bool intensity;                     // the cloud forms
};

size_t scan_bytes_padded(const locgpu_point_layout& L, int64_t n) { return ((size_t)n * L.stride_bytes + 4 + 15) / 16 * 16; }

// The blobs → pinned staging → HBM on the copy stream, in groups of consecutive scans of about 4 MB: a few host threads copy groups —
// one memcpy per scan, no field is read — and enqueue each group's H2D as soon as it is there.
hipError_t stage_records(locgpu_ctx* ctx, const RecCall& c, const std::vector<size_t>& off) {
    RecordIngestScratch* S = ctx->recingest;
    const int n_scans = c.n_scans;
    std::vector<int> first;  // the first scan of every group, and n_scans
    for (int s = 0; s < n_scans; ++s)
        if (first.empty() || off[s] - off[first.back()] >= (4u << 20)) first.push_back(s);
    const int n_groups = (int)first.size();
    first.push_back(n_scans);
    const unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    const int nt = std::min<int>(n_groups, (int)std::min<unsigned>(8u, std::max(2u, hw / 4)));  // the batch uploader's thread count
    std::atomic<int> next{0};
    std::atomic<int> err{(int)hipSuccess};
    auto worker = [&]() {
        (void)hipSetDevice(ctx->device);
        for (int g = next.fetch_add(1); g < n_groups && err.load() == (int)hipSuccess; g = next.fetch_add(1)) {
            const int s0 = first[g], s1 = first[g + 1];
            for (int s = s0; s < s1; ++s)
                if (c.n_points[s] > 0) std::memcpy(S->h_bytes + off[s], c.records[s], (size_t)c.n_points[s] * c.layout->stride_bytes);
            const size_t bytes = off[s1] - off[s0];
            if (bytes == 0) continue;
            const hipError_t e = hipMemcpyAsync(S->d_bytes + off[s0], S->h_bytes + off[s0], bytes, hipMemcpyHostToDevice, ctx->copy_stream);
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

// The pass for c.n_scans blobs into dst [n_scans][dst_max_n] (+ ring bytes unless dst_ring is NULL, + device counts unless dst_counts
// is NULL, + the survivors' time keys [n_scans][dst_max_n] unless dst_time is NULL: plain form of a layout with a time field only) on
// ctx->stream; counts, verdict and refused-time counts are on their way to S->h_res when it returns.
hipError_t records_dev(locgpu_ctx* ctx, const RecCall& c, float4* dst, unsigned char* dst_ring, int* dst_counts, uint32_t dst_max_n, double* dst_time = nullptr) {
    RecordIngestScratch* S = scratch(ctx);
    const locgpu_point_layout& L = *c.layout;
    const int n_scans = c.n_scans, K = c.motion ? c.motion->n_knots : 0, rows = c.motion ? 2 : 1;
    std::vector<size_t> off((size_t)n_scans + 1, 0);
    int64_t longest = 0;
    for (int s = 0; s < n_scans; ++s) {
        off[s + 1] = off[s] + scan_bytes_padded(L, c.n_points[s]);
        longest = std::max(longest, c.n_points[s]);
    }
    const uint32_t n_tiles = (uint32_t)std::max<int64_t>(1, (longest + kRecTile - 1) / kRecTile);
    const size_t tiles = (size_t)n_scans * n_tiles, n_res = (size_t)rows * n_scans + 2, n_motion = c.motion ? (size_t)n_scans * (8 * K + 2) : 0;
    if (off[n_scans] / 16 > 0xFFFFFFFFull) return hipErrorInvalidValue;
    LOCGPU_TRY(grow(S->h_bytes, off[n_scans] + 16));
    LOCGPU_TRY(grow(S->d_bytes, off[n_scans] + 16));
    LOCGPU_TRY(grow(S->h_meta, 2 * (size_t)n_scans));
    LOCGPU_TRY(grow(S->d_meta, 2 * (size_t)n_scans));
    LOCGPU_TRY(grow(S->tile_cnt, 2 * tiles));
    LOCGPU_TRY(grow(S->tile_off, tiles));
    LOCGPU_TRY(grow(S->res, n_res));
    LOCGPU_TRY(grow(S->h_res, n_res));
    if (c.motion) {
        LOCGPU_TRY(grow(S->h_motion, n_motion));
        LOCGPU_TRY(grow(S->d_motion, n_motion));
    }
    double* dbg = nullptr;
    if (c.motion) S->dbg_scans = 0;
    if (c.motion && S->debug) {
        LOCGPU_TRY(grow(S->d_dbg, std::max<size_t>((size_t)n_scans * dst_max_n * 12, 12)));
        dbg = S->d_dbg;
    }
    LOCGPU_TRY(S->staged.ensure());
    const bool prof = ctx->profile != 0;
    S->prof_valid = false;
    if (prof) {
        for (Event& e : S->prof) LOCGPU_TRY(e.ensure(hipEventDefault));
        LOCGPU_TRY(hipEventRecord(S->prof[0], ctx->copy_stream));
    }
    for (int s = 0; s < n_scans; ++s) {
        S->h_meta[s] = (uint32_t)c.n_points[s];
        S->h_meta[n_scans + s] = (uint32_t)(off[s] / 16);
    }
    LOCGPU_TRY(hipMemcpyAsync(S->d_meta, S->h_meta, 2 * (size_t)n_scans * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->copy_stream));
    if (c.motion) {
        const size_t nk = (size_t)n_scans * K;
        std::memcpy(S->h_motion, c.motion->knot_times, nk * sizeof(double));
        std::memcpy(S->h_motion + nk, c.motion->knot_poses, 7 * nk * sizeof(double));
        std::memcpy(S->h_motion + 8 * nk, c.motion->ref_times, (size_t)n_scans * sizeof(double));
        std::memcpy(S->h_motion + 8 * nk + n_scans, c.time_offsets, (size_t)n_scans * sizeof(double));
        LOCGPU_TRY(hipMemcpyAsync(S->d_motion, S->h_motion, n_motion * sizeof(double), hipMemcpyHostToDevice, ctx->copy_stream));
    }
    LOCGPU_TRY(stage_records(ctx, c, off));
    if (prof) {
        LOCGPU_TRY(hipEventRecord(S->prof[1], ctx->copy_stream));
        LOCGPU_TRY(hipEventRecord(S->prof[2], ctx->stream));
    }
    RecView v;
    v.words = reinterpret_cast<const uint32_t*>(S->d_bytes.get());
    v.n_pts = S->d_meta.get();
    v.off16 = S->d_meta.get() + n_scans;
    v.stride = L.stride_bytes;
    v.xyz_off = L.xyz_offset;
    v.time_off = L.time_offset;
    v.time_kind = c.motion || dst_time ? L.time_kind : (uint32_t)LOCGPU_TIME_NONE;
    v.ring_off = L.ring_offset;
    v.ring_kind = L.ring_kind;
    v.int_off = L.intensity_offset;
    v.int_kind = c.intensity ? L.intensity_kind : (uint32_t)LOCGPU_INTENSITY_NONE;
    v.min_range = L.min_range;
    v.time_scale = L.time_scale;
    const double* motion = c.motion ? S->d_motion.get() : nullptr;
    unsigned char* ring = L.ring_kind != LOCGPU_RING_NONE ? dst_ring : nullptr;
    hipStream_t s = ctx->stream;
    const dim3 grid(n_tiles, n_scans);
    hipLaunchKernelGGL(rec_count_kernel, grid, dim3(kRI), 0, s, v, n_tiles, n_scans, motion, K, S->tile_cnt.get());
    ingest_launch_offsets(s, S->tile_cnt.get(), n_tiles, S->tile_off.get(), S->res.get(), n_scans, rows);
    ingest_launch_verdict(s, S->res.get(), n_scans, dst_max_n, rows);
    if (c.motion)
        hipLaunchKernelGGL(rec_scatter_kernel<true>, grid, dim3(kRI), 0, s, v, n_tiles, S->tile_off.get(), S->res.get(), n_scans, dst_max_n, motion, K, dbg, dst, ring, dst_counts,
                           (double*)nullptr);
    else if (dst_time)
        hipLaunchKernelGGL((rec_scatter_kernel<false, true>), grid, dim3(kRI), 0, s, v, n_tiles, S->tile_off.get(), S->res.get(), n_scans, dst_max_n, motion, K, dbg, dst, ring,
                           dst_counts, dst_time);
    else
        hipLaunchKernelGGL(rec_scatter_kernel<false>, grid, dim3(kRI), 0, s, v, n_tiles, S->tile_off.get(), S->res.get(), n_scans, dst_max_n, motion, K, dbg, dst, ring, dst_counts,
                           (double*)nullptr);
    LOCGPU_TRY(hipGetLastError());
    if (prof) {
        LOCGPU_TRY(hipEventRecord(S->prof[3], s));
        S->prof_valid = true;
    }
    if (dbg) S->dbg_pitch = dst_max_n;
    return hipMemcpyAsync(S->h_res, S->res, n_res * sizeof(int32_t), hipMemcpyDeviceToHost, s);
}

// Both streams have been waited for: the elapsed times of the pass that just ran.
void collect_times(locgpu_ctx* ctx) {
    RecordIngestScratch* S = ctx->recingest;
    if (!S->prof_valid) return;
    float copy_ms = 0.f, kernel_ms = 0.f;
    // the compute stream waited for `staged`, which is recorded just before prof[1] on the copy stream
    if (hipEventSynchronize(S->prof[1]) == hipSuccess && hipEventElapsedTime(&copy_ms, S->prof[0], S->prof[1]) == hipSuccess &&
        hipEventElapsedTime(&kernel_ms, S->prof[2], S->prof[3]) == hipSuccess) {
        S->prof_ms[0] = copy_ms;
        S->prof_ms[1] = kernel_ms;
    }
}

// A deskewed pass has run to its end with the debug switch on and was not refused: its matrices are what
// locgpu_records_deskew_matrices reports.
void keep_debug(locgpu_ctx* ctx, const RecCall& c) {
    RecordIngestScratch* S = ctx->recingest;
    if (!c.motion || !S->debug) return;
    S->dbg_scans = c.n_scans;
    S->dbg_counts.assign(S->h_res.get(), S->h_res.get() + c.n_scans);
}

struct Field {
    const char* name;
    uint32_t off, size;
};

bool field_size(uint32_t kind, const uint32_t* sizes, int n_kinds, uint32_t& size) {
    if (kind >= (uint32_t)n_kinds) return false;
    size = sizes[kind];
    return true;
}

// The refusals of a layout, host only (ctx may be NULL): LOCGPU_OK, or LOCGPU_ERR_INVALID with the text set.
int check_layout(locgpu_ctx* ctx, const std::string& who, const locgpu_point_layout* L, bool deskew) {
    if (!L) return fail(ctx, LOCGPU_ERR_INVALID, who + ": layout is NULL");
    if (L->stride_bytes < kMinStride || L->stride_bytes > kMaxStride) return fail(ctx, LOCGPU_ERR_INVALID, who + ": stride_bytes must be in 12..64");
    static const uint32_t time_sizes[] = {0, 4, 8, 4}, ring_sizes[] = {0, 1, 2}, int_sizes[] = {0, 4, 1};
    Field f[4] = {{"xyz", L->xyz_offset, 12}, {"time", L->time_offset, 0}, {"ring", L->ring_offset, 0}, {"intensity", L->intensity_offset, 0}};
    if (!field_size(L->time_kind, time_sizes, 4, f[1].size)) return fail(ctx, LOCGPU_ERR_INVALID, who + ": unknown time_kind");
    if (!field_size(L->ring_kind, ring_sizes, 3, f[2].size)) return fail(ctx, LOCGPU_ERR_INVALID, who + ": unknown ring_kind");
    if (!field_size(L->intensity_kind, int_sizes, 3, f[3].size)) return fail(ctx, LOCGPU_ERR_INVALID, who + ": unknown intensity_kind");
    for (const Field& x : f) {
        if (x.size == 0) continue;
        // offset + size > stride without overflow: size <= 12 <= stride
        if (x.off > L->stride_bytes - x.size) return fail(ctx, LOCGPU_ERR_INVALID, who + ": the " + x.name + " field does not fit stride_bytes (offset + size > stride_bytes)");
        if (&x != &f[0] && x.off < f[0].off + 12 && f[0].off < x.off + x.size) return fail(ctx, LOCGPU_ERR_INVALID, who + ": the " + x.name + " field overlaps xyz");
    }
    if (deskew && L->time_kind == LOCGPU_TIME_NONE) return fail(ctx, LOCGPU_ERR_INVALID, who + ": a deskewed ingest needs a time field (time_kind is LOCGPU_TIME_NONE)");
    if (!std::isfinite(L->min_range) || L->min_range < 0.f) return fail(ctx, LOCGPU_ERR_INVALID, who + ": min_range must be finite and not negative");
    if (!std::isfinite(L->time_scale) || L->time_scale == 0.0) return fail(ctx, LOCGPU_ERR_INVALID, who + ": time_scale must be finite and not 0");
    return LOCGPU_OK;
}

// The text of a time refusal: the first scan with a refused survivor time, and how many.
std::string time_refusal(const int32_t* bad, int n_scans, const char* target) {
    int i = 0;
    while (i < n_scans && bad[i] == 0) ++i;
    return ": scan " + std::to_string(i) + " has " + std::to_string(bad[i]) +
           " survivors whose time is not finite, lies before the first knot or more than 0.5 s behind the last knot (the " + target + " is unchanged)";
}

int batch_upload_records(locgpu_batch* b, const locgpu_point_layout* layout, const void* const* records, const int64_t* n_points, bool deskew, const double* time_offsets,
                         const locgpu_sweep_motion* motion, int32_t* out_counts, int32_t* out_status) {
    const std::string who = deskew ? "batch_upload_records_deskew" : "batch_upload_records";
    locgpu_ctx* ctx = b ? b->ctx : nullptr;
    int rc = check_layout(ctx, who, layout, deskew);  // argument checks first: they need neither a batch nor a device
    if (rc != LOCGPU_OK) return rc;
    if (!b) return fail(nullptr, LOCGPU_ERR_INVALID, who + ": NULL batch");
    if (b->shared_src) return fail(ctx, LOCGPU_ERR_INVALID, "batch upload: a shared-source batch takes its cloud when it is created");
    if (b->sharded) return fail(ctx, LOCGPU_ERR_INVALID, who + ": sharded batches are not supported");
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, "batch upload: an alignment of this batch has been begun and not finished");
    const int n_scans = b->n_scans;
    if (n_scans > 0 && (!records || !n_points)) return fail(ctx, LOCGPU_ERR_INVALID, who + ": records or n_points is NULL");
    for (int i = 0; i < n_scans; ++i) {
        if (n_points[i] < 0 || n_points[i] > (int64_t)b->max_n * 16)
            return fail(ctx, LOCGPU_ERR_INVALID, who + ": n_points[" + std::to_string(i) + "] must be in 0..16 x the batch's max_points_per_scan");
        if (n_points[i] > 0 && !records[i]) return fail(ctx, LOCGPU_ERR_INVALID, who + ": records[" + std::to_string(i) + "] is NULL");
    }
    if (deskew) {
        if (n_scans > 0 && !time_offsets) return fail(ctx, LOCGPU_ERR_INVALID, who + ": time_offsets is NULL");
        for (int i = 0; i < n_scans; ++i)
            if (!std::isfinite(time_offsets[i])) return fail(ctx, LOCGPU_ERR_INVALID, who + ": time_offsets[" + std::to_string(i) + "] is not finite");
        rc = check_sweep_motion(ctx, who, motion, n_scans, false, 0.0, 0.0);
        if (rc != LOCGPU_OK) return rc;
    }
    if (out_status) std::fill(out_status, out_status + n_scans, 0);
    if (n_scans == 0) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    rc = order_behind_batch(ctx, b, (who + ": ordering behind the batch").c_str());
    if (rc != LOCGPU_OK) return rc;
    const bool rings = layout->ring_kind != LOCGPU_RING_NONE;
    hipError_t e = !rings || b->d_rings ? hipSuccess : b->d_rings.alloc(std::max<size_t>(b->pitch, 1));
    if (e != hipSuccess) return hip_fail(ctx, e, (who + ": ring bytes").c_str());
    // locgpu_batch_keep_times: the plain form of a layout with a time field leaves the survivors' time keys; a deskewed form never does
    const bool times = !deskew && b->keep_times && layout->time_kind != LOCGPU_TIME_NONE;
    e = !times || b->d_times ? hipSuccess : b->d_times.alloc(std::max<size_t>(b->pitch, 1));
    if (e != hipSuccess) return hip_fail(ctx, e, (who + ": point times").c_str());
    const RecCall c{layout, records, n_points, n_scans, time_offsets, deskew ? motion : nullptr, false};
    e = records_dev(ctx, c, b->d_src, b->d_rings, b->d_counts, (uint32_t)b->max_n, times ? b->d_times.get() : nullptr);
    // the one read-back: when it is there the whole pass has run, and whatever uses the batch next — on any stream — finds it complete
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamSynchronize(ctx->stream);
        return hip_fail(ctx, e, who.c_str());
    }
    b->paced_tail = false;
    collect_times(ctx);
    const int32_t* res = ctx->recingest->h_res;
    if (out_counts) std::memcpy(out_counts, res, (size_t)n_scans * sizeof(int32_t));
    if (!res[n_scans]) {
        const int32_t* bad = res + n_scans + 2;
        if (deskew && std::any_of(bad, bad + n_scans, [](int32_t x) { return x != 0; })) {
            if (out_status)
                for (int i = 0; i < n_scans; ++i) out_status[i] = bad[i] != 0;
            return fail(ctx, LOCGPU_ERR_INVALID, who + time_refusal(bad, n_scans, "batch"));
        }
        return fail(ctx, LOCGPU_ERR_INVALID, who + ": a scan has " + std::to_string(res[n_scans + 1]) + " survivors, the batch was created for " + std::to_string(b->max_n) +
                                                 " per scan (the batch is unchanged)");
    }
    keep_debug(ctx, c);
    set_host_counts(b, res);
    b->rings_valid = rings;
    b->times_valid = times;
    return LOCGPU_OK;
}

int cloud_upload_records(locgpu_cloud* cl, const locgpu_point_layout* layout, const void* records, int64_t n, bool deskew, double time_offset,
                         const locgpu_sweep_motion* motion, uint8_t* ring_out, size_t* n_out) {
    const std::string who = deskew ? "cloud_upload_records_deskew" : "cloud_upload_records";
    locgpu_ctx* ctx = cl ? cl->ctx : nullptr;
    int rc = check_layout(ctx, who, layout, deskew);
    if (rc != LOCGPU_OK) return rc;
    if (!cl) return fail(nullptr, LOCGPU_ERR_INVALID, who + ": NULL cloud");
    if (n < 0 || n > 0x7FFFFFFF) return fail(ctx, LOCGPU_ERR_INVALID, who + ": n must be in 0..2^31 - 1");
    if (n > 0 && !records) return fail(ctx, LOCGPU_ERR_INVALID, who + ": records is NULL");
    if (deskew) {  // before the cloud is touched: a refusal leaves it as it was
        if (!std::isfinite(time_offset)) return fail(ctx, LOCGPU_ERR_INVALID, who + ": time_offset is not finite");
        rc = check_sweep_motion(ctx, who, motion, 1, false, 0.0, 0.0);
        if (rc != LOCGPU_OK) return rc;
    }
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    RecordIngestScratch* S = scratch(ctx);
    const bool rings = layout->ring_kind != LOCGPU_RING_NONE;
    // room for every record: this form has no capacity refusal. A deskewed call may still be refused for a survivor's time, and then
    // the cloud keeps its points: a growth carries them over.
    hipError_t e = cloud_reserve(cl, std::max<size_t>((size_t)n, 1), deskew);
    if (e == hipSuccess && rings) e = grow(S->d_ring, (size_t)n + 1);
    if (e == hipSuccess && rings && ring_out) e = grow(S->h_ring, (size_t)n + 1);
    if (e != hipSuccess) return hip_fail(ctx, e, (who + ": buffers").c_str());
    const RecCall c{layout, &records, &n, 1, &time_offset, deskew ? motion : nullptr, true};
    e = records_dev(ctx, c, cl->d, S->d_ring, nullptr, (uint32_t)n);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamSynchronize(ctx->stream);
        cl->n = 0;
        return hip_fail(ctx, e, who.c_str());
    }
    collect_times(ctx);
    const int32_t* res = S->h_res;
    if (!res[1]) return fail(ctx, LOCGPU_ERR_INVALID, who + time_refusal(res + 3, 1, "cloud"));  // the count always fits: only a time is refused here
    keep_debug(ctx, c);
    const size_t cnt = (size_t)res[0];
    if (ring_out && rings && cnt) {
        e = hipMemcpyAsync(S->h_ring, S->d_ring, cnt, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) return hip_fail(ctx, e, (who + ": ring bytes").c_str());
        std::memcpy(ring_out, S->h_ring, cnt);
    }
    cl->n = cnt;
    cl->is_dense = 1;  // every survivor is finite
    if (n_out) *n_out = cnt;
    (void)cloud_mark_ready(cl);
    return LOCGPU_OK;
}

}  // namespace

void record_ingest_free(locgpu_ctx* ctx) {
    delete ctx->recingest;
    ctx->recingest = nullptr;
}

}  // namespace locgpu

using namespace locgpu;

extern "C" {

int locgpu_batch_upload_records(locgpu_batch* b, const locgpu_point_layout* layout, const void* const* records, const int64_t* n_points, int32_t* out_counts) {
    return batch_upload_records(b, layout, records, n_points, false, nullptr, nullptr, out_counts, nullptr);
}

int locgpu_batch_upload_records_deskew(locgpu_batch* b, const locgpu_point_layout* layout, const void* const* records, const int64_t* n_points, const double* time_offsets,
                                       const locgpu_sweep_motion* motion, int32_t* out_counts, int32_t* out_status) {
    return batch_upload_records(b, layout, records, n_points, true, time_offsets, motion, out_counts, out_status);
}

int locgpu_cloud_upload_records(locgpu_cloud* c, const locgpu_point_layout* layout, const void* records, int64_t n, uint8_t* ring_out, size_t* n_out) {
    return cloud_upload_records(c, layout, records, n, false, 0.0, nullptr, ring_out, n_out);
}

int locgpu_cloud_upload_records_deskew(locgpu_cloud* c, const locgpu_point_layout* layout, const void* records, int64_t n, double time_offset,
                                       const locgpu_sweep_motion* motion, uint8_t* ring_out, size_t* n_out) {
    return cloud_upload_records(c, layout, records, n, true, time_offset, motion, ring_out, n_out);
}

int locgpu_records_deskew_debug(locgpu_ctx* ctx, int on) {
    if (!ctx) return fail(nullptr, LOCGPU_ERR_INVALID, "records_deskew_debug: NULL context");
    RecordIngestScratch* S = scratch(ctx);
    S->debug = on != 0;
    if (!S->debug) {  // off: nothing is kept
        S->dbg_scans = 0;
        (void)hipSetDevice(ctx->device);
        (void)hipStreamSynchronize(ctx->stream);
        S->d_dbg.reset();
    }
    return LOCGPU_OK;
}

int locgpu_records_deskew_matrices(locgpu_ctx* ctx, int scan, double* out, size_t capacity, size_t* n_out) {
    if (!ctx) return fail(nullptr, LOCGPU_ERR_INVALID, "records_deskew_matrices: NULL context");
    RecordIngestScratch* S = ctx->recingest;
    if (!S || S->dbg_scans == 0) return fail(ctx, LOCGPU_ERR_INVALID, "records_deskew_matrices: no deskewed record ingest has run on this context with locgpu_records_deskew_debug on");
    if (scan < 0 || scan >= S->dbg_scans) return fail(ctx, LOCGPU_ERR_INVALID, "records_deskew_matrices: scan index out of range");
    const size_t cnt = (size_t)S->dbg_counts[scan];
    if (n_out) *n_out = cnt;
    if (!out) return LOCGPU_OK;
    if (capacity < cnt * 12) return fail(ctx, LOCGPU_ERR_INVALID, "records_deskew_matrices: capacity < 12 doubles per survivor");
    if (cnt == 0) return LOCGPU_OK;
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    hipError_t e = hipMemcpyAsync(out, S->d_dbg + (size_t)scan * S->dbg_pitch * 12, cnt * 12 * sizeof(double), hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(ctx, e, "records_deskew_matrices: D2H");
    return LOCGPU_OK;
}

int locgpu_records_ingest_times(locgpu_ctx* ctx, double out_ms[2]) {
    if (!ctx || !out_ms) return fail(ctx, LOCGPU_ERR_INVALID, "records_ingest_times: NULL argument");
    out_ms[0] = ctx->recingest ? ctx->recingest->prof_ms[0] : 0.0;
    out_ms[1] = ctx->recingest ? ctx->recingest->prof_ms[1] : 0.0;
    return LOCGPU_OK;
}

}  // extern "C"
