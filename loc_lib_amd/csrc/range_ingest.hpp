// loc_lib_amd/csrc/range_ingest.hpp — sensor-native range images decoded in HBM (range_ingest.hip; include/locgpu.h, "Range-image ingest").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <string>

#include "device_buffer.hpp"

struct locgpu_ctx;
struct locgpu_sweep_motion;

// A sensor model resident in HBM: the four caller-supplied tables in ONE block, copied once by locgpu_sensor_create. The context
// keeps a list of its sensors (locgpu_ctx::sensors) and frees the ones the caller did not destroy.
struct locgpu_sensor {
    locgpu_ctx* ctx = nullptr;
    uint32_t n_rings = 0, n_cols = 0, az_per_ring = 0;
    float range_scale = 0.f, min_range = 0.f;
    locgpu::DevBuf<float> d_tables;  // cos_el[n_rings] | sin_el[n_rings] | cos_az[n_az] | sin_az[n_az], n_az = n_cols or n_rings · n_cols
    // locgpu_sensor_set_col_times: one firing time per column, and the table's extremes for the host-side refusals of a deskewed ingest
    locgpu::DevBuf<double> d_col_time;
    bool has_col_times = false;
    double col_time_min = 0.0, col_time_max = 0.0;
    size_t n_az() const { return az_per_ring ? (size_t)n_rings * n_cols : (size_t)n_cols; }
    size_t cells() const { return (size_t)n_rings * n_cols; }
};

namespace locgpu {

// CloudConver::Conver's two rules on a raw point (cloud_subscriber.cpp:7-29, point_cloud_utils.h:41-44) — the one device copy, shared by
// the range-image decode below and the point-record ingest (record_ingest.hip): true when the point is kept. The distance is compiled
// with contraction off whatever the build's flags are; every product and sum is one IEEE float32 operation rounded to nearest.
__device__ __forceinline__ bool conver_keep(float x, float y, float z, float min_range) {
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
    float d;
    {
#pragma clang fp contract(off)
        const float xx = x * x, yy = y * y, zz = z * z;
        d = sqrtf((xx + yy) + zz);  // PointDistance; sqrtf is correctly rounded (hipcc's default for float32 sqrt and division)
    }
    return !(d < min_range);
}

// Decode of one cell and Conver's two rules — the one copy of the arithmetic, in the order the header states it. Every operation is
// one IEEE float32 operation rounded to nearest: the decode is multiplications only.
// Returns false when the cell yields no point.
__device__ __forceinline__ bool range_decode_cell(uint32_t k, float range_scale, float min_range, float ce, float se, float ca, float sa, float4& p) {
    if (k == 0) return false;  // no return
    const float r = (float)k * range_scale;
    const float h = r * ce;
    const float x = h * ca;
    const float y = h * sa;
    const float z = r * se;
    if (!conver_keep(x, y, z, min_range)) return false;
    p = float4{x, y, z, 0.f};
    return true;
}

constexpr int kRI = 256;  // threads per block of every ingest kernel

// Sum of `x` over the block in every thread's `total`; returns the exclusive prefix of the calling thread. One barrier pair.
__device__ __forceinline__ uint32_t block_exclusive(uint32_t x, uint32_t* s_wave, uint32_t& total) {
    static_assert(kRI == 256, "four waves");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t inc = x;
    for (int off = 1; off < 64; off <<= 1) {
        const uint32_t o = __shfl_up(inc, off, 64);
        if (lane >= off) inc += o;
    }
    __syncthreads();  // s_wave may still be read from the previous use
    if (lane == 63) s_wave[wave] = inc;
    __syncthreads();
    uint32_t before = 0;
    total = 0;
#pragma unroll
    for (int w = 0; w < kRI / 64; ++w) {
        before += w < wave ? s_wave[w] : 0u;
        total += s_wave[w];
    }
    return before + inc - x;
}

// The two middle kernels of an ingest pass, launched for the range-image and the point-record ingest alike (range_ingest.hip).
// tile_cnt [rows][n_scans][n_tiles]: row 0 = survivors per tile, row 1 (rows == 2, the record ingest's deskewed form) = survivors with a
// refused time per tile. offsets: tile_off [n_scans][n_tiles] = exclusive sums of row 0 in tile order, res[s] = scan s's survivors,
// res[n_scans + 2 + s] = its row-1 sum. verdict: res[n_scans] = 1 when every scan fits dst_max_n points and no row-1 sum is positive,
// res[n_scans + 1] = the largest count. res holds rows · n_scans + 2 entries.
void ingest_launch_offsets(hipStream_t s, const uint32_t* tile_cnt, uint32_t n_tiles, uint32_t* tile_off, int32_t* res, int n_scans, int rows);
void ingest_launch_verdict(hipStream_t s, int32_t* res, int n_scans, uint32_t dst_max_n, int rows);

// The refusals of a locgpu_sweep_motion that the host can decide, O(n_scans · K), for the range-image and the point-record ingest:
// LOCGPU_OK, or LOCGPU_ERR_INVALID with the text set. cols: the scan's other query times are known on the host (the sensor's column
// table) and lie in [q_min, q_max]; without it only the reference times are bounded here.
int check_sweep_motion(locgpu_ctx* ctx, const std::string& who, const locgpu_sweep_motion* m, int n_scans, bool cols, double q_min, double q_max);

}  // namespace locgpu
