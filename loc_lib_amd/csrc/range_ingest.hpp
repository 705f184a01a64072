// loc_lib_amd/csrc/range_ingest.hpp — sensor-native range images decoded in HBM (range_ingest.hip; include/locgpu.h, "Range-image ingest").
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "device_buffer.hpp"

struct locgpu_ctx;

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

// Decode of one cell and CloudConver::Conver's two rules (cloud_subscriber.cpp:7-29, point_cloud_utils.h:41-44) — the one copy of the
// arithmetic, in the order the header states it. Every operation is one IEEE float32 operation rounded to nearest: the decode is
// multiplications only, and the distance is compiled with contraction off whatever the build's flags are.
// Returns false when the cell yields no point.
__device__ __forceinline__ bool range_decode_cell(uint32_t k, float range_scale, float min_range, float ce, float se, float ca, float sa, float4& p) {
    if (k == 0) return false;  // no return
    const float r = (float)k * range_scale;
    const float h = r * ce;
    const float x = h * ca;
    const float y = h * sa;
    const float z = r * se;
    if (!(isfinite(x) && isfinite(y) && isfinite(z))) return false;
    float d;
    {
#pragma clang fp contract(off)
        const float xx = x * x, yy = y * y, zz = z * z;
        d = sqrtf((xx + yy) + zz);  // PointDistance; sqrtf is correctly rounded (hipcc's default for float32 sqrt and division)
    }
    if (d < min_range) return false;
    p = float4{x, y, z, 0.f};
    return true;
}

}  // namespace locgpu
