// loc_lib_amd/csrc/cloud_filters.hpp — device-resident clouds and the filters either side of the matcher.
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "device_buffer.hpp"
#include "device_math.hpp"

struct locgpu_ctx;
struct locgpu_batch;

// A cloud resident in HBM: one float4 {x, y, z, intensity} per point. `is_dense` is pcl::PointCloud::is_dense — the
// PCL filters trust it (a dense cloud is never tested for NaN), so it travels with the data.
struct locgpu_cloud {
    locgpu_ctx* ctx = nullptr;
    locgpu::DevBuf<float4> d;
    size_t n = 0;
    int is_dense = 1;
    locgpu::Event ready;  // recorded on the owner's stream behind the last call that wrote the cloud (cloud_mark_ready): what ANOTHER context waits for
};

namespace locgpu {

// Written by the setup kernel, read back by the host once per voxel filter.
struct VoxelParams {
    int32_t min_b[3], div_b[3], mul[3];
    uint32_t invalid_key;             // key given to non-finite points of a non-dense cloud (= number of cells)
    int32_t status;                   // 0 ok, 1 leaf too small (pass-through), 2 no finite point
    uint32_t n_out;                   // number of output points of the last filter
    float inv_leaf;
};

struct FilterScratch {
    size_t cap = 0;  // points the group {keys, vals, head, rank, temp} has room for
    DevBuf<uint32_t> keys[2], vals[2], head, rank;
    DevBuf<unsigned char> temp;  // scratch of the device-wide primitives at `cap` points
    DevBuf<VoxelParams> d_params;
    PinnedBuf<VoxelParams> h_params;
    DevBuf<float> d_partial;     // per-block bounding boxes of the min/max pass
    DevBuf<float4> d_tmp;        // staging for in-place filters
    PinnedBuf<float4> h_stage;   // pinned host staging for upload/download
    Event stage_ev;              // recorded behind an upload's H2D: the staging buffer is free again once it has fired
    bool stage_busy = false;
};

// A cloud as a READ-ONLY input of context `ctx` (matcher source, keyframe, target): its own context's clouds need nothing (one
// stream); a cloud of ANOTHER context on the same GPU is accepted too — a front-end that uploads and filters scan i+1 on one
// context while another matches scan i — and `ctx`'s stream is then ordered behind everything the owning context has enqueued so
// far. The caller must not let the owner modify the cloud while it is in use here. Returns hipErrorInvalidValue for another device.
hipError_t cloud_input_ready(locgpu_ctx* ctx, const locgpu_cloud* c);
// Called by the owner's entry points behind every call that wrote `c`: records c->ready on the owner's stream.
hipError_t cloud_mark_ready(locgpu_cloud* c);
void filters_free(locgpu_ctx* ctx);
void batch_filters_free(locgpu_ctx* ctx);  // batch_filters.hip: the batch front-end's workspaces (called by filters_free)
void merge_free(locgpu_ctx* ctx);          // cloud_merge.hip: the global-map pass's workspaces (called by filters_free)
void range_ingest_free(locgpu_ctx* ctx);   // range_ingest.hip: the ingest's workspaces and the context's remaining sensors (called by locgpu_destroy)
void record_ingest_free(locgpu_ctx* ctx);  // record_ingest.hip: the point-record ingest's staging and workspaces (called by locgpu_destroy)
void resident_deskew_free(locgpu_ctx* ctx);  // resident_deskew.hip: locgpu_batch_deskew's motion staging and workspaces (called by locgpu_destroy)
// batch_filters.hip, for every pass over a batch's points on its context's stream (batch_loam.hip too). order_behind_batch: the stream
// goes behind everything that may still touch b's points — its pending upload (the host side is waited for) and the idle launches a
// paced one-scan alignment may have left queued; returns a locgpu_status. set_host_counts: the batch's three copies of its counts
// agree again after d_counts was written on the device.
int order_behind_batch(locgpu_ctx* ctx, locgpu_batch* b, const char* who);
void set_host_counts(locgpu_batch* b, const int* counts);
hipError_t cloud_reserve(locgpu_cloud* c, size_t n, bool keep);
hipError_t cloud_stage(locgpu_ctx* ctx, size_t n, float4** out);
hipError_t cloud_stage_release(locgpu_ctx* ctx);  // pinned staging of at least n points

// All run on ctx->stream and return after the result size is known (one small D2H + sync each).
// `out` may alias `in`'s owner (in-place): results are produced in scratch and swapped in.
hipError_t voxel_filter_dev(locgpu_ctx* ctx, const locgpu_cloud* in, float leaf, locgpu_cloud* out, int* status);
hipError_t crop_box_dev(locgpu_ctx* ctx, const locgpu_cloud* in, const float mn[3], const float mx[3], locgpu_cloud* out);
hipError_t remove_nan_dev(locgpu_ctx* ctx, const locgpu_cloud* in, locgpu_cloud* out);
hipError_t transform_dev(locgpu_ctx* ctx, const locgpu_cloud* in, const double pose[7], locgpu_cloud* out);
hipError_t append_dev(locgpu_ctx* ctx, locgpu_cloud* dst, const locgpu_cloud* src);

// pcl::transformPointCloud with a DOUBLE 4x4 (lio.cpp:244,279,571), the one copy of its arithmetic: transform_cloud_f64_kernel
// (cloud_filters.hip) and merge_kernel (cloud_merge.hip) both call it. Per row (float)(((m0·x + m1·y) + m2·z) + m3) in double — PCL 1.8's
// templated overload, left to right; a non-finite point of a cloud that is not flagged dense is left as it is; the w lane is carried.
struct M34 { double v[12]; };  // row-major 3×4
__device__ __forceinline__ float4 transform_point_f64(const float4& p, const double* __restrict__ m, bool dense) {
    float4 o = p;
    if (dense || (isfinite(p.x) && isfinite(p.y) && isfinite(p.z))) {
        const double x = p.x, y = p.y, z = p.z;
        o.x = (float)(((m[0] * x + m[1] * y) + m[2] * z) + m[3]);
        o.y = (float)(((m[4] * x + m[5] * y) + m[6] * z) + m[7]);
        o.z = (float)(((m[8] * x + m[9] * y) + m[10] * z) + m[11]);
    }
    return o;
}
// pose.matrix() of a 7-double pose (quaternion xyzw + translation): Eigen's toRotationMatrix (quat_to_R) beside the translation.
inline void pose_to_m34(const double pose[7], M34& m) {
    double R[9];
    quat_to_R(pose, R);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) m.v[4 * r + c] = R[3 * r + c];
        m.v[4 * r + 3] = pose[4 + r];
    }
}

// loam_features.hip
void loam_free(locgpu_ctx* ctx);
void batch_loam_free(locgpu_ctx* ctx);  // batch_loam.hip: the batched picker's workspaces (called by loam_free)
hipError_t loam_extract_dev(locgpu_ctx* ctx, const locgpu_cloud* in, const unsigned char* ring, int num_scan, locgpu_cloud* edge, locgpu_cloud* surf,
                            bool* too_long);

}  // namespace locgpu
