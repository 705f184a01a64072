// loc_lib_amd/host/src/registration_facade.cpp — the reference's matcher classes as thin hosts of liblocgpu.so.
//
// Behaviour kept from the reference (file:line = reference):
//  * inputs are deep-copied by the library before a call returns (icp_registration.cpp:16,259) — callers may mutate
//    or free their clouds right away (Lio re-filters local_map_ in place, lio.cpp:297);
//  * ScanMatch returns true unconditionally (icp_registration.cpp:243, ndt_registration.cpp:260); on internal failure
//    the pose is the last successful iterate; direct NDT with det(H)==0 leaves result_pose untouched (ndt cpp:435-436);
//  * `use_ann` can only switch approximate search ON, and it is on by default (icp_registration.hpp:76-79 +
//    kdtree.h:128): every reference ICP run uses the alpha=0.1 pruned search, so does this one;
//  * the output cloud is `*result = *source` with x,y,z replaced by the float32 transform (icp cpp:241).
#include <cmath>
#include <cstring>

#include "../../../include/locgpu.h"
#include "LocUtils/model/matching/3d/icp/icp_registration.hpp"
#include "LocUtils/model/matching/3d/loam/loam_registration.hpp"
#include "LocUtils/model/matching/3d/ndt/ndt_registration.hpp"
#include "LocUtils/model/search_point/kdtree/kdtree.h"
#include "LocUtils/model/search_point/bfnn/bfnn.h"

namespace LocUtils {

namespace {
// map_planes: IcpRegistration::EnableMapPlanes — P2PLANE then runs as the labelled fast mode LOCGPU_P2PLANE_MAP
locgpu_icp_opts to_c(const IcpOptions& o, bool map_planes = false) {
    locgpu_icp_opts c;
    locgpu_icp_opts_default(&c);
    c.method = o.method_ == IcpMethod::P2P ? LOCGPU_P2P : (o.method_ == IcpMethod::P2LINE ? LOCGPU_P2LINE : LOCGPU_P2PLANE);
    if (map_planes && o.method_ == IcpMethod::P2PLANE) c.method = LOCGPU_P2PLANE_MAP;
    c.max_iteration = o.max_iteration_;
    c.max_nn_distance = o.max_nn_distance_;
    c.max_plane_distance = o.max_plane_distance_;
    c.max_line_distance = o.max_line_distance_;
    c.min_effective_pts = o.min_effective_pts_;
    c.eps = o.eps_;
    c.approximate = 1;  // see header comment: the reference never disables ANN
    c.ann_alpha = 0.1f;
    return c;
}
bool write_output_cloud(locgpu_ctx* ctx, const CloudPtr& src, const SE3& pose, CloudPtr& out) {
    if (!out) return false;  // the reference would dereference null here (loc.cpp:215 always allocates it)
    *out = *src;             // keeps intensity and the other fields, like pcl::transformPointCloud
    if (src->points.empty()) return true;
    return locgpu_transform_cloud(ctx, pose.data(), src->points.data(), src->points.size(), sizeof(PointType), out->points.data(),
                                  sizeof(PointType)) == LOCGPU_OK;
}
// The output cloud of ScanMatch as locgpu_*_scan_match wants it: a callback the library runs on its helper thread WHILE the alignment
// runs. It sizes the caller's cloud (header fields as `*out = *src` leaves them; the first touch of a fresh 3.7 MB point array happens
// here, off the caller's thread) and hands back the point array; the library copies every point's fields into it there and writes
// x, y, z behind the alignment — one pass over the caller's memory instead of a copy plus a second upload.
struct OutputCloud { const PointCloudType* src; PointCloudType* out; };
void* size_output_cloud(void* user, size_t n) {
    OutputCloud* oc = static_cast<OutputCloud*>(user);
    if (!oc->out) return nullptr;  // the reference would dereference null here (loc.cpp:215 always allocates it)
    if (oc->out != oc->src) {
        oc->out->width = oc->src->width;
        oc->out->height = oc->src->height;
        oc->out->is_dense = oc->src->is_dense;
        oc->out->points = oc->src->points;  // one pass: sized and every field in place (LOCGPU_OUT_FIELDS_DONE); x, y, z follow
    }
    (void)n;
    return oc->out->points.data();
}
}  // namespace

// ------------------------------------------------------------------------------------------------ ICP
IcpRegistration::IcpRegistration() {}
IcpRegistration::IcpRegistration(IcpOptions options) : options_(options) {}
IcpRegistration::~IcpRegistration() { locgpu_destroy(ctx_); }
void IcpRegistration::SetDevice(int device_id) { device_id_ = device_id; }
const char* IcpRegistration::Unsupported() const {
    if (options_.method_ == IcpMethod::PCLICP) return "IcpMethod::PCLICP (pcl::IterativeClosestPoint, icp_registration.cpp:385-399) is not on the GPU path: link PCL's ICP for it";
    if (!options_.use_initial_translation_) return "IcpOptions::use_initial_translation_ = false (icp_registration.cpp:273,311,351: the centroid branch, whose centres the reference never computes) is not on the GPU path";
    return nullptr;
}
const char* IcpRegistration::LastError() const { return Unsupported() ? Unsupported() : locgpu_last_error(ctx_); }
bool IcpRegistration::EnsureContext() { return ctx_ || locgpu_create(device_id_, &ctx_) == LOCGPU_OK; }

bool IcpRegistration::SetInputTarget(const CloudPtr& input_target) {
    if (Unsupported() || !input_target || !EnsureContext()) return false;
    has_target_ = locgpu_icp_set_target(ctx_, input_target->points.data(), input_target->points.size(), sizeof(PointType)) == LOCGPU_OK;
    // the fast mode's plane table is part of the ingest, not of the first ScanMatch (a failure stays in LastError; the matching calls report it)
    if (has_target_ && map_planes_ && options_.method_ == IcpMethod::P2PLANE) (void)locgpu_icp_build_map_planes(ctx_);
    return true;  // the reference returns true whatever happened (icp_registration.cpp:28)
}

bool IcpRegistration::CaculateMatrixHAndB(const CloudPtr& input_source, const SE3& predict_pose, Mat6d& H, Vec6d& B) {
    if (Unsupported() || !has_target_ || !input_source) return false;
    const locgpu_icp_opts o = to_c(options_, map_planes_);
    double h[36], b[6];
    int ok = 0;
    have_last_pose_ = false;  // the evaluation replaces the source copy ScanMatch left in HBM: GetFitnessScore has nothing to score
    if (locgpu_icp_hb(ctx_, input_source->points.data(), input_source->points.size(), sizeof(PointType), predict_pose.data(), &o, h, b, nullptr,
                      &ok) != LOCGPU_OK)
        return false;
    // the reference ACCUMULATES into the caller's H and B (icp cpp:87-88 `H +=`), LoamRegistration passes zeros
    for (int i = 0; i < 36; ++i) H.data()[i] += h[i];  // symmetric: storage order irrelevant
    for (int i = 0; i < 6; ++i) B.data()[i] += b[i];
    return ok != 0;
}

bool IcpRegistration::ScanMatch(const CloudPtr& input_source, const SE3& predict_pose, CloudPtr& result_cloud_ptr, SE3& result_pose) {
    if (Unsupported()) return false;  // a refusal, loudly (LastError): neither result_pose nor the output cloud is touched
    if (!input_source) return true;
    SE3 pose = predict_pose;
    have_last_pose_ = false;
    if (has_target_ && !input_source->points.empty()) {
        // alignment + output cloud in ONE call: the source crosses PCIe once, the transform runs on the copy the alignment left in HBM
        const locgpu_icp_opts o = to_c(options_, map_planes_);
        double out[7];
        OutputCloud oc{input_source.get(), result_cloud_ptr.get()};
        if (locgpu_icp_scan_match(ctx_, input_source->points.data(), input_source->points.size(), sizeof(PointType), predict_pose.data(), &o, out,
                                  nullptr, nullptr, sizeof(PointType) | LOCGPU_OUT_FIELDS_DONE, size_output_cloud, &oc) == LOCGPU_OK) {
            std::memcpy(pose.data(), out, sizeof(out));
            result_pose = pose;
            last_pose_ = pose;  // what a later GetFitnessScore scores (the source stays in HBM until the next call)
            have_last_pose_ = true;
            return true;  // icp_registration.cpp:243
        }
    }
    result_pose = pose;  // no target / empty source / a failed call: the prediction, and the cloud under it
    if (ctx_) write_output_cloud(ctx_, input_source, result_pose, result_cloud_ptr);
    return true;  // icp_registration.cpp:243
}

void IcpRegistration::EnableFitnessScore(double max_range) {
    fitness_enabled_ = true;
    fitness_range_ = max_range;
}

void IcpRegistration::EnableMapPlanes(bool on) { map_planes_ = on; }

float IcpRegistration::GetFitnessScore() {
    if (!fitness_enabled_ || !have_last_pose_) return 0.0f;  // icp_registration.cpp:246-250: the reference's stub
    locgpu_fitness f;
    if (locgpu_icp_fitness_resident(ctx_, last_pose_.data(), fitness_range_, &f) != LOCGPU_OK) return 0.0f;
    return (float)f.score;
}

bool IcpRegistration::InitialPoseSearch(const CloudPtr& source, const std::vector<SE3>& candidates, SE3& best_pose, float& best_score) {
    if (Unsupported() || !has_target_ || !source || source->points.empty() || candidates.empty()) return false;
    const locgpu_icp_opts o = to_c(options_, map_planes_);
    locgpu_init_search_opts so;
    locgpu_init_search_opts_default(&so);
    so.max_range = fitness_range_;
    const size_t m = candidates.size();
    std::vector<double> in(7 * m), out(7 * m);
    for (size_t i = 0; i < m; ++i) std::memcpy(&in[7 * i], candidates[i].data(), 7 * sizeof(double));
    std::vector<locgpu_fitness> fit(m);
    int best = -1;
    if (locgpu_icp_init_search(ctx_, source->points.data(), source->points.size(), sizeof(PointType), in.data(), (int)m, &o, &so, out.data(), fit.data(),
                               nullptr, &best) != LOCGPU_OK || best < 0)
        return false;
    std::memcpy(best_pose.data(), &out[7 * (size_t)best], 7 * sizeof(double));
    best_score = (float)fit[best].score;
    return true;
}

// ------------------------------------------------------------------------------------------------ NDT
NdtRegistration::NdtRegistration() { options_.inv_voxel_size_ = 1.0 / options_.voxel_size_; }
NdtRegistration::NdtRegistration(NdtOptions options) : options_(options) { options_.inv_voxel_size_ = 1.0 / options_.voxel_size_; }
NdtRegistration::~NdtRegistration() { locgpu_destroy(ctx_); }
void NdtRegistration::SetDevice(int device_id) { device_id_ = device_id; }
const char* NdtRegistration::Unsupported() const {
    if (options_.method_ == NdtMethod::PCL_NDT) return "NdtMethod::PCL_NDT (pcl::NormalDistributionsTransform, ndt_registration.cpp:69,246) is not on the GPU path: link PCL's NDT for it";
    if (options_.remove_centroid_) return "NdtOptions::remove_centroid_ = true (ndt_registration.cpp:380-384) is not on the GPU path";
    return nullptr;
}
const char* NdtRegistration::LastError() const { return Unsupported() ? Unsupported() : locgpu_last_error(ctx_); }
bool NdtRegistration::EnsureContext() { return ctx_ || locgpu_create(device_id_, &ctx_) == LOCGPU_OK; }

bool NdtRegistration::SetInputTarget(const CloudPtr& input_target) {
    if (Unsupported()) return false;
    if (!input_target || !EnsureContext()) return true;  // ndt cpp:67-83 always true
    locgpu_ndt_opts o;
    locgpu_ndt_opts_default(&o);
    o.max_iteration = options_.max_iteration_;
    o.voxel_size = options_.voxel_size_;
    o.min_effective_pts = options_.min_effective_pts_;
    o.min_pts_in_voxel = options_.min_pts_in_voxel_;
    o.eps = options_.eps_;
    o.res_outlier_th = options_.res_outlier_th_;
    o.nearby_type = options_.nearby_type_ == NdtNearbyType::CENTER ? 0 : 1;
    o.method = options_.method_ == NdtMethod::INCREMENTAL_NDT ? 2 : 1;
    o.capacity = (int64_t)options_.capacity_;
    has_target_ = locgpu_ndt_set_target(ctx_, input_target->points.data(), input_target->points.size(), sizeof(PointType), &o) == LOCGPU_OK;
    return true;
}

bool NdtRegistration::CaculateMatrixHAndB(const CloudPtr&, const SE3&, Mat6d&, Vec6d&) { return true; }  // empty body in the reference (ndt cpp:43-49)

bool NdtRegistration::ScanMatch(const CloudPtr& input_source, const SE3& predict_pose, CloudPtr& result_cloud_ptr, SE3& result_pose) {
    if (Unsupported()) return false;  // a refusal, loudly (LastError): neither result_pose nor the output cloud is touched
    if (!input_source) return true;
    have_last_pose_ = false;
    if (has_target_ && !input_source->points.empty()) {
        // result_pose is in-out: status 2 (incremental, too few residuals) assigns the current pose (ndt cpp:351); status 1 (det(H) == 0)
        // means AlignNdt returned before assigning it (ndt cpp:435-436) — the library leaves it as the caller had it and transforms the
        // output cloud by that value (:258)
        OutputCloud oc{input_source.get(), result_cloud_ptr.get()};
        locgpu_align_stats st;
        if (locgpu_ndt_scan_match(ctx_, input_source->points.data(), input_source->points.size(), sizeof(PointType), predict_pose.data(),
                                  result_pose.data(), &st, nullptr, sizeof(PointType) | LOCGPU_OUT_FIELDS_DONE, size_output_cloud, &oc) == LOCGPU_OK) {
            last_pose_ = result_pose;  // what a later GetFitnessScore scores (the source stays in HBM until the next call)
            have_last_pose_ = true;
            return true;  // ndt_registration.cpp:260
        }
    }
    if (ctx_) write_output_cloud(ctx_, input_source, result_pose, result_cloud_ptr);
    return true;  // ndt_registration.cpp:260
}

void NdtRegistration::EnableFitnessScore() { fitness_enabled_ = true; }

float NdtRegistration::GetFitnessScore() {
    if (!fitness_enabled_) return 0.0f;  // ndt_registration.cpp:466-471: the reference's stub
    locgpu_fitness f;
    // the incremental method is refused by the library (LOCGPU_ERR_INVALID; its text is LastError())
    if (!have_last_pose_ || locgpu_ndt_fitness_resident(ctx_, last_pose_.data(), &f) != LOCGPU_OK) return INFINITY;
    return (float)f.score;
}

bool NdtRegistration::InitialPoseSearch(const CloudPtr& source, const std::vector<SE3>& candidates, SE3& best_pose, float& best_score) {
    best_score = INFINITY;
    if (Unsupported() || !has_target_ || !source || source->points.empty() || candidates.empty()) return false;
    const size_t m = candidates.size();
    std::vector<double> in(7 * m), out(7 * m);
    for (size_t i = 0; i < m; ++i) std::memcpy(&in[7 * i], candidates[i].data(), 7 * sizeof(double));
    std::vector<locgpu_fitness> fit(m);
    int best = -1;
    // the search runs on the context's shared-source batch: the source copy of the last ScanMatch stays where it is
    if (locgpu_ndt_init_search(ctx_, source->points.data(), source->points.size(), sizeof(PointType), in.data(), (int)m, nullptr, out.data(), fit.data(), nullptr,
                               &best) != LOCGPU_OK || best < 0)
        return false;
    std::memcpy(best_pose.data(), &out[7 * (size_t)best], 7 * sizeof(double));
    best_score = (float)fit[best].score;
    return true;
}

// ------------------------------------------------------------------------------------------------ LOAM
LoamRegistration::LoamRegistration() {}
LoamRegistration::LoamRegistration(LoamOption option) : options_(option) {}
LoamRegistration::~LoamRegistration() {
    locgpu_loam_destroy(search_);  // first: it borrows the two contexts
    locgpu_batch_destroy(edge_batch_);
    locgpu_batch_destroy(surf_batch_);
    locgpu_destroy(edge_ctx_);
    locgpu_destroy(surf_ctx_);
}
void LoamRegistration::SetDevice(int device_id) { device_id_ = device_id; }
const char* LoamRegistration::LastError() const { return last_error_.c_str(); }
void LoamRegistration::EnableFitnessScore(double max_range) {
    fitness_enabled_ = true;
    fitness_range_ = max_range;
}

// The handle of the score and the search: the matcher's own loop options over the two contexts SetInputTarget filled. A class without
// a context yet (no SetInputTarget) cannot be borrowed: that is the missing target.
bool LoamRegistration::EnsureSearchHandle() {
    if (search_) return true;
    if ((options_.use_surf_points_ && !surf_ctx_) || (options_.use_edge_points_ && !edge_ctx_)) { last_error_ = "LoamRegistration: SetInputTarget has not been called"; return false; }
    locgpu_loam_opts o;
    locgpu_loam_opts_default(&o);
    o.surf = to_c(options_.surf_icp_option_);
    o.edge = to_c(options_.edge_icp_option_);
    o.use_surf_points = options_.use_surf_points_;
    o.use_edge_points = options_.use_edge_points_;
    o.max_iteration = options_.max_iteration_;
    o.eps = options_.eps_;
    if (locgpu_loam_create_on(options_.use_surf_points_ ? surf_ctx_ : nullptr, options_.use_edge_points_ ? edge_ctx_ : nullptr, &o, &search_) != LOCGPU_OK) {
        last_error_ = locgpu_loam_last_error(nullptr);
        return false;
    }
    return true;
}

float LoamRegistration::GetFitnessScore() {
    if (!fitness_enabled_) return 0.0f;  // loam_registration.cpp:101-104: the reference's stub
    if (!have_last_pose_) { last_error_ = "LoamRegistration::GetFitnessScore: no ScanMatch has succeeded yet"; return INFINITY; }
    if (!EnsureSearchHandle()) return INFINITY;
    locgpu_fitness f[3];
    const bool e = options_.use_edge_points_ && last_edge_, s = options_.use_surf_points_ && last_surf_;
    if (locgpu_loam_fitness(search_, e ? last_edge_->points.data() : nullptr, e ? last_edge_->points.size() : 0, s ? last_surf_->points.data() : nullptr,
                            s ? last_surf_->points.size() : 0, sizeof(PointType), last_pose_.data(), 1, fitness_range_, f) != LOCGPU_OK) {
        last_error_ = locgpu_loam_last_error(search_);
        return INFINITY;
    }
    return (float)f[0].score;
}

bool LoamRegistration::InitialPoseSearch(const CloudPtr& edge_input, const CloudPtr& surf_input, const std::vector<SE3>& candidates, SE3& best_pose,
                                         float& best_score) {
    best_score = INFINITY;
    if (candidates.empty()) { last_error_ = "LoamRegistration::InitialPoseSearch: no candidates"; return false; }
    if (!EnsureSearchHandle()) return false;
    locgpu_init_search_opts so;
    locgpu_init_search_opts_default(&so);
    so.max_range = fitness_range_;
    const size_t m = candidates.size();
    std::vector<double> in(7 * m), out(7 * m);
    for (size_t i = 0; i < m; ++i) std::memcpy(&in[7 * i], candidates[i].data(), 7 * sizeof(double));
    std::vector<locgpu_fitness> fit(3 * m);
    int best = -1;
    const bool e = options_.use_edge_points_ && edge_input, s = options_.use_surf_points_ && surf_input;
    if (locgpu_loam_init_search(search_, e ? edge_input->points.data() : nullptr, e ? edge_input->points.size() : 0, s ? surf_input->points.data() : nullptr,
                                s ? surf_input->points.size() : 0, sizeof(PointType), in.data(), (int)m, &so, out.data(), fit.data(), nullptr, &best) != LOCGPU_OK) {
        last_error_ = locgpu_loam_last_error(search_);
        return false;
    }
    if (best < 0) { last_error_ = "LoamRegistration::InitialPoseSearch: no candidate qualifies"; return false; }
    std::memcpy(best_pose.data(), &out[7 * (size_t)best], 7 * sizeof(double));
    best_score = (float)fit[3 * (size_t)best].score;
    return true;
}

bool LoamRegistration::SetInputTarget(const CloudPtr& edge_input, const CloudPtr& surf_input) {
    if (options_.use_edge_points_ && edge_input && (edge_ctx_ || locgpu_create(device_id_, &edge_ctx_) == LOCGPU_OK))
        has_edge_ = locgpu_icp_set_target(edge_ctx_, edge_input->points.data(), edge_input->points.size(), sizeof(PointType)) == LOCGPU_OK;
    if (options_.use_surf_points_ && surf_input && (surf_ctx_ || locgpu_create(device_id_, &surf_ctx_) == LOCGPU_OK))
        has_surf_ = locgpu_icp_set_target(surf_ctx_, surf_input->points.data(), surf_input->points.size(), sizeof(PointType)) == LOCGPU_OK;
    return true;  // loam_registration.cpp:35
}

bool LoamRegistration::ScanMatch(const CloudPtr& edge_input, const CloudPtr& surf_input, const SE3& predict_pose, CloudPtr& result_cloud_ptr,
                                 SE3& result_pose) {
    // Sources stay resident for the whole loop; each iteration = one H/B evaluation per feature class (loam_registration.cpp:53-71),
    // the sum H = H_edge + H_surf, B = B_edge + B_surf (:76-77), dx = H⁻¹·B with NO effective-count or determinant test (:79),
    // update, stop at |dx| < eps_ (:85). A failed sub-evaluation aborts with `return false` before result_pose is written (:56-70).
    struct Side { locgpu_ctx* ctx; locgpu_batch** batch; size_t* cap; locgpu_icp_opts opts; bool use; };
    Side sides[2] = {{surf_ctx_, &surf_batch_, &surf_cap_, to_c(options_.surf_icp_option_), options_.use_surf_points_},
                     {edge_ctx_, &edge_batch_, &edge_cap_, to_c(options_.edge_icp_option_), options_.use_edge_points_}};
    const CloudPtr* inputs[2] = {&surf_input, &edge_input};
    const bool have[2] = {has_surf_, has_edge_};
    bool ok = true;
    have_last_pose_ = false;
    for (int i = 0; i < 2 && ok; ++i) {
        if (!sides[i].use) continue;
        if (!have[i] || !*inputs[i] || (*inputs[i])->points.empty()) { ok = false; break; }
        const void* src[1] = {(*inputs[i])->points.data()};
        const size_t cnt[1] = {(*inputs[i])->points.size()};
        // the batch of the previous call is reused (deep copy of the new source into its buffers); it only grows
        if (!*sides[i].batch || *sides[i].cap < cnt[0]) {
            locgpu_batch_destroy(*sides[i].batch);
            *sides[i].batch = nullptr;
            *sides[i].cap = cnt[0] + cnt[0] / 4 + 1024;
            ok = locgpu_batch_create_empty(sides[i].ctx, 1, *sides[i].cap, sides[i].batch) == LOCGPU_OK;
        }
        ok = ok && locgpu_batch_upload_async(*sides[i].batch, src, cnt, sizeof(PointType)) == LOCGPU_OK &&
             locgpu_batch_upload_wait(*sides[i].batch) == LOCGPU_OK;
    }
    SE3 pose = predict_pose;
    for (int iter = 0; ok && iter < options_.max_iteration_; ++iter) {
        double sum[44] = {0};
        for (int i = 0; i < 2 && ok; ++i) {
            if (!sides[i].use) continue;
            double hb[44];
            ok = locgpu_icp_hb_batch(sides[i].ctx, *sides[i].batch, pose.data(), &sides[i].opts, hb) == LOCGPU_OK && hb[43] != 0.0;
            for (int k = 0; k < 42; ++k) sum[k] += hb[k];
        }
        if (!ok) break;
        sum[42] = 1e18;  // no effective-count gate in the LOAM loop
        double dx[6];
        int applied = 0, stop = 0;
        locgpu_gn_update(sum, LOCGPU_P2PLANE, 0, options_.eps_, pose.data(), dx, &applied, &stop);
        if (stop) break;
    }
    if (!ok) return false;
    result_pose = pose;
    if (fitness_enabled_) {  // what a later GetFitnessScore scores: nothing of this is kept without the opt-in
        last_edge_.reset(edge_input ? new PointCloudType(*edge_input) : nullptr);
        last_surf_.reset(surf_input ? new PointCloudType(*surf_input) : nullptr);
        last_pose_ = pose;
        have_last_pose_ = true;
    }
    // *cloud += *edge; *cloud += *surf; transformPointCloud (loam_registration.cpp:93-96)
    CloudPtr cloud(new PointCloudType);
    if (edge_input) cloud->points.insert(cloud->points.end(), edge_input->points.begin(), edge_input->points.end());
    if (surf_input) cloud->points.insert(cloud->points.end(), surf_input->points.begin(), surf_input->points.end());
    locgpu_ctx* any = surf_ctx_ ? surf_ctx_ : edge_ctx_;
    if (any) write_output_cloud(any, cloud, result_pose, result_cloud_ptr);
    return true;
}

// ------------------------------------------------------------------------------------------------ search plug-in
KdtreeRegistration::KdtreeRegistration(bool) {}
KdtreeRegistration::~KdtreeRegistration() { locgpu_destroy(ctx_); }

bool KdtreeRegistration::SetTargetCloud(const CloudPtr& cloud) {
    if (!cloud || cloud->points.empty()) return false;  // kdtree.cpp:263-266
    if (!ctx_ && locgpu_create(0, &ctx_) != LOCGPU_OK) return false;
    return locgpu_icp_set_target(ctx_, cloud->points.data(), cloud->points.size(), sizeof(PointType)) == LOCGPU_OK;
}

bool KdtreeRegistration::FindNearstPointsBatch(const float* xyz, size_t n, int k, std::vector<int>& out) {
    out.assign(n * (size_t)k, -1);
    return ctx_ && locgpu_knn(ctx_, xyz, n, k, approximate_ ? 1 : 0, alpha_, LOCGPU_SEARCH_TREE_FAITHFUL, out.data(), nullptr) == LOCGPU_OK;
}

std::vector<int> KdtreeRegistration::FindNearstPoints(const Vec3f& point, int k) {
    const float q[3] = {point[0], point[1], point[2]};
    std::vector<int> out;
    if (!FindNearstPointsBatch(q, 1, k, out)) out.clear();  // k > size_: empty result (kdtree.cpp:149-153)
    return out;
}

void KdtreeRegistration::FindCloud(const CloudPtr&, std::vector<std::pair<size_t, size_t>>&) {}
void KdtreeRegistration::SetEnableANN(bool use_ann, float alpha) { approximate_ = use_ann; alpha_ = alpha; }

// ------------------------------------------------------------------------------------------------ BfnnRegistration (bfnn.cpp:7-50)
BfnnRegistration::BfnnRegistration(bool) {}
BfnnRegistration::~BfnnRegistration() { locgpu_destroy(ctx_); }

bool BfnnRegistration::SetTargetCloud(const CloudPtr& cloud) {
    if (!cloud || cloud->points.empty()) return false;  // bfnn.cpp:16-19
    if (!ctx_ && locgpu_create(0, &ctx_) != LOCGPU_OK) return false;
    return locgpu_bfnn_set_target(ctx_, cloud->points.data(), cloud->points.size(), sizeof(PointType)) == LOCGPU_OK;
}

bool BfnnRegistration::FindNearstPointsBatch(const float* xyz, size_t n, int k, std::vector<int>& out) {
    out.assign(n * (size_t)k, -1);
    return ctx_ && locgpu_bfnn_knn(ctx_, xyz, n, k, out.data()) == LOCGPU_OK;
}

std::vector<int> BfnnRegistration::FindNearstPoints(const Vec3f& point, int k) {
    const float q[3] = {point[0], point[1], point[2]};
    std::vector<int> out;
    if (!FindNearstPointsBatch(q, 1, k, out)) out.clear();
    return out;
}

void BfnnRegistration::FindCloud(const CloudPtr&, std::vector<std::pair<size_t, size_t>>&) {}

}  // namespace LocUtils
