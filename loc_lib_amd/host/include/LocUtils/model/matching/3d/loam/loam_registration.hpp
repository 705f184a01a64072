// Drop-in for LocUtils/include/LocUtils/model/matching/3d/loam/loam_registration.hpp (:22-60): LoamOption and
// LoamRegistration, the matcher slam_demo selects with `matching_method: 0`. It owns one P2Line matcher for edge points and one
// P2Plane matcher for surface points and runs its own Gauss–Newton loop on the SUM of their normal equations
// (loam_registration.cpp:38-99). Here both evaluations run on the GPU over resident batches; the 6×6 solve stays on the host.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "LocUtils/model/matching/3d/icp/icp_registration.hpp"
#include "LocUtils/model/matching/3d/matching_interface.h"

#include "LocUtils/model/feature_extract/loam_feature_extract.hpp"  // LoamFeatureOptions

struct locgpu_ctx;
struct locgpu_batch;
struct locgpu_loam;

namespace LocUtils {

struct LoamOption {  // reference hpp:22-36
    LoamFeatureOptions feature_option_;
    IcpOptions surf_icp_option_{IcpMethod::P2PLANE};
    IcpOptions edge_icp_option_{IcpMethod::P2LINE};
    int min_edge_pts_{20};
    int min_surf_pts_{20};
    int max_iteration_{20};
    bool use_edge_points_{true};
    bool use_surf_points_{true};
    double eps_{1e-3};
};

class LoamRegistration : public MatchingInterface {
public:
    LoamRegistration();
    explicit LoamRegistration(LoamOption option);
    ~LoamRegistration() override;
    LoamRegistration(const LoamRegistration&) = delete;
    LoamRegistration& operator=(const LoamRegistration&) = delete;

    using MatchingInterface::ScanMatch;
    using MatchingInterface::SetInputTarget;
    bool SetInputTarget(const CloudPtr& edge_input, const CloudPtr& surf_input) override;
    bool ScanMatch(const CloudPtr& edge_input, const CloudPtr& surf_input, const SE3& predict_pose, CloudPtr& result_cloud_ptr,
                   SE3& result_pose) override;
    float GetFitnessScore() override;
    void SetDevice(int device_id);

    // Not in the reference, where GetFitnessScore is a stub that returns 0 (loam_registration.cpp:101-104). After
    // EnableFitnessScore(max_range [m]) GetFitnessScore() returns the JOINT score of the last ScanMatch at its result pose (locgpu.h,
    // locgpu_loam_fitness: the pooled mean squared distance of both classes' inliers, each class against its own map). It is computed
    // on that call, on copies of the two scans ScanMatch was given — kept only after the opt-in — through a handle that borrows this
    // matcher's two contexts (locgpu_loam_create_on), made on first use. ScanMatch's results are what they were. +infinity before
    // the first successful ScanMatch, when no point lies within max_range and when the library fails (LastError). WITHOUT the opt-in
    // GetFitnessScore() keeps returning the reference's 0.0f.
    void EnableFitnessScore(double max_range);
    // Not in the reference: aligns the pair of feature scans from every candidate pose with this matcher's options in one batched
    // call on the GPU (locgpu_loam_init_search: each scan is uploaded once, every candidate runs the device-side joint loop), scores
    // every result (EnableFitnessScore's range, 1 m by default) and hands back the best: the lowest joint score among the results
    // with at least half of their points within range. false — best_score = +infinity, best_pose untouched — when no candidate
    // qualifies, a target is missing, or the library fails (LastError). Leaves what GetFitnessScore() reports alone.
    bool InitialPoseSearch(const CloudPtr& edge_input, const CloudPtr& surf_input, const std::vector<SE3>& candidates, SE3& best_pose, float& best_score);
    // Text of the last failure of the two calls above (the reference only logs through glog).
    const char* LastError() const;

private:
    LoamOption options_;
    locgpu_ctx* edge_ctx_ = nullptr;  // icp_edge_ptr_ (P2Line)
    locgpu_ctx* surf_ctx_ = nullptr;  // icp_surf_ptr_ (P2Plane)
    // one-scan source batches, kept across ScanMatch calls (device buffers of a batch are a dozen hipMalloc/hipFree pairs)
    locgpu_batch* edge_batch_ = nullptr;
    locgpu_batch* surf_batch_ = nullptr;
    size_t edge_cap_ = 0, surf_cap_ = 0;
    int device_id_ = 0;
    bool has_edge_ = false, has_surf_ = false;
    // the score and the search: a handle over edge_ctx_ / surf_ctx_ (borrowed), and what the last ScanMatch left to score
    bool EnsureSearchHandle();
    locgpu_loam* search_ = nullptr;
    bool fitness_enabled_ = false, have_last_pose_ = false;
    double fitness_range_ = 1.0;
    SE3 last_pose_;
    CloudPtr last_edge_, last_surf_;  // deep copies, made only after EnableFitnessScore
    std::string last_error_;
};

}  // namespace LocUtils
