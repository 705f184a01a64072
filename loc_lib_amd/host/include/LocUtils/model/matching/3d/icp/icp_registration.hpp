// Drop-in for LocUtils/include/LocUtils/model/matching/3d/icp/icp_registration.hpp: same enum, option struct
// (field for field, same defaults — slam_demo only overwrites some of them, lio_matching_flow.cpp:32-38), constructors
// and virtuals. The work happens in liblocgpu.so (include/locgpu.h); nothing is computed on the CPU here.
// IcpMethod::PCLICP (a pass-through to pcl::IterativeClosestPoint in the reference, :385-399) is not on the
// accelerated path: constructing with it is accepted, matching calls report failure through the bool.
#pragma once
#include <memory>
#include <vector>

#include "LocUtils/model/matching/3d/matching_interface.h"

struct locgpu_ctx;

namespace LocUtils {

enum class IcpMethod { P2P, P2LINE, P2PLANE, PCLICP };  // reference hpp:15-20

struct IcpOptions {  // reference hpp:22-39
    IcpOptions() {}
    IcpOptions(IcpMethod method) { method_ = method; }
    int max_iteration_ = 20;
    double max_nn_distance_ = 1.0;
    double max_plane_distance_ = 0.1;
    double max_line_distance_ = 0.5;
    int min_effective_pts_ = 10;
    double eps_ = 1e-2;
    double euc_fitness_eps_ = 0.36;
    bool use_initial_translation_ = true;
    bool use_ann{false};
    IcpMethod method_{IcpMethod::P2P};
};

class IcpRegistration : public MatchingInterface {
public:
    IcpRegistration();
    explicit IcpRegistration(IcpOptions options);
    ~IcpRegistration() override;
    IcpRegistration(const IcpRegistration&) = delete;
    IcpRegistration& operator=(const IcpRegistration&) = delete;

    bool SetInputTarget(const CloudPtr& input_target) override;
    bool CaculateMatrixHAndB(const CloudPtr& input_source, const SE3& predict_pose, Mat6d& H, Vec6d& B) override;
    bool ScanMatch(const CloudPtr& input_source, const SE3& predict_pose, CloudPtr& result_cloud_ptr, SE3& result_pose) override;
    float GetFitnessScore() override;

    // Not in the reference, where GetFitnessScore is a stub that returns 0 (icp_registration.cpp:246-250). After
    // EnableFitnessScore(max_range [m]) GetFitnessScore() returns the score of the last ScanMatch as pcl::Registration::getFitnessScore
    // defines it (locgpu.h, locgpu_icp_fitness): it is computed on that call, from the source copy ScanMatch left in HBM and the
    // result pose — ScanMatch itself does nothing more than before. +inf when no point lies within max_range; 0 before the first
    // ScanMatch or when the library fails (LastError). WITHOUT the opt-in GetFitnessScore() keeps returning the reference's 0.0f.
    // NdtRegistration and LoamRegistration have opt-ins of their own (their headers): an NDT context has no nearest-neighbour
    // structure to score against, and a LOAM alignment has two.
    void EnableFitnessScore(double max_range);
    // Not in the reference: a labelled FAST MODE, never the source of a parity claim. With it on and method_ == P2PLANE the matcher
    // fits ONE plane per map point when the target is set (SetInputTarget builds the table; locgpu_icp_build_map_planes) and every
    // iteration is plain point-to-plane against the plane of the nearest map point (LOCGPU_P2PLANE_MAP) instead of the reference's
    // math::FitPlane per source point and iteration (math_utils.h:112-136, icp_registration.cpp:161-213). ScanMatch,
    // CaculateMatrixHAndB and InitialPoseSearch follow the switch; GetFitnessScore scores whatever ScanMatch ran. Other methods and
    // the switch left off: nothing changes. Call it before SetInputTarget (later is allowed: the first matching call builds the table).
    void EnableMapPlanes(bool on);
    // Not in the reference: aligns `source` from every candidate pose with this matcher's options in one batched call on the GPU
    // (locgpu_icp_init_search: the cloud is uploaded once), scores every result (EnableFitnessScore's range, 1 m by default) and hands
    // back the best: the lowest score among the results with at least half of their points within range. false — and best_pose /
    // best_score untouched — when no candidate qualifies, there is no target, or the library fails (LastError).
    bool InitialPoseSearch(const CloudPtr& source, const std::vector<SE3>& candidates, SE3& best_pose, float& best_score);

    // Which GPU the matcher lives on (default 0). Not in the reference; must be called before SetInputTarget.
    void SetDevice(int device_id);
    // Text of the last liblocgpu error (the reference only logs through glog) — or, when the options name a branch of the reference
    // that is not on the GPU path (IcpMethod::PCLICP, icp_registration.cpp:385-399; use_initial_translation_ = false, :273,311,351),
    // the refusal: SetInputTarget, CaculateMatrixHAndB and ScanMatch then return false and touch nothing, instead of quietly running
    // something else.
    const char* LastError() const;

private:
    bool EnsureContext();
    const char* Unsupported() const;  // nullptr when the options are on the GPU path
    IcpOptions options_;
    locgpu_ctx* ctx_ = nullptr;
    int device_id_ = 0;
    bool has_target_ = false;
    bool fitness_enabled_ = false, have_last_pose_ = false;  // have_last_pose_: the last ScanMatch left its source in HBM
    bool map_planes_ = false;
    double fitness_range_ = 1.0;
    SE3 last_pose_;
};

}  // namespace LocUtils
