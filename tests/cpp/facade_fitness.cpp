// tests/cpp/facade_fitness.cpp — the fitness score and the initial-pose search through the C++ façade (tests/test_gpu_init_search.py):
//   * GetFitnessScore() is the reference's 0.0f without EnableFitnessScore (icp_registration.cpp:246-250) and the score of the last
//     ScanMatch after it — the very bits locgpu_icp_fitness gives for the same cloud and pose;
//   * ScanMatch's pose and output cloud are byte-identical with and without the opt-in;
//   * InitialPoseSearch returns what locgpu_icp_init_search returns.
// Usage: facade_fitness <method 0..2> <map.bin> <scan.bin> <pose7.bin> <candidates.bin> <out.bin>
// Cloud files: raw float32 [n][3]; candidates.bin: m × 7 doubles. out.bin (doubles): pose 7, façade score, ABI score, inliers, finite
// points, best pose 7, best score, best index.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/locgpu.h"
#include "LocUtils/model/matching/3d/icp/icp_registration.hpp"

using namespace LocUtils;

static std::vector<char> slurp(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    std::vector<char> raw((size_t)std::ftell(f));
    std::fseek(f, 0, SEEK_SET);
    if (std::fread(raw.data(), 1, raw.size(), f) != raw.size()) std::exit(2);
    std::fclose(f);
    return raw;
}

static CloudPtr load(const char* path) {
    const std::vector<char> raw = slurp(path);
    const float* v = reinterpret_cast<const float*>(raw.data());
    CloudPtr c(new PointCloudType);
    c->points.resize(raw.size() / 12);
    for (size_t i = 0; i < c->points.size(); ++i) {
        c->points[i].x = v[3 * i]; c->points[i].y = v[3 * i + 1]; c->points[i].z = v[3 * i + 2];
        c->points[i].intensity = (float)i;
    }
    return c;
}

int main(int argc, char** argv) {
    if (argc != 7) { std::fprintf(stderr, "usage\n"); return 2; }
    const int method = std::atoi(argv[1]);
    CloudPtr map = load(argv[2]), scan = load(argv[3]);
    SE3 predict;
    { const std::vector<char> raw = slurp(argv[4]); if (raw.size() != 56) return 2; std::memcpy(predict.data(), raw.data(), 56); }
    const std::vector<char> cand_raw = slurp(argv[5]);
    const size_t m = cand_raw.size() / 56;
    std::vector<SE3> cands(m);
    for (size_t i = 0; i < m; ++i) std::memcpy(cands[i].data(), cand_raw.data() + 56 * i, 56);
    const double max_range = 1.0;
    IcpOptions o(method == 0 ? IcpMethod::P2P : (method == 1 ? IcpMethod::P2LINE : IcpMethod::P2PLANE));

    // without the opt-in: the drop-in behaviour
    IcpRegistration plain(o);
    plain.SetInputTarget(map);
    if (plain.GetFitnessScore() != 0.0f) return 10;
    CloudPtr out_plain(new PointCloudType);
    SE3 res_plain;
    if (!plain.ScanMatch(scan, predict, out_plain, res_plain)) return 3;
    if (plain.GetFitnessScore() != 0.0f) return 11;

    // with it
    IcpRegistration scored(o);
    scored.EnableFitnessScore(max_range);
    scored.SetInputTarget(map);
    if (scored.GetFitnessScore() != 0.0f) return 12;  // nothing matched yet
    CloudPtr out_scored(new PointCloudType);
    SE3 res_scored;
    if (!scored.ScanMatch(scan, predict, out_scored, res_scored)) return 3;
    const float score = scored.GetFitnessScore();
    if (std::memcmp(res_plain.data(), res_scored.data(), 56) != 0) return 13;
    if (out_plain->points.size() != out_scored->points.size() ||
        std::memcmp(out_plain->points.data(), out_scored->points.data(), out_plain->points.size() * sizeof(PointType)) != 0)
        return 14;
    const float again = scored.GetFitnessScore();
    if (std::memcmp(&score, &again, 4) != 0) return 15;

    // the C ABI on the same cloud and pose
    locgpu_ctx* ctx = nullptr;
    if (locgpu_create(0, &ctx) != LOCGPU_OK) return 5;
    if (locgpu_icp_set_target(ctx, map->points.data(), map->points.size(), sizeof(PointType)) != LOCGPU_OK) return 5;
    locgpu_fitness f;
    if (locgpu_icp_fitness(ctx, scan->points.data(), scan->points.size(), sizeof(PointType), res_scored.data(), 1, max_range, &f) != LOCGPU_OK) return 6;
    const float abi_score = (float)f.score;
    if (std::memcmp(&score, &abi_score, 4) != 0) return 16;

    // InitialPoseSearch against locgpu_icp_init_search with the options the façade derives from IcpOptions
    SE3 best_pose;
    float best_score = -1.0f;
    const bool found = scored.InitialPoseSearch(scan, cands, best_pose, best_score);
    locgpu_icp_opts co;
    locgpu_icp_opts_default(&co);
    co.method = method;
    locgpu_init_search_opts so;
    locgpu_init_search_opts_default(&so);
    so.max_range = max_range;
    std::vector<double> poses(7 * m);
    std::vector<locgpu_fitness> fit(m);
    int best = -1;
    if (locgpu_icp_init_search(ctx, scan->points.data(), scan->points.size(), sizeof(PointType), reinterpret_cast<const double*>(cand_raw.data()), (int)m, &co, &so,
                               poses.data(), fit.data(), nullptr, &best) != LOCGPU_OK)
        return 7;
    if (found != (best >= 0)) return 17;
    if (found) {
        if (std::memcmp(best_pose.data(), &poses[7 * (size_t)best], 56) != 0) return 18;
        const float want = (float)fit[best].score;
        if (std::memcmp(&best_score, &want, 4) != 0) return 19;
    }
    { const float after = scored.GetFitnessScore(); if (std::memcmp(&score, &after, 4) != 0) return 20; }  // still the last ScanMatch's
    locgpu_destroy(ctx);

    FILE* fo = std::fopen(argv[6], "wb");
    if (!fo) return 2;
    std::fwrite(res_scored.data(), 8, 7, fo);
    const double tail[4] = {(double)score, f.score, (double)f.inliers, (double)f.finite_points};
    std::fwrite(tail, 8, 4, fo);
    std::fwrite(best_pose.data(), 8, 7, fo);
    const double tail2[2] = {(double)best_score, (double)best};
    std::fwrite(tail2, 8, 2, fo);
    std::fclose(fo);
    return 0;
}
