// tests/cpp/facade_ndt_fitness.cpp — the NDT fitness score and initial-pose search through the C++ façade (tests/test_gpu_ndt_init_search.py):
//   * GetFitnessScore() is the reference's 0.0f without EnableFitnessScore (ndt_registration.cpp:466-471); after it, +infinity before
//     any ScanMatch and then the score of the last ScanMatch — the very bits locgpu_ndt_fitness gives for the same cloud and pose;
//   * ScanMatch's pose and output cloud are byte-identical with and without the opt-in;
//   * InitialPoseSearch returns what locgpu_ndt_init_search returns;
//   * NdtMethod::INCREMENTAL_NDT: the score is +infinity, the search returns false, and LastError says why.
// Usage: facade_ndt_fitness <map.bin> <scan.bin> <pose7.bin> <candidates.bin> <out.bin>
// Cloud files: raw float32 [n][3]; candidates.bin: m × 7 doubles. out.bin (doubles): pose 7, façade score, ABI score, inliers, finite
// points, best pose 7, best score, best index.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/locgpu.h"
#include "LocUtils/model/matching/3d/ndt/ndt_registration.hpp"

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
    if (argc != 6) { std::fprintf(stderr, "usage\n"); return 2; }
    CloudPtr map = load(argv[1]), scan = load(argv[2]);
    SE3 predict;
    { const std::vector<char> raw = slurp(argv[3]); if (raw.size() != 56) return 2; std::memcpy(predict.data(), raw.data(), 56); }
    const std::vector<char> cand_raw = slurp(argv[4]);
    const size_t m = cand_raw.size() / 56;
    std::vector<SE3> cands(m);
    for (size_t i = 0; i < m; ++i) std::memcpy(cands[i].data(), cand_raw.data() + 56 * i, 56);
    NdtOptions o;  // the reference's defaults: DIRECT_NDT, NEARBY6, voxel 1.0

    // without the opt-in: the drop-in behaviour
    NdtRegistration plain(o);
    plain.SetInputTarget(map);
    if (plain.GetFitnessScore() != 0.0f) return 10;
    CloudPtr out_plain(new PointCloudType);
    SE3 res_plain = predict;
    if (!plain.ScanMatch(scan, predict, out_plain, res_plain)) return 3;
    if (plain.GetFitnessScore() != 0.0f) return 11;

    // with it
    NdtRegistration scored(o);
    scored.EnableFitnessScore();
    scored.SetInputTarget(map);
    { const float before = scored.GetFitnessScore(); if (!(std::isinf(before) && before > 0)) return 12; }  // nothing matched yet
    CloudPtr out_scored(new PointCloudType);
    SE3 res_scored = predict;
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
    if (locgpu_ndt_set_target(ctx, map->points.data(), map->points.size(), sizeof(PointType), nullptr) != LOCGPU_OK) return 5;
    locgpu_fitness f;
    if (locgpu_ndt_fitness(ctx, scan->points.data(), scan->points.size(), sizeof(PointType), res_scored.data(), 1, &f) != LOCGPU_OK) return 6;
    const float abi_score = (float)f.score;
    if (std::memcmp(&score, &abi_score, 4) != 0) return 16;

    // InitialPoseSearch against locgpu_ndt_init_search
    SE3 best_pose;
    float best_score = -1.0f;
    const bool found = scored.InitialPoseSearch(scan, cands, best_pose, best_score);
    std::vector<double> poses(7 * m);
    std::vector<locgpu_fitness> fit(m);
    int best = -1;
    if (locgpu_ndt_init_search(ctx, scan->points.data(), scan->points.size(), sizeof(PointType), reinterpret_cast<const double*>(cand_raw.data()), (int)m, nullptr,
                               poses.data(), fit.data(), nullptr, &best) != LOCGPU_OK)
        return 7;
    if (found != (best >= 0)) return 17;
    if (found) {
        if (std::memcmp(best_pose.data(), &poses[7 * (size_t)best], 56) != 0) return 18;
        const float want = (float)fit[best].score;
        if (std::memcmp(&best_score, &want, 4) != 0) return 19;
    } else if (!std::isinf(best_score)) {
        return 19;
    }
    { const float after = scored.GetFitnessScore(); if (std::memcmp(&score, &after, 4) != 0) return 20; }  // still the last ScanMatch's
    locgpu_destroy(ctx);

    // the incremental method is not scored and not searched: refused, in words
    {
        NdtOptions oi;
        oi.method_ = NdtMethod::INCREMENTAL_NDT;
        NdtRegistration inc(oi);
        inc.EnableFitnessScore();
        inc.SetInputTarget(map);
        CloudPtr out_inc(new PointCloudType);
        SE3 res_inc = predict;
        if (!inc.ScanMatch(scan, predict, out_inc, res_inc)) return 3;
        const float s_inc = inc.GetFitnessScore();
        if (!(std::isinf(s_inc) && s_inc > 0)) return 21;
        if (!std::strstr(inc.LastError(), "incremental")) return 22;
        SE3 bp = predict;
        float bs = -1.0f;
        if (inc.InitialPoseSearch(scan, cands, bp, bs)) return 23;
        if (!(std::isinf(bs) && bs > 0) || std::memcmp(bp.data(), predict.data(), 56) != 0) return 24;
        if (!std::strstr(inc.LastError(), "incremental")) return 25;
    }

    FILE* fo = std::fopen(argv[5], "wb");
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
