// tests/cpp/facade_loam_search.cpp — the LOAM matcher's joint fitness score and initial-pose search through the C++ façade
// (tests/test_loam_search_abi.py without arguments, tests/test_gpu_loam_init_search.py with them):
//   * GetFitnessScore() is the reference's 0.0f without EnableFitnessScore (loam_registration.cpp:101-104); after it, +infinity before
//     any ScanMatch — both without touching a device: this is all the program does when it is run without arguments;
//   * then the score of the last ScanMatch — the very bits locgpu_loam_fitness gives for the same scans and pose;
//   * ScanMatch's pose and output cloud are byte-identical with and without the opt-in;
//   * InitialPoseSearch returns what locgpu_loam_init_search returns.
// Usage: facade_loam_search [<edge_map.bin> <surf_map.bin> <edge.bin> <surf.bin> <pose7.bin> <candidates.bin> <out.bin>]
// Cloud files: raw float32 [n][3]; candidates.bin: m × 7 doubles. out.bin (doubles): pose 7, façade score, ABI joint score, joint
// inliers, joint finite points, best pose 7, best score, best index.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../include/locgpu.h"
#include "LocUtils/model/matching/3d/loam/loam_registration.hpp"

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
    if (argc != 1 && argc != 8) { std::fprintf(stderr, "usage\n"); return 2; }
    LoamOption o;  // the reference's defaults: both classes, 20 iterations, eps 1e-3
    {
        // no target, no ScanMatch, no device: the stub without the opt-in, +infinity and a reason with it
        LoamRegistration plain(o);
        if (plain.GetFitnessScore() != 0.0f) return 10;
        LoamRegistration scored(o);
        scored.EnableFitnessScore(1.0);
        const float before = scored.GetFitnessScore();
        if (!(std::isinf(before) && before > 0)) return 12;
        if (!std::strstr(scored.LastError(), "ScanMatch")) return 26;
        // a search without targets is refused in words, best_pose untouched
        SE3 bp, kept;
        std::memcpy(kept.data(), bp.data(), 56);
        float bs = -1.0f;
        CloudPtr none(new PointCloudType);
        if (scored.InitialPoseSearch(none, none, std::vector<SE3>(1), bp, bs)) return 27;
        if (!(std::isinf(bs) && bs > 0) || std::memcmp(bp.data(), kept.data(), 56) != 0 || !std::strstr(scored.LastError(), "SetInputTarget")) return 28;
    }
    if (argc == 1) return 0;

    CloudPtr edge_map = load(argv[1]), surf_map = load(argv[2]), edge = load(argv[3]), surf = load(argv[4]);
    SE3 predict;
    { const std::vector<char> raw = slurp(argv[5]); if (raw.size() != 56) return 2; std::memcpy(predict.data(), raw.data(), 56); }
    const std::vector<char> cand_raw = slurp(argv[6]);
    const size_t m = cand_raw.size() / 56;
    std::vector<SE3> cands(m);
    for (size_t i = 0; i < m; ++i) std::memcpy(cands[i].data(), cand_raw.data() + 56 * i, 56);

    // without the opt-in: the drop-in behaviour
    LoamRegistration plain(o);
    plain.SetInputTarget(edge_map, surf_map);
    CloudPtr out_plain(new PointCloudType);
    SE3 res_plain = predict;
    if (!plain.ScanMatch(edge, surf, predict, out_plain, res_plain)) return 3;
    if (plain.GetFitnessScore() != 0.0f) return 11;

    // with it
    LoamRegistration scored(o);
    scored.EnableFitnessScore(1.0);
    scored.SetInputTarget(edge_map, surf_map);
    { const float before = scored.GetFitnessScore(); if (!(std::isinf(before) && before > 0)) return 12; }  // nothing matched yet
    CloudPtr out_scored(new PointCloudType);
    SE3 res_scored = predict;
    if (!scored.ScanMatch(edge, surf, predict, out_scored, res_scored)) return 3;
    const float score = scored.GetFitnessScore();
    if (std::memcmp(res_plain.data(), res_scored.data(), 56) != 0) return 13;
    if (out_plain->points.size() != out_scored->points.size() ||
        std::memcmp(out_plain->points.data(), out_scored->points.data(), out_plain->points.size() * sizeof(PointType)) != 0)
        return 14;
    const float again = scored.GetFitnessScore();
    if (std::memcmp(&score, &again, 4) != 0) return 15;

    // the C ABI on the same scans and pose, through a handle that owns its contexts
    locgpu_loam_opts lo;
    locgpu_loam_opts_default(&lo);  // LoamOption's defaults, and the façade's approximate search (ann_alpha 0.1)
    locgpu_loam* l = nullptr;
    if (locgpu_loam_create(0, &lo, &l) != LOCGPU_OK) return 5;
    if (locgpu_loam_set_target(l, edge_map->points.data(), edge_map->points.size(), surf_map->points.data(), surf_map->points.size(), sizeof(PointType)) != LOCGPU_OK) return 5;
    locgpu_fitness f[3];
    if (locgpu_loam_fitness(l, edge->points.data(), edge->points.size(), surf->points.data(), surf->points.size(), sizeof(PointType), res_scored.data(), 1, 1.0, f) !=
        LOCGPU_OK)
        return 6;
    const float abi_score = (float)f[0].score;
    if (std::memcmp(&score, &abi_score, 4) != 0) return 16;

    // InitialPoseSearch against locgpu_loam_init_search
    SE3 best_pose;
    float best_score = -1.0f;
    const bool found = scored.InitialPoseSearch(edge, surf, cands, best_pose, best_score);
    std::vector<double> poses(7 * m);
    std::vector<locgpu_fitness> fit(3 * m);
    int best = -1;
    if (locgpu_loam_init_search(l, edge->points.data(), edge->points.size(), surf->points.data(), surf->points.size(), sizeof(PointType),
                                reinterpret_cast<const double*>(cand_raw.data()), (int)m, nullptr, poses.data(), fit.data(), nullptr, &best) != LOCGPU_OK)
        return 7;
    if (found != (best >= 0)) return 17;
    if (found) {
        if (std::memcmp(best_pose.data(), &poses[7 * (size_t)best], 56) != 0) return 18;
        const float want = (float)fit[3 * (size_t)best].score;
        if (std::memcmp(&best_score, &want, 4) != 0) return 19;
    } else if (!std::isinf(best_score)) {
        return 19;
    }
    { const float after = scored.GetFitnessScore(); if (std::memcmp(&score, &after, 4) != 0) return 20; }  // still the last ScanMatch's
    // ... and a ScanMatch after the search is still the plain one's
    CloudPtr out_after(new PointCloudType);
    SE3 res_after = predict;
    if (!scored.ScanMatch(edge, surf, predict, out_after, res_after)) return 3;
    if (std::memcmp(res_plain.data(), res_after.data(), 56) != 0) return 21;
    locgpu_loam_destroy(l);

    FILE* fo = std::fopen(argv[7], "wb");
    if (!fo) return 2;
    std::fwrite(res_scored.data(), 8, 7, fo);
    const double tail[4] = {(double)score, f[0].score, (double)f[0].inliers, (double)f[0].finite_points};
    std::fwrite(tail, 8, 4, fo);
    std::fwrite(best_pose.data(), 8, 7, fo);
    const double tail2[2] = {(double)best_score, (double)best};
    std::fwrite(tail2, 8, 2, fo);
    std::fclose(fo);
    return 0;
}
