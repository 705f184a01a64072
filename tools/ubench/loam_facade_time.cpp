// tools/ubench/loam_facade_time.cpp — times LocUtils::LoamRegistration::ScanMatch as slam_demo calls it (lio.cpp:51,323-330): host feature
// clouds in, pose and a fresh output cloud out, end to end on the caller's thread. Links the façade only, so the same source times any
// build of liblocutils_gpu.so (profiles/loam_align.md compares two).
// Usage: loam_facade_time <edge_map.bin> <surf_map.bin> <edge_scan.bin> <surf_scan.bin> <pose7.bin> <warmup> <reps>   (clouds: raw float32 [n][3])
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <vector>

#include "LocUtils/model/matching/3d/loam/loam_registration.hpp"

using namespace LocUtils;

static CloudPtr load(const char* path) {
    FILE* f = std::fopen(path, "rb");
    if (!f) { std::perror(path); std::exit(2); }
    std::fseek(f, 0, SEEK_END);
    const long bytes = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    std::vector<float> raw(bytes / 4);
    if (std::fread(raw.data(), 4, raw.size(), f) != raw.size()) std::exit(2);
    std::fclose(f);
    CloudPtr c(new PointCloudType);
    c->points.resize(raw.size() / 3);
    for (size_t i = 0; i < c->points.size(); ++i) { c->points[i].x = raw[3 * i]; c->points[i].y = raw[3 * i + 1]; c->points[i].z = raw[3 * i + 2]; }
    return c;
}

int main(int argc, char** argv) {
    if (argc != 8) { std::fprintf(stderr, "usage: %s edge_map surf_map edge_scan surf_scan pose7 warmup reps\n", argv[0]); return 2; }
    CloudPtr edge_map = load(argv[1]), surf_map = load(argv[2]), edge = load(argv[3]), surf = load(argv[4]);
    SE3 predict, result;
    FILE* f = std::fopen(argv[5], "rb");
    if (!f || std::fread(predict.data(), 8, 7, f) != 7) return 2;
    std::fclose(f);
    const int warmup = std::atoi(argv[6]), reps = std::atoi(argv[7]);
    std::shared_ptr<MatchingInterface> match_ptr = std::make_shared<LoamRegistration>(LoamOption());
    match_ptr->SetInputTarget(edge_map, surf_map);
    std::vector<double> ms;
    bool ok = true;
    for (int r = -warmup; r < reps; ++r) {
        CloudPtr out(new PointCloudType);
        const auto t0 = std::chrono::steady_clock::now();
        ok = match_ptr->ScanMatch(edge, surf, predict, out, result) && ok;
        const auto t1 = std::chrono::steady_clock::now();
        if (r >= 0) ms.push_back(std::chrono::duration<double, std::milli>(t1 - t0).count());
    }
    std::sort(ms.begin(), ms.end());
    auto q = [&](double p) { return ms[std::min(ms.size() - 1, (size_t)(p * ms.size()))]; };
    std::printf("{\"ok\": %d, \"reps\": %d, \"edge\": %zu, \"surf\": %zu, \"min_ms\": %.4f, \"p10_ms\": %.4f, \"median_ms\": %.4f, \"p90_ms\": %.4f, \"max_ms\": %.4f, \"pose\": [%.17g, %.17g, %.17g, %.17g, %.17g, %.17g, %.17g]}\n",
                (int)ok, reps, edge->points.size(), surf->points.size(), ms.front(), q(0.10), q(0.50), q(0.90), ms.back(), result.data()[0], result.data()[1],
                result.data()[2], result.data()[3], result.data()[4], result.data()[5], result.data()[6]);
    return ok ? 0 : 3;
}
