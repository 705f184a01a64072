// tests/cpp/facade_map_planes.cpp — IcpRegistration::EnableMapPlanes through the C++ façade (tests/test_gpu_map_planes.py):
//   * ScanMatch without EnableMapPlanes(true) — never called, or called with false — is byte-identical to LOCGPU_P2PLANE through the C ABI;
//   * with the switch on it equals locgpu_icp_scan_match with LOCGPU_P2PLANE_MAP, pose and output cloud, bit for bit;
//   * CaculateMatrixHAndB follows the switch (equals locgpu_icp_hb with the respective method).
// Usage: facade_map_planes <map.bin> <scan.bin> <pose7.bin> <out.bin>
// Cloud files: raw float32 [n][3]. out.bin (doubles): plain pose 7, map-plane pose 7.
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

struct AbiResult { double pose[7]; std::vector<PointType> cloud; double H[36], B[6]; int ok; };

static bool abi_run(locgpu_ctx* ctx, const CloudPtr& scan, const SE3& predict, int method, AbiResult& r) {
    locgpu_icp_opts co;
    locgpu_icp_opts_default(&co);
    co.method = method;
    r.cloud = scan->points;
    if (locgpu_icp_scan_match(ctx, scan->points.data(), scan->points.size(), sizeof(PointType), predict.data(), &co, r.pose, nullptr, r.cloud.data(),
                              sizeof(PointType), nullptr, nullptr) != LOCGPU_OK)
        return false;
    return locgpu_icp_hb(ctx, scan->points.data(), scan->points.size(), sizeof(PointType), predict.data(), &co, r.H, r.B, nullptr, &r.ok) == LOCGPU_OK;
}

static int same_as(IcpRegistration& reg, const CloudPtr& scan, const SE3& predict, const AbiResult& want, int base, SE3& res) {
    CloudPtr out(new PointCloudType);
    if (!reg.ScanMatch(scan, predict, out, res)) return base;
    if (std::memcmp(res.data(), want.pose, 56) != 0) return base + 1;
    if (out->points.size() != want.cloud.size() || std::memcmp(out->points.data(), want.cloud.data(), want.cloud.size() * sizeof(PointType)) != 0) return base + 2;
    Mat6d H;
    Vec6d B;
    std::memset(H.data(), 0, 36 * sizeof(double));
    std::memset(B.data(), 0, 6 * sizeof(double));
    const bool ok = reg.CaculateMatrixHAndB(scan, predict, H, B);
    if (ok != (want.ok != 0)) return base + 3;
    if (std::memcmp(H.data(), want.H, sizeof(want.H)) != 0 || std::memcmp(B.data(), want.B, sizeof(want.B)) != 0) return base + 4;  // H is symmetric: storage order irrelevant
    return 0;
}

int main(int argc, char** argv) {
    if (argc != 5) { std::fprintf(stderr, "usage\n"); return 2; }
    CloudPtr map = load(argv[1]), scan = load(argv[2]);
    SE3 predict;
    { const std::vector<char> raw = slurp(argv[3]); if (raw.size() != 56) return 2; std::memcpy(predict.data(), raw.data(), 56); }

    locgpu_ctx* ctx = nullptr;
    if (locgpu_create(0, &ctx) != LOCGPU_OK) return 5;
    if (locgpu_icp_set_target(ctx, map->points.data(), map->points.size(), sizeof(PointType)) != LOCGPU_OK) return 5;
    AbiResult plain, fast;
    if (!abi_run(ctx, scan, predict, LOCGPU_P2PLANE, plain) || !abi_run(ctx, scan, predict, LOCGPU_P2PLANE_MAP, fast)) return 6;
    locgpu_destroy(ctx);
    if (std::memcmp(plain.pose, fast.pose, 56) == 0 && std::memcmp(plain.H, fast.H, sizeof(plain.H)) == 0) return 7;  // the two methods do differ

    IcpOptions o(IcpMethod::P2PLANE);
    SE3 res_plain, res_off, res_on, res_p2p;
    IcpRegistration never(o);
    never.SetInputTarget(map);
    if (int rc = same_as(never, scan, predict, plain, 10, res_plain)) return rc;
    IcpRegistration off(o);
    off.EnableMapPlanes(false);
    off.SetInputTarget(map);
    if (int rc = same_as(off, scan, predict, plain, 20, res_off)) return rc;
    IcpRegistration on(o);
    on.EnableMapPlanes(true);
    on.SetInputTarget(map);
    if (int rc = same_as(on, scan, predict, fast, 30, res_on)) return rc;
    // switched on after the target was set: the first matching call builds the table
    IcpRegistration late(o);
    late.SetInputTarget(map);
    late.EnableMapPlanes(true);
    if (int rc = same_as(late, scan, predict, fast, 40, res_on)) return rc;
    // the switch only concerns P2PLANE
    {
        locgpu_ctx* c2 = nullptr;
        if (locgpu_create(0, &c2) != LOCGPU_OK) return 5;
        if (locgpu_icp_set_target(c2, map->points.data(), map->points.size(), sizeof(PointType)) != LOCGPU_OK) return 5;
        AbiResult p2p;
        if (!abi_run(c2, scan, predict, LOCGPU_P2P, p2p)) return 6;
        locgpu_destroy(c2);
        IcpRegistration other{IcpOptions(IcpMethod::P2P)};
        other.EnableMapPlanes(true);
        other.SetInputTarget(map);
        if (int rc = same_as(other, scan, predict, p2p, 50, res_p2p)) return rc;
    }

    FILE* fo = std::fopen(argv[4], "wb");
    if (!fo) return 2;
    std::fwrite(res_plain.data(), 8, 7, fo);
    std::fwrite(res_on.data(), 8, 7, fo);
    std::fclose(fo);
    return 0;
}
