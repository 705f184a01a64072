// tests/cpp/forest_pack_check.cpp — the host packing of a forest target (build_packed_forest, csrc/kdtree_build.cpp): three clouds of 5,
// 300 and 20 000 points become three segments, each byte for byte the single-tree build of its cloud, at even ascending bases with a
// sentinel leaf behind each, the same bytes for 1 and for 8 build threads; and the refusals. Stand-alone: compiled with and without
// -fsanitize=address,undefined by tests/test_pairs_abi.py.
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "kdtree_build.hpp"

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

int main() {
    setenv("LOCGPU_BUILD_THREADS", "8", 1);  // the pool is made at the first build: eight threads whatever the host has
    std::mt19937 rng(11);
    const size_t sizes[3] = {5, 300, 20000};
    std::vector<std::vector<float>> clouds(3);
    for (int j = 0; j < 3; ++j) {
        clouds[j].resize(3 * sizes[j]);
        std::normal_distribution<float> g(0.f, j == 1 ? 0.5f : 20.f);
        for (auto& v : clouds[j]) v = g(rng);
    }
    for (size_t i = 0; i < sizes[1]; i += 7) { clouds[1][3 * i] = 1.f; clouds[1][3 * i + 1] = 2.f; clouds[1][3 * i + 2] = 3.f; }  // duplicates: a segment shorter than 3n − 1
    const float* ptr[3] = {clouds[0].data(), clouds[1].data(), clouds[2].data()};

    locgpu::PackedKdTree single[3];
    for (int j = 0; j < 3; ++j) {
        std::string err;
        CHECK(locgpu::build_packed_kdtree(ptr[j], sizes[j], single[j], err), "single build %d: %s", j, err.c_str());
    }
    locgpu::PackedForest f[2];
    const unsigned threads[2] = {1, 8};
    for (int t = 0; t < 2; ++t) {
        std::string err;
        int bad = 7;
        CHECK(locgpu::build_packed_forest(ptr, sizes, 3, f[t], err, &bad, threads[t]), "forest build with %u threads: %s", threads[t], err.c_str());
        CHECK(bad == -1, "bad index %d after a build that succeeded", bad);
        const locgpu::PackedForest& F = f[t];
        CHECK(F.base.size() == 3 && F.seg_slots.size() == 3 && F.leaves.size() == 3 && F.depth.size() == 3, "table sizes");
        CHECK(F.base[0] == 0, "base[0] = %u", F.base[0]);
        size_t leaves = 0, nodes = 0, points = 0;
        int max_depth = 0;
        for (int j = 0; j < 3; ++j) {
            CHECK(F.base[j] % 2 == 0, "base[%d] = %u is odd", j, F.base[j]);
            if (j > 0) {
                const size_t prev_end = (size_t)F.base[j - 1] + F.seg_slots[j - 1] + 2;  // the segment and its sentinel leaf
                CHECK(F.base[j] >= prev_end && F.base[j] <= prev_end + 1, "base[%d] = %u does not follow segment %d, which ends at %zu", j, F.base[j], j - 1, prev_end);
                if (F.base[j] == prev_end + 1) CHECK(F.slots[prev_end] == 0, "padding slot is not zero");
            }
            CHECK(F.seg_slots[j] == single[j].slots.size(), "segment %d has %u slots, the single build %zu", j, F.seg_slots[j], single[j].slots.size());
            CHECK((size_t)F.base[j] + F.seg_slots[j] + 2 <= F.slots.size(), "segment %d runs past the array", j);
            CHECK(std::memcmp(F.slots.data() + F.base[j], single[j].slots.data(), single[j].slots.size() * 8) == 0, "segment %d differs from the single build", j);
            const uint64_t* sent = F.slots.data() + F.base[j] + F.seg_slots[j];
            CHECK(sent[0] == locgpu::kSentinelLeafSlots[0] && sent[1] == locgpu::kSentinelLeafSlots[1], "no sentinel leaf behind segment %d", j);
            CHECK(F.leaves[j] == single[j].num_leaves && F.depth[j] == single[j].depth, "segment %d: leaves %zu / %zu, depth %d / %d", j, F.leaves[j], single[j].num_leaves,
                  F.depth[j], single[j].depth);
            leaves += single[j].num_leaves; nodes += single[j].num_nodes; points += single[j].num_points;
            if (single[j].depth > max_depth) max_depth = single[j].depth;
        }
        CHECK(F.slots.size() == (size_t)F.base[2] + F.seg_slots[2] + 2, "the array ends behind the last sentinel leaf");
        CHECK(F.slots.size() < locgpu::kForestMaxSlots, "size limit");
        CHECK(F.num_leaves == leaves && F.num_nodes == nodes && F.num_points == points && F.max_depth == max_depth && F.bounded, "totals");
    }
    // sentinel leaf: tag 3, and three coordinates whose squares overflow
    CHECK((uint32_t)(locgpu::kSentinelLeafSlots[0] >> 62) == 3u, "sentinel tag");
    CHECK(single[1].slots.size() < 3 * sizes[1] - 1, "the duplicate cloud was meant to make a shorter tree");
    CHECK(f[0].slots.size() == f[1].slots.size() && std::memcmp(f[0].slots.data(), f[1].slots.data(), f[0].slots.size() * 8) == 0, "1 and 8 threads pack different bytes");
    CHECK(f[0].base == f[1].base && f[0].seg_slots == f[1].seg_slots && f[0].depth == f[1].depth && f[0].leaves == f[1].leaves, "1 and 8 threads make different tables");

    // refusals: the index of the target that cannot be built, -1 for the forest's own
    {
        locgpu::PackedForest g;
        std::string err;
        int bad = 7;
        const size_t with_empty[3] = {5, 0, 20000};
        CHECK(!locgpu::build_packed_forest(ptr, with_empty, 3, g, err, &bad) && bad == 1 && !err.empty() && g.slots.empty(), "an empty target must be refused by index");
        const float* with_null[3] = {ptr[0], ptr[1], nullptr};
        CHECK(!locgpu::build_packed_forest(with_null, sizes, 3, g, err, &bad) && bad == 2, "a NULL target must be refused by index");
        CHECK(!locgpu::build_packed_forest(ptr, sizes, 0, g, err, &bad) && bad == -1, "n_trees = 0 must be refused");
        CHECK(!locgpu::build_packed_forest(nullptr, sizes, 3, g, err, &bad) && bad == -1, "NULL arrays must be refused");
    }
    // many small trees on the pool (more trees than threads), against their single builds
    {
        const int n = 37;
        std::vector<std::vector<float>> cs(n);
        std::vector<const float*> p(n);
        std::vector<size_t> sz(n);
        for (int j = 0; j < n; ++j) {
            sz[j] = 1 + (size_t)(rng() % 4000);
            cs[j].resize(3 * sz[j]);
            std::normal_distribution<float> g(0.f, 10.f);
            for (auto& v : cs[j]) v = g(rng);
            p[j] = cs[j].data();
        }
        locgpu::PackedForest F;
        std::string err;
        CHECK(locgpu::build_packed_forest(p.data(), sz.data(), n, F, err), "37 trees: %s", err.c_str());
        for (int j = 0; j < n; ++j) {
            locgpu::PackedKdTree t;
            CHECK(locgpu::build_packed_kdtree(p[j], sz[j], t, err), "single build");
            CHECK(F.seg_slots[j] == t.slots.size() && std::memcmp(F.slots.data() + F.base[j], t.slots.data(), t.slots.size() * 8) == 0, "tree %d of 37 differs", j);
            CHECK(F.base[j] % 2 == 0, "odd base");
        }
    }
    std::puts("forest harness ok");
    return 0;
}
