// tests/cpp/forest_device_plan_check.cpp — the host half of the device KD-tree build (csrc/forest_plan.hpp): the layout rules (bases,
// pads, child slot, leaf position, slot encoding) and the sequential per-node split that the kernel's lane-per-node path runs, driven
// level by level on the host the way the kernel drives them (one list of nodes per level, records ping-ponged between two arrays,
// children listed in their parents' order), against build_packed_forest byte for byte and build_packed_kdtree's leaf slots and depth.
// It does NOT cover the kernel's cooperative path (a wave's sums through LDS): the GPU tests do. Stand-alone: compiled with and without
// -fsanitize=address,undefined by tests/test_forest_device_abi.py.
#include <cmath>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>
#include "forest_plan.hpp"
#include "kdtree_build.hpp"

#define CHECK(cond, ...) do { if (!(cond)) { std::printf("FAILED %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); return 1; } } while (0)

using namespace locgpu;
using fplan::Node;
using fplan::Rec;
using fplan::Slot;

struct Built { int depth = 0; bool bounded = true, degenerate = false, too_deep = false; };

// One tree, level by level: what one workgroup of forest_build_kernel does, one node after the other.
static Built build_levels(const float* xyz, uint32_t n, Slot* slots, uint32_t* leaf_slots, bool pad) {
    Built out;
    std::vector<Rec> rec[2] = {std::vector<Rec>(n), std::vector<Rec>(n)};
    std::vector<Node> list[2] = {std::vector<Node>(n / 2 + 1), std::vector<Node>(n / 2 + 1)};
    fplan::write_sentinel(slots + fplan::tree_slots(n));
    if (pad) slots[fplan::tree_slots(n) + 2] = Slot{0u, 0u};
    for (uint32_t i = 0; i < n; ++i) {
        rec[0][i] = Rec{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], (int32_t)i};
        if (!(fplan::float_bounded(rec[0][i].x) && fplan::float_bounded(rec[0][i].y) && fplan::float_bounded(rec[0][i].z))) out.bounded = false;
    }
    if (n == 1) { fplan::write_leaf(slots, rec[0][0]); leaf_slots[0] = 0; out.depth = 1; return out; }
    list[0][0] = Node{0u, n, 0u, 0u};
    uint32_t count = 1;
    int level = 1, cur = 0;
    while (count > 0 && !out.degenerate) {
        if (level >= fplan::kMaxDepth) { out.too_deep = true; break; }
        for (uint32_t i = 0; i < count; ++i) {
            Node& nd = list[cur][i];
            const fplan::Split sp = fplan::split_seq(rec[cur].data() + nd.off, rec[cur ^ 1].data() + nd.off, nd.len);
            slots[nd.slot] = fplan::node_slot(sp.th, sp.axis, fplan::right_slot(nd.slot, sp.nl));
            nd.nl = sp.nl;
            if (!fplan::float_bounded(sp.th)) out.bounded = false;
            if (fplan::degenerate(nd.len, sp.nl)) out.degenerate = true;
        }
        uint32_t at = 0;
        for (uint32_t i = 0; i < count; ++i) {
            const Node nd = list[cur][i];
            if (at + fplan::child_nodes(nd) > list[cur ^ 1].size()) { std::printf("node list overflow\n"); std::exit(1); }
            fplan::emit_children(nd, rec[cur ^ 1].data(), slots, leaf_slots, list[cur ^ 1].data() + at);
            at += fplan::child_nodes(nd);
        }
        count = at;
        cur ^= 1;
        ++level;
    }
    out.depth = level;
    return out;
}

int main() {
    setenv("LOCGPU_BUILD_THREADS", "4", 1);
    std::mt19937 rng(25);
    // sizes of both parities, around the kernel's tile and lane thresholds, a local map; and the special clouds of the GPU test
    std::vector<size_t> sizes = {1, 2, 3, 5, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2049, 4000, 20000};
    std::vector<std::vector<float>> clouds;
    for (size_t s : sizes) {
        std::vector<float> c(3 * s);
        std::normal_distribution<float> g(0.f, 20.f);
        for (auto& v : c) v = g(rng);
        clouds.push_back(c);
    }
    {   // a line along y: two variances are zero
        std::vector<float> c(3 * 301);
        for (size_t i = 0; i < 301; ++i) { c[3 * i] = 1.5f; c[3 * i + 1] = 0.37f * (float)((i * 97) % 301); c[3 * i + 2] = -2.f; }
        clouds.push_back(c);
    }
    {   // equal x and y variances (y is x of the same points, permuted by reflection: the same multiset of deviations is NOT enough — the sums must agree bit for bit, so y = x)
        std::vector<float> c(3 * 500);
        std::normal_distribution<float> g(0.f, 5.f);
        for (size_t i = 0; i < 500; ++i) { const float v = g(rng); c[3 * i] = v; c[3 * i + 1] = v; c[3 * i + 2] = 0.1f * g(rng); }
        clouds.push_back(c);
    }
    {   // 4000 points about 5000 m from the origin: the sums round
        std::vector<float> c(3 * 4000);
        std::normal_distribution<float> g(0.f, 20.f);
        for (size_t i = 0; i < 4000; ++i) { c[3 * i] = 5000.f + g(rng); c[3 * i + 1] = -5000.f + g(rng); c[3 * i + 2] = 0.1f * g(rng); }
        clouds.push_back(c);
    }
    {   // scaled by 1e-22: squares are subnormal
        std::vector<float> c(3 * 777);
        std::normal_distribution<float> g(0.f, 20.f);
        for (auto& v : c) v = g(rng) * 1e-22f;
        clouds.push_back(c);
    }
    const size_t n_trees = clouds.size();
    std::vector<const float*> ptr(n_trees);
    std::vector<size_t> n(n_trees);
    for (size_t j = 0; j < n_trees; ++j) { ptr[j] = clouds[j].data(); n[j] = clouds[j].size() / 3; }

    PackedForest F;
    std::string err;
    CHECK(build_packed_forest(ptr.data(), n.data(), (int)n_trees, F, err), "host forest: %s", err.c_str());
    std::vector<uint32_t> base(n_trees);
    size_t total = 0;
    CHECK(fplan::plan_bases(n.data(), n_trees, kForestMaxSlots, base.data(), &total), "plan_bases refused");
    CHECK(total == F.slots.size(), "planned %zu slots, the host forest has %zu", total, F.slots.size());
    CHECK(base == F.base, "bases differ");
    size_t pads = 0;
    std::vector<uint64_t> mine(total, 0xAAAAAAAAAAAAAAAAull);  // not zero: a pad the plan forgets to write shows
    static_assert(sizeof(Slot) == 8, "slot");
    for (size_t j = 0; j < n_trees; ++j) {
        PackedKdTree single;
        CHECK(build_packed_kdtree(ptr[j], n[j], single, err), "single build %zu", j);
        CHECK(single.slots.size() == 3 * n[j] - 1, "cloud %zu has a degenerate split: not a case for the device plan", j);
        const bool pad = j + 1 < n_trees && base[j + 1] != fplan::segment_end(base[j], n[j]);
        pads += pad;
        std::vector<uint32_t> leaf_slots(n[j], 0xFFFFFFFFu);
        const Built b = build_levels(ptr[j], (uint32_t)n[j], reinterpret_cast<Slot*>(mine.data()) + base[j], leaf_slots.data(), pad);
        CHECK(!b.degenerate && !b.too_deep, "tree %zu: degenerate %d, too deep %d", j, b.degenerate, b.too_deep);
        CHECK(b.depth == single.depth && b.depth == F.depth[j], "tree %zu: depth %d, host %d", j, b.depth, single.depth);
        CHECK(b.bounded == single.bounded, "tree %zu: bounded %d, host %d", j, b.bounded, single.bounded);
        CHECK(leaf_slots == single.leaf_slots, "tree %zu: leaf slots differ", j);
        CHECK(std::memcmp(mine.data() + base[j], single.slots.data(), single.slots.size() * 8) == 0, "tree %zu differs from the host build", j);
    }
    CHECK(pads > 0, "the sizes were meant to need a pad slot");
    CHECK(std::memcmp(mine.data(), F.slots.data(), total * 8) == 0, "the forest differs from build_packed_forest");

    // layout rules on their own
    CHECK(fplan::next_base(0, 1) == 4 && fplan::next_base(0, 2) == 8 && fplan::segment_end(0, 2) == 7, "bases");
    {
        const size_t big[2] = {(size_t)1 << 27, (size_t)1 << 27};
        uint32_t bb[2];
        size_t tt;
        CHECK(!fplan::plan_bases(big, 2, kForestMaxSlots, bb, &tt), "a forest beyond the limit must be refused");
    }
    // flags: a duplicated point is found degenerate, 1e19 unbounded like the host
    {
        std::vector<float> c = clouds[5];
        c[3 * 7] = c[3 * 8]; c[3 * 7 + 1] = c[3 * 8 + 1]; c[3 * 7 + 2] = c[3 * 8 + 2];
        std::vector<uint64_t> s(3 * 32 + 2);
        std::vector<uint32_t> l(32);
        CHECK(build_levels(c.data(), 32, reinterpret_cast<Slot*>(s.data()), l.data(), false).degenerate, "a duplicated point must be flagged");
        c = clouds[5];
        c[3 * 9 + 1] = 1e19f;
        PackedKdTree single;
        CHECK(build_packed_kdtree(c.data(), 32, single, err), "single");
        const Built b = build_levels(c.data(), 32, reinterpret_cast<Slot*>(s.data()), l.data(), false);
        CHECK(b.degenerate == (single.slots.size() != 3 * 32 - 1), "1e19: degenerate %d", b.degenerate);
        CHECK(b.degenerate || (b.bounded == single.bounded && !b.bounded && std::memcmp(s.data(), single.slots.data(), single.slots.size() * 8) == 0), "1e19: bounded / bytes");
    }
    std::puts("forest device plan ok");
    return 0;
}
