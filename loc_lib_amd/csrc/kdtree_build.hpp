// loc_lib_amd/csrc/kdtree_build.hpp — host-side packed KD-tree ingest (see kdtree_build.cpp).
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

namespace locgpu {

struct PackedKdTree {
    std::vector<uint64_t> slots;  // 8-byte slots, preorder (layout in kdtree_build.cpp)
    std::vector<uint32_t> leaf_slots;  // slot index of every leaf, in preorder (what the exact-search grid is built from on the device)
    size_t num_leaves = 0;        // KdTree::size_ (kdtree.h:124)
    size_t num_nodes = 0;         // internal + leaf nodes
    size_t num_points = 0;
    int depth = 0;                // root = level 1
    bool bounded = true;          // every coordinate and split threshold is finite and below 1e18 in magnitude (squared distances cannot overflow)
};

// xyz: n packed float32 triples. Returns false and sets err on failure.
bool build_packed_kdtree(const float* xyz, size_t n, PackedKdTree& out, std::string& err);

// The sentinel leaf that stands behind a packed tree (two slots; icp_target.hip, search_walk.hpp): coordinates so large that the
// squared distance overflows to +inf for every sane query. {x = 3.0e38f ; tag 3, index 0} {y = 3.0e38f ; z = 3.0e38f}.
constexpr uint64_t kSentinelLeafSlots[2] = {0xC00000007F61B1E6ull, 0x7F61B1E67F61B1E6ull};

// A forest: n trees, each slot for slot what build_packed_kdtree makes of its cloud alone (local slot indices, root at local slot
// 0), packed behind one another in ONE array. Segment j starts at base[j] — a multiple of 2 slots (a leaf is read with one 16-byte
// load), base[0] = 0 — holds seg_slots[j] slots and is followed by its own sentinel leaf; a slot of padding (zero) follows where the
// next base would be odd. slots.size() = the end of the last segment's sentinel leaf.
// The whole forest must lie below kForestMaxSlots slots (4 GiB, what ONE tree may hold: build_packed_kdtree's own limit), which also
// keeps every absolute slot far below the search stage's kInvalidSlot.
constexpr size_t kForestMaxSlots = (size_t)1 << 29;
struct PackedForest {
    std::vector<uint64_t> slots;
    std::vector<uint32_t> base, seg_slots;
    std::vector<size_t> leaves;  // per tree: KdTree::size_
    std::vector<int> depth;      // per tree, root = level 1
    size_t num_leaves = 0, num_nodes = 0, num_points = 0;  // over all trees
    int max_depth = 0;
    bool bounded = true;  // AND over the trees
};
// xyz[j]: n[j] packed float32 triples. Trees are built in parallel ACROSS trees — each one by a single thread, in the builder's own
// summation order — on the build pool, with as many threads as build_packed_kdtree would wake for a cloud of all the points together
// (max_threads > 0: at most that many; the tests' knob). Returns false and sets err on failure; *bad (optional) = the index of the
// tree that could not be built, -1 when the failure is the forest's (its size).
bool build_packed_forest(const float* const* xyz, const size_t* n, int n_trees, PackedForest& out, std::string& err, int* bad = nullptr, unsigned max_threads = 0);

}  // namespace locgpu
