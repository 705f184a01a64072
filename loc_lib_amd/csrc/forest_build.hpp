// loc_lib_amd/csrc/forest_build.hpp — the packed KD-trees of a forest built on the device (forest_build.hip).
#pragma once
#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "device_buffer.hpp"
#include "forest_plan.hpp"

struct locgpu_ctx;

namespace locgpu {

// One workgroup of kFbThreads builds one tree, level by level. A node longer than kFbLaneLen points is split by ONE WAVE: its lanes
// load tiles of kFbTile points and write the terms to the wave's LDS tile, lanes 0..2 run the three dependent sums in index order.
// A node of at most kFbLaneLen points is split by one lane (fplan::split_seq).
constexpr int kFbThreads = 1024, kFbWaves = kFbThreads / 64, kFbTile = 256, kFbLaneLen = 32;

// What the host tells the kernel about tree j, and what it gets back.
struct ForestBuildTab {
    unsigned long long src_off;  // first point of the tree in the source array (float4 {x, y, z, ·})
    uint32_t pt_off;             // first record / leaf index of the tree in the scratch arrays
    uint32_t node_off;           // first entry of the tree's node lists (n / 2 + 1 entries each)
    uint32_t n;                  // points
    uint32_t base;               // first slot of the tree in the output array (even)
    uint32_t pad;                // 1: a zero slot follows the sentinel leaf (the next base would be odd)
    uint32_t reserved;
};
constexpr uint32_t kFbUnbounded = 1u, kFbDegenerate = 2u, kFbTooDeep = 4u;
struct ForestBuildRes { int32_t depth; uint32_t flags; };

// The context's share: grow-only scratch, the tree being built beside ctx->d_tree, and what locgpu_icp_device_build_info reports.
struct ForestBuildScratch {
    DevBuf<float4> recs;           // [2][points]: the records, ping-ponged between levels
    DevBuf<fplan::Node> nodes;     // [2][node entries]
    DevBuf<ForestBuildTab> tab;
    DevBuf<ForestBuildRes> res;
    DevBuf<uint2> tree;            // swapped with ctx->d_tree on success
    DevBuf<uint32_t> leaf_slots;   // swapped with ctx->d_leaf_slots on success
    Event ev[2];                   // round the kernel, under LOCGPU_FOREST_TIMES only
    int last_path = 0;             // 0: no such call yet, 1: device build, 2: host build (a degenerate split)
    int last_kind = 0;             // 1: forest, 2: single cloud
    int first_degenerate = -1;
    int levels = 0;
};

// Enqueues the build of n_trees trees on `s`. recs: 2 × points, nodes: 2 × node_entries. tree / leaf_slots: the output arrays (slots
// from tab[j].base, leaf slots from tab[j].pt_off, local to the tree).
void launch_forest_build(const float4* src, const ForestBuildTab* tab, int n_trees, float4* recs, size_t points, fplan::Node* nodes, size_t node_entries, uint2* tree,
                         uint32_t* leaf_slots, ForestBuildRes* res, hipStream_t s);

}  // namespace locgpu
