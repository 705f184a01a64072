// loc_lib_amd/csrc/forest_plan.hpp — the part of the device KD-tree build (forest_build.hip) that is the same text on
// the host and on the device: where a forest's trees stand (bases, pads), where a node's children and leaves stand, how a slot is
// encoded, and the SEQUENTIAL split of one node, which the kernel's lane-per-node path runs as it stands here. It is the arithmetic of
// Builder::split (kdtree_build.cpp; FindSplitAxisAndThresh, kdtree.cpp:96-123, mean and variance as math_utils.h:35-47): float32 sums
// in index order, one IEEE operation at a time. Compile with -ffp-contract=off.
// tests/cpp/forest_device_plan_check.cpp drives these functions level by level on the host and compares the bytes with
// build_packed_forest. That covers this header, not the kernel's cooperative path, whose sums run through LDS (same order, other code).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define LOCGPU_FPLAN_HD __host__ __device__ inline
#else
#define LOCGPU_FPLAN_HD inline
#endif

namespace locgpu {
namespace fplan {

// A point travels with its index (kdtree_build.cpp's Rec): a node's points are contiguous 16-byte records in stable-partition order.
struct alignas(16) Rec { float x, y, z; int32_t id; };
// One 8-byte slot of the packed tree, low word first (= the uint64 of kdtree_build.cpp on a little-endian machine, = a uint2).
struct alignas(8) Slot { uint32_t lo, hi; };
// A node of the current level: its points are records [off, off + len) of its tree, len >= 2, its slot is `slot` (local to the tree);
// nl = points on its left, filled in by the split.
struct alignas(16) Node { uint32_t off, len, slot, nl; };

constexpr uint32_t kSentinelLo0 = 0x7F61B1E6u, kSentinelHi0 = 0xC0000000u, kSentinelLo1 = 0x7F61B1E6u, kSentinelHi1 = 0x7F61B1E6u;  // kSentinelLeafSlots
constexpr int kMaxDepth = 64;  // the traversal stack's entries (kMaxSearchDepth): a deeper tree is refused

LOCGPU_FPLAN_HD uint32_t fbits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
LOCGPU_FPLAN_HD bool float_bounded(float f) { return __builtin_fabsf(f) < 1e18f; }  // false for NaN

// ---- layout of a forest: tree j of n points takes 3n − 1 slots from an even base, its sentinel leaf stands behind it, and a zero slot
// of padding follows where the next base would be odd (build_packed_forest).
LOCGPU_FPLAN_HD size_t tree_slots(size_t n) { return 3 * n - 1; }
LOCGPU_FPLAN_HD size_t segment_end(size_t base, size_t n) { return base + tree_slots(n) + 2; }               // behind the sentinel leaf
LOCGPU_FPLAN_HD size_t next_base(size_t base, size_t n) { const size_t e = segment_end(base, n); return e + (e & 1); }
// base[j] for every tree; *total = slots of the whole array (the end of the last sentinel leaf). false: beyond max_slots.
LOCGPU_FPLAN_HD bool plan_bases(const size_t* n, size_t n_trees, size_t max_slots, uint32_t* base, size_t* total) {
    size_t at = 0;
    for (size_t j = 0; j < n_trees; ++j) {
        at += at & 1;
        if (at + tree_slots(n[j]) + 2 > max_slots) return false;
        base[j] = (uint32_t)at;
        at = segment_end(at, n[j]);
    }
    *total = at;
    return true;
}

// ---- where the children stand: a sub-tree of m points is 3m − 1 slots, so both are known the moment the node is split (build_direct).
LOCGPU_FPLAN_HD uint32_t left_slot(uint32_t slot) { return slot + 1; }
LOCGPU_FPLAN_HD uint32_t right_slot(uint32_t slot, uint32_t nl) { return slot + 3 * nl; }
// The leaves of a tree in preorder are its points in their final order: the first leaf index of a node is its record offset.
LOCGPU_FPLAN_HD uint32_t left_leaf_pos(uint32_t off) { return off; }
LOCGPU_FPLAN_HD uint32_t right_leaf_pos(uint32_t off, uint32_t nl) { return off + nl; }

// ---- encoding
LOCGPU_FPLAN_HD Slot node_slot(float th, int axis, uint32_t right) { return Slot{fbits(th), ((uint32_t)axis << 30) | right}; }
LOCGPU_FPLAN_HD void write_leaf(Slot* at, const Rec& r) {
    at[0] = Slot{fbits(r.x), (3u << 30) | (uint32_t)r.id};
    at[1] = Slot{fbits(r.y), fbits(r.z)};
}
LOCGPU_FPLAN_HD void write_sentinel(Slot* at) {
    at[0] = Slot{kSentinelLo0, kSentinelHi0};
    at[1] = Slot{kSentinelLo1, kSentinelHi1};
}

// ---- the split
LOCGPU_FPLAN_HD int pick_axis(float vx, float vy, float vz) {  // strict >: axis 0 wins ties
    int axis = 0;
    float best = vx;
    if (vy > best) { best = vy; axis = 1; }
    if (vz > best) { best = vz; axis = 2; }
    return axis;
}
LOCGPU_FPLAN_HD float coord(const Rec& r, int axis) { return axis == 0 ? r.x : (axis == 1 ? r.y : r.z); }

struct Split { int axis; float th; uint32_t nl; };
// src[0, len) → dst[0, len): `c < th` left, else right, both sides in their order. len >= 2. The node's own sum, taken over its own
// points, is bit for bit the sum Builder::split is handed by the parent (which only adds +0.0f for the other side's points).
LOCGPU_FPLAN_HD Split split_seq(const Rec* src, Rec* dst, uint32_t len) {
    float sx = 0.f, sy = 0.f, sz = 0.f;
    for (uint32_t i = 0; i < len; ++i) { sx = sx + src[i].x; sy = sy + src[i].y; sz = sz + src[i].z; }
    const float fl = (float)len;
    const float mx = sx / fl, my = sy / fl, mz = sz / fl;
    float vx = 0.f, vy = 0.f, vz = 0.f;
    for (uint32_t i = 0; i < len; ++i) {
        const float dx = src[i].x - mx, dy = src[i].y - my, dz = src[i].z - mz;
        const float qx = dx * dx, qy = dy * dy, qz = dz * dz;
        vx = vx + qx; vy = vy + qy; vz = vz + qz;
    }
    const float fl1 = (float)(len - 1);
    vx = vx / fl1; vy = vy / fl1; vz = vz / fl1;
    Split s;
    s.axis = pick_axis(vx, vy, vz);
    s.th = s.axis == 0 ? mx : (s.axis == 1 ? my : mz);
    uint32_t nl = 0;
    for (uint32_t i = 0; i < len; ++i) nl += coord(src[i], s.axis) < s.th ? 1u : 0u;
    uint32_t l = 0, r = nl;
    for (uint32_t i = 0; i < len; ++i) {
        const Rec p = src[i];
        if (coord(p, s.axis) < s.th) dst[l++] = p;
        else dst[r++] = p;
    }
    s.nl = nl;
    return s;
}
LOCGPU_FPLAN_HD bool degenerate(uint32_t len, uint32_t nl) { return nl == 0 || nl == len; }  // every point on one side (kdtree.cpp:66-70)

// ---- behind the split of a whole level: a child of one point becomes a leaf, a longer one a node of the next level
LOCGPU_FPLAN_HD uint32_t child_nodes(const Node& nd) {
    if (degenerate(nd.len, nd.nl)) return 0;
    return (nd.nl > 1 ? 1u : 0u) + (nd.len - nd.nl > 1 ? 1u : 0u);
}
// recs: the tree's records AFTER the level's partitions; slots, leaf_slots: the tree's; next: where this node's child_nodes() go.
LOCGPU_FPLAN_HD void emit_children(const Node& nd, const Rec* recs, Slot* slots, uint32_t* leaf_slots, Node* next) {
    if (degenerate(nd.len, nd.nl)) return;
    const uint32_t nr = nd.len - nd.nl, ls = left_slot(nd.slot), rs = right_slot(nd.slot, nd.nl);
    const uint32_t lp = left_leaf_pos(nd.off), rp = right_leaf_pos(nd.off, nd.nl);
    if (nd.nl == 1) { write_leaf(slots + ls, recs[lp]); leaf_slots[lp] = ls; }
    else *next++ = Node{nd.off, nd.nl, ls, 0};
    if (nr == 1) { write_leaf(slots + rs, recs[rp]); leaf_slots[rp] = rs; }
    else *next = Node{nd.off + nd.nl, nr, rs, 0};
}

}  // namespace fplan
}  // namespace locgpu
