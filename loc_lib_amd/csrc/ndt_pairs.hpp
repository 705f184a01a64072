// loc_lib_amd/csrc/ndt_pairs.hpp — pairwise batch NDT: the build of a voxel SET target (include/locgpu.h, "Pairwise batch NDT";
// DESIGN.md §23). A scan is looked up in its own grid of the set by launch_ndt_accum / launch_ndt_fitness with pair_target
// (ndt_kernels.hpp).
//
// A set of n targets is ONE NdtTable in the layout of ndt_kernels.hpp — 16-byte slots, open addressing, dense 128-byte records — whose
// 64-bit keys carry the target's index above the voxel (ndt_set_key.hpp: target:16 | x:16 | y:16 | z:16), so a scan's look-up in its
// own target is the ordinary look-up under another key: no second compare, no second table. The records of a target are dense and in
// key order, target after target. The build is the ordinary build's sequence (ndt_ingest.hpp) run once over all targets' points.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <vector>

#include "ndt_kernels.hpp"
#include "ndt_set_key.hpp"

namespace locgpu {

// What the build's one read-back holds per target.
struct NdtSetTarget {
    int points = 0, runs = 0, voxels = 0, bad_key = 0;  // voxels: the runs with more than min_pts_in_voxel points, i.e. the records
};

// SetDirectNdtTargetCloud (ndt_registration.cpp:87-148) of n_targets clouds into `t`: target j = counts[j] points from
// d_pts + j * scan_stride (a batch's scan-major storage), or, scan_stride == 0, behind one another (the packed concatenation).
// `t` is replaced as a whole and only on success; info[j] is filled whenever the read-back came back. *bad_target: the first target
// with a point outside the set's ±2^15-voxel key range (t untouched), else -1. Blocking on `s`.
hipError_t ndt_set_build(NdtTable& t, const float4* d_pts, size_t scan_stride, const int* counts, int n_targets, double voxel_size, int min_pts_in_voxel, hipStream_t s,
                         std::vector<NdtSetTarget>& info, int* bad_target);
// Test read-back: records [first, first + n) as dense arrays (keys n×3 int32 without the target, mu n×3, info n×9), in key order.
hipError_t ndt_set_dump(const NdtTable& t, size_t first, size_t n, int* keys, double* mu, double* info, hipStream_t s);

}  // namespace locgpu
