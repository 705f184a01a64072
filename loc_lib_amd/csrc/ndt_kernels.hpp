// loc_lib_amd/csrc/ndt_kernels.hpp — direct-NDT voxel table in HBM and its kernels' launchers.
//
// Replaces std::unordered_map<Eigen::Vector3i, NdtVoxelData> grids_ (ndt_registration.hpp:130) with an open-addressing hash
// table of 16-byte slots {64-bit packed key (21 bits per axis, biased), dense voxel index} — four to a cache line, so a collision walk
// mostly stays in the line it started in — and a DENSE array of 128-byte records {μ (3 f64), info (9 f64, row-major), key}: one more
// cache line once the key has been found (rounds 1-4: key → voxel index → μ → info, three dependent gathers into four arrays; a
// record per table slot instead of a dense array was measured too: a four times larger footprint, 13 % slower). Only voxels the
// reference keeps (count > min_pts_in_voxel, ndt cpp:111,137) are in the table.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "device_buffer.hpp"
#include "device_math.hpp"
#include "ndt_key.hpp"
#include "ndt_set_key.hpp"

struct alignas(128) NdtRecord {
    double mu[3];
    double info[9];
    unsigned long long key;
    double pad[3];
};
static_assert(sizeof(NdtRecord) == 128, "one cache line per voxel");
struct alignas(16) NdtSlot {
    unsigned long long key;  // kNdtEmpty when free
    unsigned int vid;        // index of the voxel's record
    unsigned int pad;
};

struct NdtTable {
    locgpu::DevBuf<NdtSlot> d_slots;  // [cap]
    locgpu::DevBuf<NdtRecord> d_rec;  // [n_vox (allocated: runs)], dense
    size_t cap = 0, n_vox = 0;
    double inv_voxel = 1.0;
    double res_outlier_th = 20.0;
    int n_nearby = 7;
};

namespace locgpu {

// Voxel of a point: `(pt * inv_voxel_size_).cast<int>()` (ndt cpp:100,404).
__device__ __forceinline__ void ndt_key_of(const D3& p, double inv, int& kx, int& ky, int& kz) {
    kx = (int)(p.x * inv); ky = (int)(p.y * inv); kz = (int)(p.z * inv);  // C++ double→int: truncation toward zero
}

// The key rule of a look-up kernel (ndt_accum_kernel, ndt_fitness_accum_kernel): how the seven keys of a point are formed. Passed to the
// kernel by value as its last argument; the kernels are templates over it and carry the rest of their text once.
struct NdtOneTarget {};  // ndt_pack keys, coordinates within ±2^20: a table built by ndt_build
struct NdtVoxelSet {     // ndt_set_pack keys (ndt_set_key.hpp) under the target of the scan, coordinates within ±2^15: ndt_set_build
    const uint32_t* pair_target;  // [n_scans] on the device: the target's index, which the kernel shifts into the key
};

// Sizes and allocates t's slots and n_rec records for `runs` voxel runs, fills the slots with the empty marker and zeroes the records
// (enqueued on s). Sets t.cap.
hipError_t ndt_table_alloc(NdtTable& t, size_t runs, size_t n_rec, hipStream_t s);
// Build (SetDirectNdtTargetCloud, ndt_registration.cpp:87-148). Returns hipError; *bad_key is set when a point falls
// outside the ±2^20-voxel key range.
hipError_t ndt_build(NdtTable& t, const float4* d_pts, size_t n, double voxel_size, int min_pts_in_voxel, hipStream_t s, bool* bad_key);
// Test read-back: records [first, first + n) as dense arrays (keys n×3 int32, mu n×3, info n×9), in table order. set_keys: the keys are
// a voxel set's (ndt_set_unpack, the target dropped), else ndt_pack's.
hipError_t ndt_dump_range(const NdtTable& t, size_t first, size_t n, bool set_keys, int* keys, double* mu, double* info, hipStream_t s);
// ... up to out_cap voxels of a single-target table, from the first.
hipError_t ndt_dump(const NdtTable& t, int* keys, double* mu, double* info, size_t out_cap, hipStream_t s);
// Test read-back of the slot array itself: the first min(out_cap, t.cap) slots' raw keys (kNdtEmpty: free) and record indices (-1 for a
// free slot), in slot order. Copies only; NULL arrays are skipped.
hipError_t ndt_slots_read(const NdtTable& t, uint64_t* keys, int32_t* vid, size_t out_cap, hipStream_t s);

// K5: per-point 7-voxel probe + χ² gate + un-weighted JᵀJ / Jᵀe sums (AlignNdt inner loop, ndt cpp:399-433).
// active / n_active (optional): the scans to launch (SearchArgs::active); split_scans > 0: split the partial sums as a plain batch of
// that many scans would (AccumArgs::split_scans). pair_target (optional): t is a voxel set and scan i is looked up under target
// pair_target[i] of it (a device array of n_scans words, locgpu_batch::d_pair_base) — same grid, same split of the sums, same partial
// layout; nullptr: t holds one target.
int launch_ndt_accum(const NdtTable* t, const float4* src, const int* counts, const PoseState* st, int max_n, int n_scans, double* partials,
                     hipStream_t s, const int* active = nullptr, int n_active = 0, int split_scans = 0, const int* src_of = nullptr,
                     const uint32_t* pair_target = nullptr);

// Fitness score against the direct table (ndt_fitness.hip): per scan {Σ over the inliers of the smallest accepted residual, inliers,
// finite points, 0} → out[scan][kFitW] (launch.hpp). partials: room for n_scans × icp_fitness_rows(max_n) × kFitW doubles.
// pair_target: as for launch_ndt_accum.
void launch_ndt_fitness(const NdtTable* t, const float4* src, const int* counts, const PoseState* st, int max_n, int n_scans, double* partials,
                        double* out, hipStream_t s, const int* src_of = nullptr, const uint32_t* pair_target = nullptr);

}  // namespace locgpu
