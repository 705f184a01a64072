// loc_lib_amd/csrc/ndt_inc.hpp — incremental NDT state and launchers (see ndt_inc.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "device_math.hpp"

namespace locgpu {

struct IncNdtState;

IncNdtState* inc_ndt_create(size_t capacity, double voxel_size);
void inc_ndt_destroy(IncNdtState* st);
size_t inc_ndt_num_voxels(const IncNdtState* st);
hipError_t inc_ndt_ingest(IncNdtState& st, const float4* host_pts, const float4* d_pts, size_t n, hipStream_t s, bool* bad_key);
void launch_inc_accum(const IncNdtState* st, double res_th, int n_nearby, const float4* src, const int* counts, const PoseState* ps, int max_n,
                      int n_scans, double* partials, hipStream_t s, const int* active = nullptr, int n_active = 0, const int* src_of = nullptr);
size_t inc_ndt_dump(const IncNdtState* st, int32_t* keys, double* mu, double* info, size_t cap);
// Test read-back of the key → slot table of the last call: its size, and the first min(cap, size) entries' raw keys (kNdtEmpty: free)
// and voxel-slot indices (-1 for a free entry). Copies only; NULL arrays are skipped.
size_t inc_ndt_table_size(const IncNdtState* st);
hipError_t inc_ndt_slots_read(const IncNdtState* st, uint64_t* keys, int32_t* vid, size_t cap, hipStream_t s);
const void* inc_ndt_table_ptr(const IncNdtState* st);

}  // namespace locgpu
