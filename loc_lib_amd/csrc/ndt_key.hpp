// loc_lib_amd/csrc/ndt_key.hpp — the key rules of the NDT voxel tables: the empty marker, the 64-bit packed key of a single target's
// voxel (21 bits per axis, biased by 2^20, in range for −2^20 < k < 2^20) and the two hashes that give a key its first slot — ndt_hash
// (the incremental table, ndt_inc.hip) and ndt_hash32 (the direct table and the voxel set, ndt_kernels.hip / ndt_pairs.hip). The set's
// key (target above voxel) is in ndt_set_key.hpp. No HIP in here: tests/cpp/ndt_key_check.cpp compiles it with a plain host compiler,
// and tests/ndt_table_cases.py restates it in numpy to design collision chains — a change to either hash must be followed there.
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define LOCGPU_HD __host__ __device__
#else
#define LOCGPU_HD
#endif

namespace locgpu {

constexpr unsigned long long kNdtEmpty = ~0ull;
constexpr int kNdtBias = 1 << 20;

LOCGPU_HD inline bool ndt_key_in_range(int x, int y, int z) {
    return x > -kNdtBias && x < kNdtBias && y > -kNdtBias && y < kNdtBias && z > -kNdtBias && z < kNdtBias;
}
LOCGPU_HD inline unsigned long long ndt_pack(int x, int y, int z) {
    return ((unsigned long long)(unsigned)(x + kNdtBias) << 42) | ((unsigned long long)(unsigned)(y + kNdtBias) << 21) |
           (unsigned long long)(unsigned)(z + kNdtBias);
}
LOCGPU_HD inline size_t ndt_hash(unsigned long long k, size_t cap_mask) {
    k ^= k >> 33; k *= 0xff51afd7ed558ccdull; k ^= k >> 33; k *= 0xc4ceb9fe1a85ec53ull; k ^= k >> 33;
    return (size_t)k & cap_mask;
}

// Slot of a voxel in the DIRECT table (the incremental one keeps ndt_hash): the two halves of the packed key folded with one
// multiply, then the 32-bit murmur finaliser — the accumulate kernel hashes seven voxels per point, and the 64-bit finaliser seven
// times over was a good part of its integer instructions. On the bench map's 614 k voxels it collides no more often than the 64-bit
// one (11 k keys share a first slot at load 0.02; x·A ^ y·B ^ z·C, the classic spatial hash, ten times as many: walls and ground are
// lattices of keys, and its products cancel on them).
LOCGPU_HD inline size_t ndt_hash32(unsigned long long key, size_t cap_mask) {
    uint32_t h = (uint32_t)key + (uint32_t)(key >> 32) * 0x9E3779B1u;
    h ^= h >> 16; h *= 0x85ebca6bu; h ^= h >> 13; h *= 0xc2b2ae35u; h ^= h >> 16;
    return (size_t)h & cap_mask;
}

}  // namespace locgpu
