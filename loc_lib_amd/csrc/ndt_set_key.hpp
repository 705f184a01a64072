// loc_lib_amd/csrc/ndt_set_key.hpp — the host-side rules of a voxel SET target (ndt_pairs.hpp): how a target's index and a voxel share
// one 64-bit key, which voxels that key can name, what an ingest refuses before the device is touched, and the per-scan words a pairs
// call forms from target_of. No HIP in here: tests/cpp/ndt_set_key_check.cpp compiles it with a plain host compiler.
//
// Key: target:16 | x:16 | y:16 | z:16, coordinates biased by 2^15 and in range for −2^15 < k < 2^15. The packing is LINEAR in the
// coordinates, as ndt_pack is (ndt_kernels.hpp): a face neighbour's key is the centre's ± one constant, and — formed in signed 64-bit
// arithmetic — centre + delta is the neighbour's key whenever the NEIGHBOUR is in range, whether the centre is or not. The all-ones
// key stays the empty marker of the table (kNdtEmpty): target 65535 is never given out, hence at most 65535 targets.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#if defined(__HIPCC__)
#define LOCGPU_HD __host__ __device__
#else
#define LOCGPU_HD
#endif

namespace locgpu {

constexpr int kNdtSetBias = 1 << 15;
constexpr int kNdtSetMaxTargets = 65535;
constexpr size_t kNdtSetMaxPoints = 0x7FFFFF00u;  // all targets together: runs and records are counted in ints on the device

LOCGPU_HD inline bool ndt_set_coord_ok(int k) { return k > -kNdtSetBias && k < kNdtSetBias; }
LOCGPU_HD inline bool ndt_set_key_in_range(int x, int y, int z) { return ndt_set_coord_ok(x) && ndt_set_coord_ok(y) && ndt_set_coord_ok(z); }
// the word a pairs call uploads per scan → the key bits of its target
LOCGPU_HD inline unsigned long long ndt_set_target_bits(uint32_t target) { return (unsigned long long)target << 48; }
// target bits + the voxel, linear and signed (any |coordinate| a 32-bit int holds: the sum wraps modulo 2^64, never overflows a signed type)
LOCGPU_HD inline unsigned long long ndt_set_pack(unsigned long long target_bits, int x, int y, int z) {
    return target_bits + (unsigned long long)((long long)x + kNdtSetBias) * (1ull << 32) + (unsigned long long)((long long)y + kNdtSetBias) * (1ull << 16) +
           (unsigned long long)((long long)z + kNdtSetBias);
}
// the key difference of the voxel at offset (ox, oy, oz), each in {-1, 0, 1}
LOCGPU_HD inline unsigned long long ndt_set_delta(int ox, int oy, int oz) {
    return (unsigned long long)((long long)ox * (1ll << 32) + (long long)oy * (1ll << 16) + (long long)oz);
}
LOCGPU_HD inline void ndt_set_unpack(unsigned long long key, int& target, int& x, int& y, int& z) {
    target = (int)(key >> 48);
    x = (int)((key >> 32) & 0xFFFF) - kNdtSetBias;
    y = (int)((key >> 16) & 0xFFFF) - kNdtSetBias;
    z = (int)(key & 0xFFFF) - kNdtSetBias;
}

// What locgpu_ndt_set_target_set refuses before it touches the device (every refusal of the host form but the key range, which the
// key kernel finds). false: `err` says why and names the target's index where there is one.
inline bool ndt_set_check_targets(const void* const* pts, const size_t* n, int n_targets, size_t stride_bytes, std::string& err) {
    if (!pts || !n) { err = "NULL arrays"; return false; }
    if (n_targets < 1 || n_targets > kNdtSetMaxTargets) { err = "n_targets = " + std::to_string(n_targets) + " is not in 1 ... " + std::to_string(kNdtSetMaxTargets); return false; }
    if (stride_bytes < 12) { err = "stride < 12"; return false; }
    size_t total = 0;
    for (int j = 0; j < n_targets; ++j) {
        if (!pts[j] || n[j] == 0) { err = "target " + std::to_string(j) + ": empty cloud"; return false; }
        if (n[j] > kNdtSetMaxPoints || total + n[j] > kNdtSetMaxPoints) { err = "target " + std::to_string(j) + ": more than " + std::to_string(kNdtSetMaxPoints) + " points in the set"; return false; }
        total += n[j];
    }
    return true;
}

// The per-scan words of a pairs call from its target_of: words[i] = base ? base[target_of[i]] : target_of[i] (ICP: the first slot of
// the target's tree in the forest; NDT: the target's index, which the kernels shift into the key, ndt_set_target_bits), skip[i] = 1
// and word 0 for target_of[i] == -1. false, with nothing written: an entry that is neither -1 nor one of the n_targets targets.
inline bool pair_words(const int* target_of, int n_scans, int n_targets, const uint32_t* base, std::vector<uint32_t>& words, std::vector<unsigned char>& skip,
                       std::string& err) {
    for (int i = 0; i < n_scans; ++i)
        if (target_of[i] < -1 || target_of[i] >= n_targets) {
            err = "target_of[" + std::to_string(i) + "] = " + std::to_string(target_of[i]) + " is neither -1 nor one of the " + std::to_string(n_targets) + " targets";
            return false;
        }
    words.assign((size_t)n_scans, 0u);
    skip.assign((size_t)n_scans, 0);
    for (int i = 0; i < n_scans; ++i) {
        if (target_of[i] < 0) skip[i] = 1;
        else words[i] = base ? base[(size_t)target_of[i]] : (uint32_t)target_of[i];
    }
    return true;
}

}  // namespace locgpu
