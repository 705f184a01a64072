// loc_lib_amd/csrc/loam_sector.hpp — the per-point and per-sector bodies of the LOAM feature picker, written ONCE for the single-cloud
// pass (loam_features.hip) and the batched pass (batch_loam.hip). Every quirk of LoamFeatureExtract::Extract + ExtractFromSector
// (loam_feature_extract.cpp:19-151) listed at the top of loam_features.hip lives here: both passes call these functions on a
// ring-ordered cloud L and a table of ring starts, so a ring gives the same bytes whichever pass it went through.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace locgpu {
namespace loam {

constexpr int kLB = 256;           // threads per workgroup of every picker kernel
constexpr int kMaxSector = 2048;   // longest sector (ring length / 6) the LDS sort holds
constexpr int kMaxEdges = 20;
constexpr uint32_t kMinRing = 131;  // rings with fewer points are skipped (:40-43)

// first position of the ascending keys[0..n) whose key is ≥ r
__device__ __forceinline__ uint32_t key_lower_bound(const uint32_t* __restrict__ keys, uint32_t n, uint32_t r) {
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (keys[mid] < r) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

// curvature of the point P of a ring, P[-5..5] its ring neighbours (loam_feature_extract.cpp:47-69): float32 sums left to right,
// the squared norm in double.
__device__ __forceinline__ double ring_curvature(const float4* P) {
    const float fx = P[-5].x + P[-4].x + P[-3].x + P[-2].x + P[-1].x - 10 * P[0].x + P[1].x + P[2].x + P[3].x + P[4].x + P[5].x;
    const float fy = P[-5].y + P[-4].y + P[-3].y + P[-2].y + P[-1].y - 10 * P[0].y + P[1].y + P[2].y + P[3].y + P[4].y + P[5].y;
    const float fz = P[-5].z + P[-4].z + P[-3].z + P[-2].z + P[-1].z - 10 * P[0].z + P[1].z + P[2].z + P[3].z + P[4].z + P[5].z;
    const double dx = fx, dy = fy, dz = fz;
    return dx * dx + dy * dy + dz * dz;
}

__device__ __forceinline__ bool gap_too_large(const float4& a, const float4& b) {
    const double dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;  // float differences, widened (:123-126)
    return dx * dx + dy * dy + dz * dz > 0.05;
}

// First element of sector `sec` of a ring of `size` points, relative to ring position 5 (the first point with a curvature).
__device__ __forceinline__ int sector_start(uint32_t size, int sec) { return (((int)size - 10) / 6) * sec; }

// Sector `sec` of the ring L[base .. base + size), by one workgroup of kLB threads (all of them call this). Writes the sector's edges
// to edge_slot[task·20 …] and its surface points to surf_slot[base + 5 + sector start …] (sectors do not overlap there), plus the two
// counts of the task. A sector longer than kMaxSector sets *too_long and counts nothing.
__device__ __forceinline__ void sector_body(const float4* __restrict__ L, const double* __restrict__ curv, uint32_t base, uint32_t size, int sec, size_t task,
                                            float4* __restrict__ edge_slot, float4* __restrict__ surf_slot, uint32_t* __restrict__ edge_cnt,
                                            uint32_t* __restrict__ surf_cnt, int32_t* too_long) {
    __shared__ double s_val[kMaxSector];
    __shared__ int s_id[kMaxSector];
    __shared__ unsigned char s_picked[kMaxSector + 16];
    __shared__ int s_edges[kMaxEdges];
    __shared__ int s_n_edge;
    __shared__ uint32_t s_wave[kLB / 64];
    const int tid = threadIdx.x;
    if (size < kMinRing) {
        if (tid == 0) { edge_cnt[task] = 0; surf_cnt[task] = 0; }
        return;
    }
    const int total = (int)size - 10;
    const int len = total / 6;
    const int s_start = len * sec;
    const int s_end = sec == 5 ? total - 1 : len * (sec + 1) - 1;
    const int m = s_end - s_start;  // the sub-vector excludes element `sector_end`
    if (m > kMaxSector) {
        if (tid == 0) { edge_cnt[task] = 0; surf_cnt[task] = 0; *too_long = 1; }
        return;
    }
    if (m <= 0) {
        if (tid == 0) { edge_cnt[task] = 0; surf_cnt[task] = 0; }
        return;
    }
    int pow2 = 1;
    while (pow2 < m) pow2 <<= 1;
    for (int t = tid; t < pow2; t += kLB) {
        const int id = 5 + s_start + t;  // cloud_curvature[k].id_ = k + 5
        s_val[t] = t < m ? curv[base + id] : __builtin_inf();
        s_id[t] = t < m ? id : 0x7FFFFFFF;
    }
    for (int t = tid; t < m + 16; t += kLB) s_picked[t] = 0;
    __syncthreads();
    // bitonic sort ascending by (value, id)
    for (int k = 2; k <= pow2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = tid; t < pow2; t += kLB) {
                const int x = t ^ j;
                if (x > t) {
                    const double va = s_val[t], vb = s_val[x];
                    const int ia = s_id[t], ib = s_id[x];
                    const bool a_gt_b = va > vb || (va == vb && ia > ib);
                    const bool up = (t & k) == 0;
                    if (a_gt_b == up) { s_val[t] = vb; s_val[x] = va; s_id[t] = ib; s_id[x] = ia; }
                }
            }
            __syncthreads();
        }
    }
    // the pick loop (:100-139), sequential by definition; picked flags are indexed by id − s_start (ids reach 5 beyond either end)
    if (tid == 0) {
        int n_picked = 0, n_edge = 0;
        const float4* R = L + base;
        for (int i = m - 1; i >= 0; --i) {
            const int ind = s_id[i];
            if (s_picked[ind - s_start]) continue;
            if (s_val[i] <= 0.1) break;
            n_picked++;
            s_picked[ind - s_start] = 1;
            if (n_picked <= kMaxEdges) s_edges[n_edge++] = ind;
            else break;
            for (int k = 1; k <= 5; k++) {
                if (gap_too_large(R[ind + k], R[ind + k - 1])) break;
                s_picked[ind + k - s_start] = 1;
            }
            for (int k = -1; k >= -5; k--) {
                if (gap_too_large(R[ind + k], R[ind + k + 1])) break;
                s_picked[ind + k - s_start] = 1;
            }
        }
        s_n_edge = n_edge;
        edge_cnt[task] = (uint32_t)n_edge;
    }
    __syncthreads();
    for (int e = tid; e < s_n_edge; e += kLB) edge_slot[task * kMaxEdges + e] = L[base + s_edges[e]];
    // surface points: unpicked elements in ascending sorted order (:143-149) — ordered compaction, 256 positions per round
    uint32_t running = 0;
    const int lane = tid & 63, wave = tid >> 6;
    for (int t0 = 0; t0 < m; t0 += kLB) {
        const int t = t0 + tid;
        int ind = 0;
        bool keep = false;
        if (t < m) { ind = s_id[t]; keep = !s_picked[ind - s_start]; }
        const unsigned long long bal = __ballot(keep);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(bal);
        __syncthreads();
        uint32_t before = 0, all = 0;
        for (int w = 0; w < kLB / 64; ++w) { before += w < wave ? s_wave[w] : 0u; all += s_wave[w]; }
        if (keep) surf_slot[base + 5 + s_start + running + before + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull))] = L[base + ind];
        running += all;
        __syncthreads();
    }
    if (tid == 0) surf_cnt[task] = running;
}

}  // namespace loam
}  // namespace locgpu
