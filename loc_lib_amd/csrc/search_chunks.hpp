// loc_lib_amd/csrc/search_chunks.hpp — the chunk driver of the candidate searches and of the scores of one cloud under many poses:
// one driver, three matchers (ICP and direct NDT in locgpu_api.hip over the context's shared-source batch, LOAM in loam_align.hip over
// the handle's pair of storage batches). What a chunk IS — which batches take its shape, how it is aligned and scored — is the caller's.
#pragma once
#include <algorithm>
#include <cstddef>

#include "../../include/locgpu.h"

namespace locgpu {

// A chunk holds at most kSearchEntries entries and kSearchBytes of per-entry workspace.
constexpr int kSearchEntries = 256;
constexpr size_t kSearchBytes = (size_t)1 << 30;

// Entries per chunk for m entries of bytes_per_entry workspace each: equal chunks, the last one may be shorter.
inline int search_chunk(size_t bytes_per_entry, int m) {
    const size_t fit = kSearchBytes / std::max<size_t>(bytes_per_entry, 1);
    const int chunk_max = (int)std::min<size_t>(kSearchEntries, std::max<size_t>(fit, 1));
    const int n_chunks = (m + chunk_max - 1) / chunk_max;
    return (m + n_chunks - 1) / n_chunks;
}

// One cloud under n_poses poses: score(off, cnt) scores entries [off, off + cnt).
template <class Score>
int fitness_in_chunks(int n_poses, int chunk, Score score) {
    int rc = LOCGPU_OK;
    for (int off = 0; rc == LOCGPU_OK && off < n_poses; off += chunk) rc = score(off, std::min(chunk, n_poses - off));
    return rc;
}

// The candidate search of every matcher: align_and_score(off, cnt) aligns candidates [off, off + cnt) — summing as the plain batch of
// all m would, so that chunking never shows in a pose — and scores them; then the winner is picked by the rule of locgpu.h over
// out_fit[i * fit_stride]: the lowest score among the candidates with an inlier and the inlier ratio, ties to the lower index.
template <class Chunk>
int init_search_in_chunks(int m, int chunk, double min_inlier_ratio, const locgpu_fitness* out_fit, int fit_stride, int* best, Chunk align_and_score) {
    *best = -1;
    int rc = LOCGPU_OK;
    for (int off = 0; rc == LOCGPU_OK && off < m; off += chunk) rc = align_and_score(off, std::min(chunk, m - off));
    if (rc != LOCGPU_OK) return rc;
    for (int i = 0; i < m; ++i) {
        const locgpu_fitness& f = out_fit[(size_t)i * fit_stride];
        if (f.inliers <= 0 || !((double)f.inliers >= min_inlier_ratio * (double)f.finite_points)) continue;
        if (*best < 0 || f.score < out_fit[(size_t)*best * fit_stride].score) *best = i;  // ties stay with the lower index
    }
    return LOCGPU_OK;
}

}  // namespace locgpu
