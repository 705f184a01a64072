// loc_lib_amd/csrc/launch.hpp — host-callable launchers of the kernels in icp_search.hip / icp_fit.hip / ndt_kernels.hip.
#pragma once
#include "gn_post.hpp"
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "device_math.hpp"

namespace locgpu {

struct GnParams;

struct SearchArgs {
    const uint2* tree;
    size_t tree_bytes;
    int depth;
    const float4* src;
    const int* counts;
    const PoseState* st;
    uint32_t* nn;
    size_t nn_pitch;
    int max_n, n_scans, k;
    float alpha_eff;
    int skip_nonfinite;
    unsigned long long* visit_totals;  // null unless visit counting is on
    uint32_t* redo_list;               // [n_scans*max_n] queries the fast kernel hands to the exact kernel
    unsigned int* redo_count;
    uint32_t* redo_list2;              // grid mode: first pass → second pass
    unsigned int* redo_count2;
    unsigned long long* search_stats;  // [2] cumulative: queries searched, queries redone exactly (may be null)
    // Later chunks of an alignment: the indices of the scans still open (device array) and their number. The hot search kernel and
    // the accumulate kernels then run grid.y = n_active instead of n_scans blocks of early exits (a 256-scan step's last eight
    // iterations hold a handful of scans: 460 k empty workgroups cost ≈96 µs per launch). nullptr = every scan.
    const int* active = nullptr;
    int n_active = 0;
    // Scan pools: the points of scan slot s are region src_of[s] of `src` (an arena of max_n-point regions); nullptr = region s.
    const int* src_of = nullptr;
    // instrumented pass only: bitmap over the tree's 8-byte slots (one bit each, zeroed by the caller, counted and cleared again
    // by launch_count_touched) — which slots this search launch reads at all
    uint32_t* touched = nullptr;
    // Optional, k = 5: [n_scans][ceil(max_n / 64)] words, one per 64-lane walk wave — bit `lane` set: the query's neighbour set is not
    // known to be the previous lane's (a leader of the plane fit, AccumArgs::run_flags); nullptr = the walk kernel does nothing new.
    unsigned long long* run_flags = nullptr;
    // Forest target (locgpu_icp_set_target_forest): [n_scans] first slot of the tree scan s is searched in — the walk runs on
    // tree + scan_tree_base[s] and every slot written to nn is absolute. nullptr = one tree for all scans, at slot 0.
    const uint32_t* scan_tree_base = nullptr;
};

struct AccumArgs {
    const uint2* tree;
    const float4* src;
    const int* counts;
    const PoseState* st;
    const uint32_t* nn;
    size_t nn_pitch;
    int max_n, n_scans;
    double gate;        // max_plane / max_line / max_nn distance
    double* partials;   // [n_scans][blocks_per_scan][kAccW]
    const int* active = nullptr;  // see SearchArgs
    int n_active = 0;
    const int* src_of = nullptr;  // see SearchArgs
    // > 0: split the sums as a plain batch of this many scans would (a scan pool of many slots serving jobs of that size), so that
    // a pooled scan's partial sums — hence its pose — are the plain batch's bit for bit. 0: by n_scans.
    int split_scans = 0;
    // LOCGPU_P2PLANE_MAP: the plane table of the target (map_planes.hip), one 32-byte row of four doubles per slot >> 1
    const double* planes = nullptr;
    // LOCGPU_P2PLANE, optional: the run flags the search launch just before this one on the same batch reported it wrote
    // (SearchArgs::run_flags); nullptr = the plane kernel finds the runs itself from the lists.
    const unsigned long long* run_flags = nullptr;
};

// wrote_run_flags (optional): whether the route taken wrote a.run_flags — the 64-lane walk kernel does; the 16-lane one-scan kernel,
// the exact kernel and every other search launcher do not
bool launch_icp_search(const SearchArgs& a, hipStream_t s, bool* wrote_run_flags = nullptr);
// icp_search_pairs.hip: the route launch_icp_search takes when a.scan_tree_base is set — the one-thread-per-query exact traversal, once
// per scan's own tree; no work lists, no run flags, no visit counts
bool launch_icp_search_pairs(const SearchArgs& a, hipStream_t s);
// exact tree traversal over a.redo_list only (the list is filled by a preceding fast / grid kernel)
bool launch_icp_search_redo(const SearchArgs& a, hipStream_t s);
// the walk traversal with every level stored (a.alpha_eff) over the queries in `list`, then the exact redo kernel for its ties
bool launch_icp_search_list(const SearchArgs& a, const uint32_t* list, const unsigned int* n_list, hipStream_t s);
bool launch_knn_query(const uint2* tree, int depth, const float* q, size_t nq, int k, float alpha_eff, int32_t* out, uint32_t* visits,
                      hipStream_t s);
// returns the number of partial blocks per scan the kernel wrote (what gn_solve must sum)
int launch_icp_accum(int method, const AccumArgs& a, hipStream_t s);
// list_counts (optional): the two search work-list counters, zeroed for the next iteration
// scans (optional): n_scans indices — block i solves scan scans[i] instead of scan i
// post (optional, one scan): the solve also writes an iteration word — and, once the scan is done, its result — to pinned host memory
void launch_gn_solve(const double* partials, int blocks_per_scan, PoseState* st, int n_scans, const GnParams& prm, int do_update, double* hb_out,
                     unsigned int* list_counts, hipStream_t s, const int* scans = nullptr, const GnPost* post = nullptr);
// The joint solve of the LOAM matcher (loam_registration.cpp:47-90; loam_align.hip): class 0 = surface, 1 = edge. One block per scan
// sums the surface batch's partials, then the edge batch's (each with its own blocks_per_scan, in gn_solve's fixed order), tests each
// class as IcpRegistration::CaculateMatrixHAndB does (icp_registration.cpp:204-211), solves the SUM and updates the one PoseState
// both classes' local stages read. partials[c] == nullptr: the class is switched off. hb_out (optional): kLoamHbW doubles per scan =
// H (36, row-major) and B (6) of the sum, effective_num[2], ok[2]. list_counts[c]: the class batch's search work-list counters, zeroed.
constexpr int kLoamHbW = 46;
struct LoamSolveArgs {
    const double* partials[2];
    int blocks_per_scan[2];
    int min_effective_pts[2];
    unsigned int* list_counts[2];
    int max_iteration;
    double eps;
    PoseState* st;
    int do_update;
    double* hb_out;
    const int* scans;  // optional: n_scans indices — block i solves scan scans[i]
};
void launch_loam_solve(const LoamSolveArgs& a, int n_scans, hipStream_t s);
int icp_accum_split(int method, int max_n, int n_scans);  // points per thread of the accumulate kernels (the split of the partial sums)
// Sharded batches: acc[g][0..28) = sum of the block partials of global scan g when this rank holds it (local index g - first),
// zeros otherwise — in exactly the order gn_solve_kernel sums them, so that all-reduce(acc) followed by gn_solve on acc
// (blocks_per_scan = 1) gives bit for bit the single-GPU result.
// owned (optional, scan pools): per global scan, whether this rank holds its points (then first = 0, n_local = n_total)
void launch_sum_partials(const double* partials, int blocks_per_scan, const PoseState* st_all, int first, int n_local, int n_total, double* acc,
                         hipStream_t s, const unsigned char* owned = nullptr);
// Fitness score (fitness.hip): after a k = 1 exact search stage has filled `nn`, per scan {Σd² over the inliers, inliers, finite
// points, 0} → out[scan][kFitW]. partials: room for n_scans × icp_fitness_rows(max_n) × kFitW doubles. gate2 = (float)max_range².
constexpr int kFitW = 4;
struct FitnessArgs {
    const uint2* tree;
    const float4* src;
    const int* counts;
    const PoseState* st;
    const uint32_t* nn;
    int max_n, n_scans;
    float gate2;
    double* partials;
    double* out;
    unsigned int* list_counts;    // the search stage's work-list counters, zeroed behind it (may be null)
    const int* src_of = nullptr;  // see SearchArgs
};
int icp_fitness_rows(int max_n);
void launch_icp_fitness(const FitnessArgs& a, hipStream_t s);
// Its first half alone: the block rows of every scan → a.partials (a.out and a.list_counts are not read). Returns the rows per scan.
int launch_icp_fitness_accum(const FitnessArgs& a, hipStream_t s);
// The joint score of the LOAM matcher (fitness.hip): class 0 = surface, 1 = edge; partials[c] with rows[c] rows per candidate as
// launch_icp_fitness_accum left them in the class's batch (nullptr: the class is switched off). out[n_cands][3][kFitW]: joint, surface,
// edge, each {Σd², inliers, finite points, 0}. list_counts[c] (optional): the class batch's search work-list counters, zeroed.
void launch_loam_fitness_sum(const double* const partials[2], const int rows[2], int n_cands, double* out, unsigned int* const list_counts[2], hipStream_t s);
// The last step of a score, shared with the NDT score (ndt_fitness.hip): adds the `rows` block rows {Σ, inliers, finite points, ·} of
// every scan in a fixed order → out[scan][kFitW]. list_counts (optional): the search stage's work-list counters, zeroed.
void launch_fitness_sum(const double* partials, int rows, int n_scans, double* out, unsigned int* list_counts, hipStream_t s);
struct M12f { float v[12]; };  // rows of pose.matrix().cast<float>() (icp_registration.cpp:241), a kernel argument
void launch_transform_cloud(const float4* src, size_t n, const M12f& m12, float* dst_xyz, hipStream_t s);
// loam_stream.hip: edge points then surface points under m12 into out (n_edge + n_surf float4, w carried through); out overlaps neither
void launch_loam_join_transform(const float4* edge, size_t n_edge, const float4* surf, size_t n_surf, const M12f& m12, float4* out, hipStream_t s);
// Plane table of LOCGPU_P2PLANE_MAP (map_planes.hip). queries: the coordinates of leaves [first, first + n) as the source points of a
// one-scan search batch (counts[0] = n). fit: the chunk's k = 5 lists → rows planes[slot >> 1], *n_valid += valid planes.
// dump: rows by original point index into zeroed out_n4 [n_points][4] / out_valid [n_points].
void launch_map_plane_queries(const uint2* tree, const uint32_t* leaf_slots, size_t first, int n, float4* src, int* counts, hipStream_t s);
void launch_map_plane_fit(const uint2* tree, const uint32_t* leaf_slots, size_t first, int n, const uint32_t* nn, size_t nn_pitch, double* planes,
                          unsigned long long* n_valid, hipStream_t s);
void launch_map_plane_dump(const uint2* tree, const uint32_t* leaf_slots, size_t n_leaves, const double* planes, size_t n_points, double* out_n4,
                           unsigned char* out_valid, hipStream_t s);
// Code-object self-test (once per process): no walk kernel owns static LDS, so every traversal stack starts at LDS address 0 —
// the precondition of search_walk.hpp's out-of-range rows (tests/test_gpu_lds_semantics.py pins the hardware side).
bool search_kernels_lds_ok();
// LOCGPU_STAMP is set and non-zero (read once): the diagnostic build of the walk kernel — per-query round counts behind the redo list
// (twice its size), other meanings of locgpu_search_stats_read's out[2..3], locgpu_debug_stamp_trips
bool stamp_build();
// instrumented pass: totals[3] += number of set bits of touched[0..n_words), then touched := 0
void launch_count_touched(uint32_t* touched, size_t n_words, unsigned long long* totals, hipStream_t s);
// test hook: slot lists [k][pitch] → original point indices out[query * k + j] (-1 = none, and every row past its scan's count)
void launch_nn_to_index(const uint2* tree, size_t tree_slots, const uint32_t* nn, size_t nn_pitch, const int* counts, int max_n, size_t n_queries, int k,
                        int32_t* out, hipStream_t s);

}  // namespace locgpu
