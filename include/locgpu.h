/* include/locgpu.h — C ABI of the MI355X-native registration hot path (liblocgpu.so).
 *
 * This is the drop-in boundary for the ONE path of maotian123/loc_lib this project accelerates:
 * the KD-tree neighbour search + point-to-plane/-line/-point ICP and direct-NDT Gauss–Newton loop
 * that slam_demo's front-ends run once per scan through LocUtils::MatchingInterface. The reference
 * is plain C++ with no FFI; a maintainer binds these entry points from the reference's own matcher
 * classes (see INTEGRATION.md and loc_lib_amd/host/). Every entry point names the reference interface it
 * replaces (paths relative to the reference repo root).
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch/Eigen/PCL types cross this boundary;
 *   - clouds are passed as (base pointer, point count, stride in BYTES); x,y,z are three consecutive
 *     float32 at the start of each point (pcl::PointXYZI: stride 32; packed xyz: stride 12);
 *   - poses are 7 doubles, quaternion (x,y,z,w) then translation (x,y,z): the memory layout of
 *     Sophus::SE3d::data() (LocUtils/include/LocUtils/common/eigen_types.h:66, `using SE3 = Sophus::SE3d`);
 *   - host-pointer entry points copy their inputs before returning (the reference deep-copies target
 *     and source: icp_registration.cpp:16,259), are synchronous, and are not re-entrant per context
 *     (the reference matcher is single-threaded per instance);
 *   - every function returns LOCGPU_OK (0) or a negative locgpu_status; no exception crosses the boundary.
 *     locgpu_last_error() gives the text. There is NO CPU fallback: without a HIP device every call fails.
 */
#ifndef LOCGPU_H_
#define LOCGPU_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define LOCGPU_API __attribute__((visibility("default")))

typedef struct locgpu_ctx locgpu_ctx;     /* one matcher instance (tree / voxel grid + workspaces) on one GPU */
typedef struct locgpu_batch locgpu_batch; /* a batch of scans resident in HBM */

typedef enum locgpu_status {
    LOCGPU_OK = 0,
    LOCGPU_ERR_INVALID = -1,    /* bad argument */
    LOCGPU_ERR_NO_DEVICE = -2,  /* no HIP device / HIP runtime error */
    LOCGPU_ERR_NO_TARGET = -3,  /* align/search before set_target */
    LOCGPU_ERR_K_TOO_LARGE = -4,/* k > number of tree leaves (kdtree.cpp:149-153 logs an error and returns false) */
    LOCGPU_ERR_DEPTH = -5,      /* tree deeper than the traversal stack supports */
    LOCGPU_ERR_OOM = -6
} locgpu_status;

/* IcpMethod, LocUtils/include/LocUtils/model/matching/3d/icp/icp_registration.hpp:15-20 (PCLICP is not on the path). */
typedef enum locgpu_icp_method {
    LOCGPU_P2P = 0,
    LOCGPU_P2LINE = 1,
    LOCGPU_P2PLANE = 2,
    /* A labelled FAST MODE with no reference counterpart, never the source of a parity claim (see locgpu_icp_build_map_planes):
     * point-to-plane against the plane fitted ONCE per map point at ingest, looked up at the 1-nearest leaf, instead of the
     * reference's math::FitPlane per query and iteration (math_utils.h:112-136, icp_registration.cpp:161-213). Not the default.
     * (3 and 4 are taken inside the library by the NDT variants of the Gauss-Newton solve.) */
    LOCGPU_P2PLANE_MAP = 5
} locgpu_icp_method;

/* How correspondences are searched.
 * TREE_FAITHFUL replays the reference's mean-split KD-tree and its DFS visit order bit for bit
 * (kdtree.cpp:169-236), including the alpha-pruned approximate mode that is the reference default
 * (kdtree.h:128-129). GRID_EXACT is the exact k-NN over a radix-sorted voxel grid: it equals the
 * reference with KdtreeRegistration::SetEnableANN(false) (kdtree.cpp:285-288) up to ties in distance. */
typedef enum locgpu_search_mode { LOCGPU_SEARCH_TREE_FAITHFUL = 0, LOCGPU_SEARCH_GRID_EXACT = 1 } locgpu_search_mode;

/* IcpOptions, icp_registration.hpp:22-39 (same defaults via locgpu_icp_opts_default). */
typedef struct locgpu_icp_opts {
    int32_t method;            /* locgpu_icp_method; reference default P2P */
    int32_t max_iteration;     /* 20 */
    double max_nn_distance;    /* 1.0  (compared with a SQUARED distance, icp cpp:75) */
    double max_plane_distance; /* 0.1 */
    double max_line_distance;  /* 0.5 */
    int32_t min_effective_pts; /* 10 */
    double eps;                /* 1e-2 */
    int32_t approximate;       /* 1: KdTree::approximate_ (kdtree.h:128) */
    float ann_alpha;           /* 0.1f: KdTree::alpha_ (kdtree.h:129) */
    int32_t search_mode;       /* locgpu_search_mode */
} locgpu_icp_opts;

/* NdtOptions, LocUtils/include/LocUtils/model/matching/3d/ndt/ndt_registration.hpp:27-42. */
typedef struct locgpu_ndt_opts {
    int32_t max_iteration;     /* 20 */
    double voxel_size;         /* 1.0; inv_voxel_size_ is always recomputed as 1/voxel_size (ndt cpp:15,25) */
    int32_t min_effective_pts; /* 10 */
    int32_t min_pts_in_voxel;  /* 3 (a voxel is kept iff count > this) */
    double eps;                /* 1e-2 */
    double res_outlier_th;     /* 20.0 */
    int32_t nearby_type;       /* 0 CENTER, 1 NEARBY6 (hpp:16-20) */
    int32_t method;            /* 1 DIRECT_NDT (default), 2 INCREMENTAL_NDT (NdtMethod, hpp:21-26; 0 PCL_NDT is a no-op in the reference) */
    int64_t capacity;          /* 100000: LRU voxel capacity of the incremental variant (capacity_, hpp:37) */
} locgpu_ndt_opts;

/* Per-scan result counters (the reference only logs these through glog). */
typedef struct locgpu_align_stats {
    int32_t iterations;        /* Gauss–Newton iterations executed (H,B evaluations) */
    int32_t converged;         /* 1 if the loop left through |dx| < eps */
    int32_t status;            /* 0 ok; 1 direct-NDT det(H)==0 ⇒ reference returns before writing result_pose (ndt cpp:435-436);
                                  2 incremental NDT: too few effective residuals ⇒ returns false with the current pose (ndt cpp:349-353);
                                  locgpu_loam_* only: 3 the SURFACE class's evaluation reported false, 4 the EDGE class's did ⇒
                                  ScanMatch returns false before writing result_pose (loam_registration.cpp:56-70); surface is tested first;
                                  locgpu_icp_align_pairs / locgpu_ndt_align_pairs only: 5 (LOCGPU_STATUS_NO_PAIR_TARGET) the scan was given no target and was not aligned */
    int32_t reserved;
    int64_t last_effective_num;
    double last_dx_norm;
} locgpu_align_stats;

LOCGPU_API void locgpu_icp_opts_default(locgpu_icp_opts* o);
LOCGPU_API void locgpu_ndt_opts_default(locgpu_ndt_opts* o);

/* Lifetime. A context is what one IcpRegistration / NdtRegistration instance owns (icp_registration.hpp:41-142). */
LOCGPU_API int locgpu_create(int device_id, locgpu_ctx** out);
LOCGPU_API void locgpu_destroy(locgpu_ctx* ctx);
LOCGPU_API const char* locgpu_last_error(const locgpu_ctx* ctx); /* ctx may be NULL: error of the last failed create */
LOCGPU_API int locgpu_device_count(void);

/* ---- ICP target: IcpRegistration::SetInputTarget (icp_registration.cpp:9-29) →
 *      KdtreeRegistration::SetTargetCloud / KdTree::BuildTree (kdtree.cpp:261-270, 10-31). Host pointer. */
LOCGPU_API int locgpu_icp_set_target(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes);
/* The same with the host tree build on a worker thread: returns once the points have been copied (the deep copy the reference makes,
 * icp_registration.cpp:16); the first entry point that reads the ICP target completes the ingest on the caller's thread and reports
 * its errors. See locgpu_icp_set_target_cloud_async. */
LOCGPU_API int locgpu_icp_set_target_async(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes);
/* out[0]=leaves (KdTree::size_), out[1]=tree nodes, out[2]=depth, out[3]=bytes of the packed tree in HBM */
LOCGPU_API int locgpu_icp_target_info(const locgpu_ctx* ctx, int64_t out[4]);

/* ---- Map planes: the per-map-point plane table behind LOCGPU_P2PLANE_MAP (no reference counterpart). It stands in
 * for the math::FitPlane call (math_utils.h:112-136) that IcpRegistration::CaculateMatrixHAndBP2Plane (icp_registration.cpp:161-213)
 * makes per source point and iteration. For every leaf of the target's KD-tree: its five EXACT nearest leaves (itself included; the
 * walk of KdTree::GetClosestPoint with approximate_ = false) in FP64 -> FitPlane -> the FP64 4-vector n4 (the normal is not unit, as in
 * the reference), valid iff all five (n3·p + d)² <= 1e-2; a tree of fewer than five leaves has no valid plane. One evaluation of
 * H, B with the method: for every finite source point q, qs = pose·q in FP64, the 1-nearest leaf of (float)qs under the caller's
 * approximate / ann_alpha / search_mode; no neighbour or no valid plane there: skipped; otherwise effective_num++, dis = n3·qs + n4[3],
 * skipped if |dis| > max_plane_distance, else J = [-n3ᵀ·R·hat(q), n3ᵀ], H += JᵀJ, B += -Jᵀ·dis; update, `ok` and stop rule are
 * AlignP2Plane's (icp_registration.cpp:345-381). The method is accepted by locgpu_icp_hb / _align / _scan_match / _align_cloud,
 * locgpu_icp_align_batch / _begin / _end, locgpu_icp_hb_batch, shared-source batches and locgpu_icp_init_search, eager and hipGraph,
 * tree and grid search; locgpu_gn_update takes it as P2PLANE. Scan pools (locgpu_pool_create) and sharded batches
 * (locgpu_batch_create_sharded) return LOCGPU_ERR_INVALID for it.
 * build: estimates the table for the current ICP target on the device (completing an asynchronous ingest first); idempotent; any
 * locgpu_icp_set_target* drops the table, and the first use of the method without one builds it. 32 B per row, about 1.5 rows per
 * map point; the table and a workspace for chunks of 2^20 leaves stay with the context, grow-only. */
LOCGPU_API int locgpu_icp_build_map_planes(locgpu_ctx* ctx);
/* math::FitPlane results held for the target (math_utils.h:112-136; icp_registration.cpp:161-213 reads them through the method above):
 * out[0] = leaves with a plane row, out[1] = valid planes, out[2] = bytes of the table in HBM. All zero when no table is built.
 * Like locgpu_icp_target_info it completes a pending asynchronous ingest (the context is const in name only). */
LOCGPU_API int locgpu_icp_map_planes_info(const locgpu_ctx* ctx, int64_t out[3]);
/* Debug / test read-back (like locgpu_ndt_dump) of the math::FitPlane rows (math_utils.h:112-136) the method reads in place of
 * icp_registration.cpp:161-213's own fit: rows indexed by ORIGINAL point index, n4: cap × 4 doubles, valid: cap bytes; a point that is
 * no leaf of the tree (dropped by the degenerate-split rule) is reported invalid with a zero row. Builds the table if there is none.
 * *n_out = number of target points; LOCGPU_ERR_INVALID when cap is smaller. n4 = valid = NULL with cap = 0 is a size query: it
 * only sets *n_out and returns LOCGPU_OK. */
LOCGPU_API int locgpu_icp_map_planes_dump(locgpu_ctx* ctx, double* n4, uint8_t* valid, size_t cap, size_t* n_out);

/* ---- SearchPointInterface::FindNearstPoints (search_point_interface.h:13; kdtree.cpp:272-283), many queries at once.
 * queries: nq × 3 packed float32 (host). out_idx: nq × k int32 original point indices, ascending distance (host).
 * visits (optional, host): nq × 2 uint32 {tree nodes visited, leaves visited} per query. */
LOCGPU_API int locgpu_knn(locgpu_ctx* ctx, const float* queries, size_t nq, int k, int approximate, float alpha, int search_mode,
                          int32_t* out_idx, uint32_t* visits);

/* ---- BfnnRegistration (LocUtils/include/LocUtils/model/search_point/bfnn/bfnn.h:11-37, bfnn.cpp:14-50): the brute-force
 * implementation of SearchPointInterface. set_target = SetTargetCloud (deep copy; false/-1 for an empty cloud); knn = FindNearstPoints
 * for nq queries at once: out_idx nq × k original point indices in ascending float32 distance. Equal distances — an order the
 * reference's std::sort leaves open — are ordered by index. k > cloud size is an error here (the reference reads past the end). */
LOCGPU_API int locgpu_bfnn_set_target(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes);
LOCGPU_API int locgpu_bfnn_knn(locgpu_ctx* ctx, const float* queries, size_t nq, int k, int32_t* out_idx);

/* ---- MatchingInterface::CaculateMatrixHAndB (matching_interface.h:18-24; icp_registration.cpp:31-55): one
 * evaluation of H (6×6 row-major) and B at `pose`. *ok receives the reference's bool (false: too few effective
 * points or det(H)==0). Used by LoamRegistration (loam_registration.cpp:56,66). */
LOCGPU_API int locgpu_icp_hb(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double pose[7],
                             const locgpu_icp_opts* opts, double H[36], double B[6], int64_t* effective_num, int* ok);

/* ---- IcpRegistration::ScanMatch minus the output cloud (icp_registration.cpp:216-239 → AlignP2P/P2Line/P2Plane :267-381). */
LOCGPU_API int locgpu_icp_align(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double init_pose[7],
                                const locgpu_icp_opts* opts, double out_pose[7], locgpu_align_stats* stats);

/* ---- IcpRegistration::ScanMatch WHOLE (icp_registration.cpp:216-244): the alignment and the output cloud
 * `pcl::transformPointCloud(*input_source, *result_cloud_ptr, result_pose.matrix().cast<float>())` (:241) in one call — the source is
 * uploaded once, the transform runs on the copy that is in HBM from the alignment, and x, y, z come back through pinned staging.
 * The output cloud: n points of out_stride_bytes each, given either as out_cloud or by out_fn — a callback the library calls ONCE, on a
 * helper thread, while the alignment runs, with out_user and the point count; it returns the output array (the façade sizes the caller's
 * pcl::PointCloud there: the first touch of a fresh 3.7 MB array is then off the caller's thread) or NULL for none. Both NULL: no
 * output cloud. Like pcl::transformPointCloud every output point is the source point with x, y, z replaced: unless the output array
 * IS the source array (same stride: in place) the first min(stride_bytes, out_stride_bytes) bytes of every source point are copied
 * — on the helper thread, beside the alignment. Any other overlap of the two clouds is undefined. out_stride_bytes | LOCGPU_OUT_FIELDS_DONE:
 * the output points already hold their other fields (or the callback puts them there — the façade's does `out->points = src->points`,
 * one pass over fresh memory instead of a resize and a copy): the library then only writes x, y, z. The callback must not call into
 * this context. This is what LocUtils::IcpRegistration::ScanMatch binds to. */
typedef void* (*locgpu_out_cloud_fn)(void* user, size_t n_points);
#define LOCGPU_OUT_FIELDS_DONE ((size_t)1 << (sizeof(size_t) * 8 - 1))
LOCGPU_API int locgpu_icp_scan_match(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double init_pose[7],
                                     const locgpu_icp_opts* opts, double out_pose[7], locgpu_align_stats* stats, void* out_cloud,
                                     size_t out_stride_bytes, locgpu_out_cloud_fn out_fn, void* out_user);
/* ---- NdtRegistration::ScanMatch WHOLE (ndt_registration.cpp:238-261). result_pose is IN-OUT like the reference's `SE3& result_pose`:
 * with stats->status == 1 (det(H) == 0) AlignNdt returns before it assigns it (:435-436), so the caller's value stays and the output
 * cloud is transformed by that value (:258); otherwise it receives the result. Output cloud as above. */
LOCGPU_API int locgpu_ndt_scan_match(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double init_pose[7],
                                     double result_pose[7], locgpu_align_stats* stats, void* out_cloud, size_t out_stride_bytes,
                                     locgpu_out_cloud_fn out_fn, void* out_user);

/* ---- pcl::transformPointCloud(*src, *out, pose.matrix().cast<float>()) (icp_registration.cpp:241, ndt_registration.cpp:258).
 * Writes x,y,z of each output point (float32 arithmetic); other fields of the output points are left untouched. */
LOCGPU_API int locgpu_transform_cloud(locgpu_ctx* ctx, const double pose[7], const void* src, size_t n, size_t src_stride_bytes,
                                      void* out, size_t out_stride_bytes);

/* ---- Batched many-scans-vs-one-map mode (BASELINE.json config 4; no reference counterpart — the reference loops
 * ScanMatch over scans). Scans are uploaded once and stay resident; each align call runs every scan's own GN loop. */
LOCGPU_API int locgpu_batch_create(locgpu_ctx* ctx, const void* const* srcs, const size_t* counts, size_t stride_bytes, int n_scans,
                                   locgpu_batch** out);
LOCGPU_API void locgpu_batch_destroy(locgpu_batch* b);
/* The source deep copy of ScanMatch (SetSource, icp_registration.cpp:221,252-265) for a whole batch, overlapped with the GPU's work:
 * locgpu_batch_create_empty reserves room for n_scans scans of at most max_points_per_scan points; locgpu_batch_upload_async
 * replaces the batch's scans (counts[s] <= max_points_per_scan) and returns at once — a worker packs the strided host points
 * into pinned slots and streams them to HBM on the context's copy stream, under whatever its compute streams
 * are running (e.g. the align call of ANOTHER batch: two batches alternate as a double buffer; one upload per context at a
 * time — a second one waits for the first one's packing). The host clouds must stay valid
 * until locgpu_batch_upload_wait returns (it returns the upload's status); every align / hb call on the batch waits for its
 * pending upload first. An upload into a batch whose alignment has been begun and not ended (locgpu_*_align_batch_begin) is
 * refused with LOCGPU_ERR_INVALID — rotate one more batch than there are alignments in flight. A failed upload stays with its
 * batch: that batch's next align / hb / upload_wait returns the failure until a new upload replaces its scans. */
LOCGPU_API int locgpu_batch_create_empty(locgpu_ctx* ctx, int n_scans, size_t max_points_per_scan, locgpu_batch** out);
LOCGPU_API int locgpu_batch_upload_async(locgpu_batch* b, const void* const* srcs, const size_t* counts, size_t stride_bytes);
LOCGPU_API int locgpu_batch_upload_wait(locgpu_batch* b);
/* init_poses / out_poses: n_scans × 7 doubles (host). stats: n_scans entries or NULL. */
LOCGPU_API int locgpu_icp_align_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* init_poses, const locgpu_icp_opts* opts,
                                      double* out_poses, locgpu_align_stats* stats);
LOCGPU_API int locgpu_ndt_align_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* init_poses, double* out_poses,
                                      locgpu_align_stats* stats);
/* The same alignments in two halves, for a caller that keeps several batches in flight — up to three pay — (no reference counterpart: the reference
 * matches one scan at a time). A context has three compute streams; *_begin gives the alignment one of its own — the batch's while no
 * other alignment in flight is on it, else the least-loaded one, so a caller may rotate more batches than streams — copies the poses,
 * enqueues the first eight Gauss–Newton iterations on that stream and returns, locgpu_align_batch_end waits for them,
 * enqueues further iterations while scans are still open and writes the results. Begun on batch B while batch A is not yet
 * ended, B's first iterations fill the chip under A's last ones (which hold a handful of unconverged scans):
 *     begin(A); loop { begin(B); end(A); swap(A, B); }
 * One alignment per batch at a time and no locgpu_batch_upload_async into the batch between begin and end (LOCGPU_ERR_INVALID);
 * results are those of the blocking calls, bit for bit. The target must not change between begin and end. Sharded batches: every rank begins and ends its batches in the same order. */
LOCGPU_API int locgpu_icp_align_batch_begin(locgpu_ctx* ctx, locgpu_batch* b, const double* init_poses, const locgpu_icp_opts* opts);
LOCGPU_API int locgpu_ndt_align_batch_begin(locgpu_ctx* ctx, locgpu_batch* b, const double* init_poses);
LOCGPU_API int locgpu_align_batch_end(locgpu_ctx* ctx, locgpu_batch* b, double* out_poses, locgpu_align_stats* stats);
/* One H,B evaluation for every scan of the batch at the given poses (point-sharded multi-GPU mode: the caller
 * all-reduces hb over ranks, then calls locgpu_gn_update). hb: n_scans × 44 doubles = H36, B6, effective_num, ok. */
LOCGPU_API int locgpu_icp_hb_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, const locgpu_icp_opts* opts, double* hb);
/* The update step of AlignP2Plane (icp_registration.cpp:362-375) on already-reduced normal equations:
 * returns 1 in *stop when |dx| < eps. method selects the P2P "/16" quirk (icp cpp:287). */
LOCGPU_API int locgpu_gn_update(const double hb[44], int method, int min_effective_pts, double eps, double pose[7], double dx[6],
                                int* applied, int* stop);

/* ---- LoamRegistration (LocUtils/include/LocUtils/model/matching/3d/loam/loam_registration.hpp:22-60, loam_registration.cpp:9-104), the
 * matcher slam_demo selects with `matching_method: 0` and Lio::AddCloud(FullCloudPtr) feeds from the feature picker
 * (locgpu_cloud_loam_extract). A locgpu_loam owns what one LoamRegistration owns — a surface matcher (P2Plane) and an edge matcher
 * (P2Line), here two contexts on one GPU — and runs the WHOLE Gauss–Newton loop of ScanMatch (:47-90) on the device: per iteration both
 * classes' search and fit stages and one joint solve on one stream, the stop test on the device, the host reading the flags every
 * 8 (then 4) iterations. Per iteration: surface, then edge, evaluated at the same pose; a class is false iff its effective_num <
 * min_effective_pts or its own det(H) == 0 (icp_registration.cpp:204-211), and a false class ends the alignment (:56-70); otherwise
 * dx = (H_surf + H_edge)⁻¹ (B_surf + B_edge) with no effective-count test on the sum (:76-79), pose.so3() *= exp(dx.head<3>()),
 * translation += dx.tail<3>() (:82-83), stop after the update when |dx| < eps (:85). det(H_surf + H_edge) == 0, where the reference
 * divides by zero, is an iteration without an update (what locgpu_gn_update does); the loop goes on.
 * Limits: the LOAM entry points run EAGER chunks only — locgpu_graph_enable (hipGraph), sharded batches, scan pools and the host-paced
 * one-scan path do not apply to them — LOCGPU_P2PLANE_MAP (map planes) is refused (LOCGPU_ERR_INVALID). Resident forms (declared with
 * the resident clouds below): the single-scan calls (locgpu_loam_set_target_cloud, locgpu_loam_scan_match_cloud,
 * locgpu_loam_fitness_resident, locgpu_loam_submap_*) and the SHARED-SOURCE batched form — one pair of scans under many poses
 * (locgpu_loam_fitness_cloud, locgpu_loam_init_search_cloud); the calls of this block take no batched resident form of n DIFFERENT scans:
 * locgpu_loam_align_batches, declared with the batch front-end below, does. Calls on a
 * handle follow the context's rule: one caller thread, synchronous, host inputs copied before the call returns. */
typedef struct locgpu_loam locgpu_loam;
/* LoamOption, loam_registration.hpp:22-36. Inside surf / edge only method, the three gates, min_effective_pts, approximate / ann_alpha
 * and search_mode are read: their max_iteration and eps are NOT (the loop is LoamRegistration's own, :47,85). */
typedef struct locgpu_loam_opts {
    locgpu_icp_opts surf;      /* surf_icp_option_{IcpMethod::P2PLANE} */
    locgpu_icp_opts edge;      /* edge_icp_option_{IcpMethod::P2LINE}  */
    int32_t use_surf_points;   /* 1 */
    int32_t use_edge_points;   /* 1 */
    int32_t max_iteration;     /* 20 */
    double eps;                /* 1e-3 */
} locgpu_loam_opts;
LOCGPU_API void locgpu_loam_opts_default(locgpu_loam_opts* o);
/* LoamRegistration::LoamRegistration(LoamOption) (loam_registration.cpp:15-20). The options are checked before any device is touched:
 * LOCGPU_ERR_INVALID for NULL opts, both classes switched off, LOCGPU_P2PLANE_MAP or an unknown method / search mode in an enabled class.
 * A context is created for every enabled class. locgpu_loam_last_error(NULL) gives the text of a failed create. */
LOCGPU_API int locgpu_loam_create(int device_id, const locgpu_loam_opts* opts, locgpu_loam** out);
/* The same matcher over two EXISTING ICP contexts on one GPU — what a caller that already holds an edge and a surface context with
 * their targets (the façade's LoamRegistration) needs for the score and the search below. The handle borrows the contexts, their
 * targets and their options' workspaces: it creates none, locgpu_loam_destroy leaves them alive, and whether a class has a target is
 * asked of its context at every call (LOCGPU_ERR_NO_TARGET while it has none), so a later locgpu_icp_set_target on the context is
 * seen. A switched-off class's context may be NULL. The contexts' owner must not use them during a call on the handle and must
 * destroy the handle first. LOCGPU_ERR_INVALID — before any device is touched — for NULL opts, the refusals of locgpu_loam_create,
 * a NULL context of an enabled class, one context given twice, or contexts on different GPUs. */
LOCGPU_API int locgpu_loam_create_on(locgpu_ctx* surf_ctx, locgpu_ctx* edge_ctx, const locgpu_loam_opts* opts, locgpu_loam** out);
LOCGPU_API void locgpu_loam_destroy(locgpu_loam* l);
LOCGPU_API const char* locgpu_loam_last_error(const locgpu_loam* l);
/* LoamRegistration::SetInputTarget (loam_registration.cpp:22-36): IcpRegistration::SetInputTarget of every ENABLED class (a class that
 * is switched off is not ingested; its pointer may be NULL). LOCGPU_OK only if every enabled class was ingested; a class that failed
 * has no target afterwards (LOCGPU_ERR_NO_TARGET from the calls below). */
LOCGPU_API int locgpu_loam_set_target(locgpu_loam* l, const void* edge_pts, size_t n_edge, const void* surf_pts, size_t n_surf, size_t stride_bytes);
/* One evaluation of H = H_surf + H_edge (6×6 row-major), B = B_surf + B_edge at `pose`, no update (loam_registration.cpp:53-77, each
 * term IcpRegistration::CaculateMatrixHAndB, icp_registration.cpp:31-55). eff[2] / ok[2] (optional): each class's effective_num and
 * the reference's bool, index 0 = surface, 1 = edge; a class that is switched off adds nothing and reports 0 / 1. The test hook of
 * the joint reduction. */
LOCGPU_API int locgpu_loam_hb(locgpu_loam* l, const void* edge, size_t n_edge, const void* surf, size_t n_surf, size_t stride_bytes,
                              const double pose[7], double H[36], double B[6], int64_t eff[2], int32_t ok[2]);
/* LoamRegistration::ScanMatch WHOLE (loam_registration.cpp:38-99). result_pose is IN-OUT like the reference's `SE3& result_pose` (and
 * locgpu_ndt_scan_match): with stats->status 3 or 4 a class's evaluation reported false and ScanMatch returned before
 * `result_pose = pose` (:56-70) — the caller's value stays, no output cloud is written, the call itself returns LOCGPU_OK; otherwise
 * it receives the result. stats (optional): status as above, iterations = evaluations made, last_effective_num = the two classes'
 * counts summed, converged / last_dx_norm as for ICP. out_cloud (optional): n_edge + n_surf points of out_stride_bytes each — the edge
 * points followed by the surface points (:93-95) under pose.matrix().cast<float>() (:96); only x, y, z of each point are written,
 * the other fields are the caller's. A switched-off class's scan may be NULL; when it is given its points still join the output cloud. */
LOCGPU_API int locgpu_loam_scan_match(locgpu_loam* l, const void* edge, size_t n_edge, const void* surf, size_t n_surf, size_t stride_bytes,
                                      const double init_pose[7], double result_pose[7], locgpu_align_stats* stats, void* out_cloud,
                                      size_t out_stride_bytes);
/* Many feature scans against the one pair of maps (no reference counterpart: the reference loops ScanMatch, loam_registration.cpp:38-99,
 * over scans). Scan i is edge_srcs[i] (edge_counts[i] points) with surf_srcs[i] (surf_counts[i]); every scan runs its own loop and
 * leaves it on its own. init_poses / out_poses: n_scans × 7; stats: n_scans entries or NULL. out_poses[i] = init_poses[i] for a scan
 * whose evaluation failed (status 3 / 4). The handle keeps the two classes' storage batches between calls and only grows them; the
 * partial sums are split by the call's shape, so a scan's last bits may differ between a batch and locgpu_loam_scan_match, never
 * between two equal calls. LOCGPU_ERR_INVALID for n_scans < 1. */
LOCGPU_API int locgpu_loam_align_batch(locgpu_loam* l, int n_scans, const void* const* edge_srcs, const size_t* edge_counts,
                                       const void* const* surf_srcs, const size_t* surf_counts, size_t stride_bytes, const double* init_poses,
                                       double* out_poses, locgpu_align_stats* stats);

/* ---- MatchingInterface::GetFitnessScore (matching_interface.h:53), which the reference leaves a stub that returns 0
 * (icp_registration.cpp:246-250): how good an alignment is, as pcl::Registration::getFitnessScore defines it. For a source cloud,
 * a pose T and max_range in metres (+inf allowed):
 *   q_i   = (float)(T·p_i), the product in FP64 and one cast — the query the alignment itself uses (icp_registration.cpp:169-170);
 *           points with a non-finite coordinate are skipped and not counted (pcl::isFinite, icp_registration.cpp:64);
 *   d²_i  = float32 squared distance from q_i to its EXACT nearest target point, dx² + (dy² + dz²) as the tree search evaluates
 *           it (KdTree::ComputeDisForLeaf, kdtree.cpp:197-212) — never the alpha-pruned search of the matcher's options: a score does not depend on a pruning knob;
 *   inlier iff d²_i <= (float)(max_range · max_range);
 *   score = Σ_inliers (double)d²_i / inliers, +infinity when there is no inlier.
 * The sums are reduced in a fixed order that does not depend on the batch: the same cloud and pose give the same bits alone, among
 * other poses, in a batch of any size and in a candidate search. */
typedef struct locgpu_fitness {
    double score;          /* mean squared distance of the inliers [m²]; +inf without inliers */
    int64_t inliers;       /* points with d² <= max_range² */
    int64_t finite_points; /* points that were queries at all */
} locgpu_fitness;
/* Score of ONE cloud under n_poses >= 1 poses (n_poses × 7 doubles; out: n_poses entries). The cloud is uploaded once. With more
 * than one pose the call goes through the context's shared-source batch (see locgpu_icp_init_search for what that retains). */
LOCGPU_API int locgpu_icp_fitness(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double* poses, int n_poses,
                                  double max_range, locgpu_fitness* out);
/* Score of every scan of a batch under its own pose (poses: n_scans × 7; out: n_scans entries). Ordinary and shared-source batches;
 * a sharded batch is refused with LOCGPU_ERR_INVALID. Equals locgpu_icp_fitness of each scan bit for bit. */
LOCGPU_API int locgpu_icp_fitness_batch(locgpu_ctx* ctx, locgpu_batch* batch, const double* poses, double max_range, locgpu_fitness* out);
/* Score of the source cloud that the context's most recent host-pointer single-scan call (locgpu_icp_scan_match, locgpu_icp_align,
 * locgpu_icp_hb, ...) left in HBM, under `pose`: no second upload. This is what IcpRegistration::GetFitnessScore binds to after
 * EnableFitnessScore: nothing is added to ScanMatch itself (icp_registration.cpp:216-244). LOCGPU_ERR_INVALID
 * when no such cloud is resident. */
LOCGPU_API int locgpu_icp_fitness_resident(locgpu_ctx* ctx, const double pose[7], double max_range, locgpu_fitness* out);

/* ---- A batch whose n_entries entries all read ONE resident cloud (no reference counterpart: the reference's only way to try several
 * initial poses is to call ScanMatch again, icp_registration.cpp:216-244). The cloud is uploaded once, here; poses, flags, neighbour
 * lists, sums and stats are per entry as in any batch, and locgpu_icp_align_batch / _begin / locgpu_align_batch_end /
 * locgpu_icp_hb_batch / locgpu_ndt_align_batch / locgpu_icp_fitness_batch / locgpu_ndt_fitness_batch treat it as the batch of n_entries uploaded copies of the
 * cloud, bit for bit, without the copies (16 B per point and entry). Not shardable and not poolable; locgpu_batch_upload_async into
 * it is refused with LOCGPU_ERR_INVALID (make a new one for another cloud). */
LOCGPU_API int locgpu_batch_create_shared(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, int n_entries, locgpu_batch** out);

/* ---- Initial-pose search (no reference counterpart: Loc starts ScanMatch from SetInitPose(SE3()) or a GNSS position with an IMU
 * heading, lio_matching_flow.cpp:203-205,227-262, metres and degrees off, and IcpRegistration::ScanMatch, icp_registration.cpp:216-244,
 * only refines a pose that is nearly right). Aligns the cloud from each of m candidate poses (candidates: m × 7) with the caller's ICP
 * options — any method and search mode; each candidate runs exactly the Gauss–Newton loop locgpu_icp_align_batch runs on a batch of
 * m copies of the cloud, bit for bit — scores every result (above, sopts->max_range) and reports all m (out_poses m × 7, out_fit m,
 * stats m or NULL) and the winner: *best = the lowest score among the candidates with inliers >= 1 and inliers / finite_points >=
 * min_inlier_ratio, ties to the lower index; -1 when none qualifies (the outputs are filled all the same). A candidate whose alignment
 * ended with too few effective points keeps the pose it had, as in locgpu_icp_align_batch, and is scored there. sopts NULL = defaults.
 * m is processed in equal chunks of at most 256 candidates, and of at most 1 GiB of per-candidate workspace (28 B per point and
 * candidate; a single candidate is always allowed). The context keeps that workspace and one copy of the cloud (16 B per point)
 * for the next call — grow-only within the bound — until locgpu_destroy.
 * LOCGPU_ERR_NO_TARGET before a set_target; LOCGPU_ERR_INVALID for m < 1, n == 0, a NaN max_range, a negative or NaN min_inlier_ratio. */
typedef struct locgpu_init_search_opts {
    double max_range;        /* 1.0 m: the inlier range of the score */
    double min_inlier_ratio; /* 0.5: a winner needs inliers / finite_points >= this */
} locgpu_init_search_opts;
LOCGPU_API void locgpu_init_search_opts_default(locgpu_init_search_opts* o);
LOCGPU_API int locgpu_icp_init_search(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double* candidates, int m,
                                      const locgpu_icp_opts* opts, const locgpu_init_search_opts* sopts, double* out_poses,
                                      locgpu_fitness* out_fit, locgpu_align_stats* stats, int* best);
/* ---- The JOINT score of a LOAM alignment and its initial-pose search (MatchingInterface::GetFitnessScore, which
 * LoamRegistration leaves a stub that returns 0, loam_registration.cpp:101-104; Loc starts this matcher from SetInitPose(SE3()) or a
 * GNSS position like the other two, lio_matching_flow.cpp:292-313). For a pose T and max_range every ENABLED class c — the surface
 * scan against the surface map, the edge scan against the edge map — scores {Σ_c, inliers_c, finite_c} exactly as locgpu_icp_fitness
 * defines it (exact 1-NN, fixed 1024-point split); then
 *   joint.score = (Σ_surf + Σ_edge) / (inliers_surf + inliers_edge), surface added first, +inf with no inlier in either class;
 *   joint.inliers / joint.finite_points = the sums of the two classes'; a switched-off class adds nothing and reports {+inf, 0, 0}.
 * A POOLED mean, not a sum of two means: LoamRegistration's normal equations are a plain sum over all points of both classes
 * (loam_registration.cpp:76-79), and the score weights a point the same way. The joint Σ is formed on the device from the un-rounded
 * class sums. out holds THREE entries per pose: [3i] joint, [3i + 1] surface, [3i + 2] edge; the two class entries are the bits
 * locgpu_icp_fitness gives on a context holding that class's map, and all three are the same bits alone, among other poses and in
 * any chunk of a search.
 * locgpu_loam_fitness: one pair of scans (each copied once) under n_poses >= 1 poses (n_poses × 7). A switched-off class's scan is
 * not read and may be NULL; an enabled class's scan may be empty when the other is not. The handle's storage batches take a
 * SHARED-SOURCE form — every entry reads the one region of points — so locgpu_loam_fitness_resident has nothing resident afterwards.
 * LOCGPU_ERR_NO_TARGET without a target; LOCGPU_ERR_INVALID for n_poses < 1, both scans empty, a NaN max_range. */
LOCGPU_API int locgpu_loam_fitness(locgpu_loam* l, const void* edge, size_t n_edge, const void* surf, size_t n_surf, size_t stride_bytes,
                                   const double* poses, int n_poses, double max_range, locgpu_fitness* out /* n_poses × 3 */);
/* The candidate search of locgpu_icp_init_search for the LOAM matcher: each of the m candidates (m × 7) runs exactly the joint
 * Gauss–Newton loop locgpu_loam_align_batch runs on m copies of the pair of scans, bit for bit — without the copies — and every
 * result is scored as above under sopts->max_range (out_poses m × 7, out_fit m × 3, stats m or NULL). *best = the lowest JOINT score
 * among the candidates with joint inliers >= 1 and joint inliers / finite_points >= min_inlier_ratio, ties to the lower index; -1
 * when none qualifies (the outputs are filled all the same). A candidate whose evaluation failed (status 3 / 4) keeps its initial
 * pose, as in locgpu_loam_align_batch, and is scored there. sopts NULL = defaults. m is processed in equal chunks of at most 256
 * candidates and at most 1 GiB of per-candidate workspace summed over both classes (44 B per point and candidate: the storage
 * batches are plain ones, whose source rows stay unused beyond the first; a single candidate is always allowed). The handle keeps
 * that workspace, the candidates' joint state and one pinned copy of each scan for the next call — grow-only — until
 * locgpu_loam_destroy. Errors as locgpu_loam_fitness, and LOCGPU_ERR_INVALID for m < 1 or a negative or NaN min_inlier_ratio; every
 * argument is checked before anything is copied or enqueued. */
LOCGPU_API int locgpu_loam_init_search(locgpu_loam* l, const void* edge, size_t n_edge, const void* surf, size_t n_surf, size_t stride_bytes,
                                       const double* candidates, int m, const locgpu_init_search_opts* sopts, double* out_poses,
                                       locgpu_fitness* out_fit /* m × 3 */, locgpu_align_stats* stats, int* best);

/* Host helper (no device, no context): the candidate poses centre ∘ (yaw about the centre's z axis, then x / y offsets in the
 * centre's frame) for yaw = a · yaw_step, x = i · xy_step, y = j · xy_step with |a| <= floor(yaw_half / yaw_step + 1e-9),
 * |i|, |j| <= floor(xy_half / xy_step + 1e-9) — the kind of uncertainty a GNSS position with an IMU heading has
 * (lio_matching_flow.cpp:227-262). Order: yaw-major, then x, then y, each ascending. A half of 0 means that one value (its step is
 * ignored). Writes min(count, cap) poses to out (7 doubles each) and always the count to *n_out. */
LOCGPU_API int locgpu_pose_grid(const double centre[7], double xy_half, double xy_step, double yaw_half, double yaw_step, double* out,
                                size_t cap, size_t* n_out);

/* ---- One node, several GPUs (BASELINE.json configs[3]; no reference counterpart): one process per GPU, one context per process,
 * the ranks joined by an RCCL communicator. A SHARDED batch has n_total scans; this rank holds the points of scans
 * [first_scan, first_scan + n_local) — or, for one large alignment split by points, a slice of the points of every scan
 * (first_scan = 0, n_local = n_total). Poses, convergence flags and normal equations exist for all n_total scans on every rank:
 * in each Gauss–Newton iteration the per-scan sums (21 H + 6 B + effective_num; zeros for scans a rank does not hold) are
 * all-reduced over xGMI (on the context's communication stream, in host order) and every rank solves every scan, so all ranks take the same decisions.
 * The align / hb entry points are then COLLECTIVE (every rank calls them with the same poses and options; init_poses, out_poses
 * and stats have n_total entries) and scan-sharded results are bit-identical to the single-GPU ones. */
#define LOCGPU_COMM_ID_BYTES 128
LOCGPU_API int locgpu_comm_unique_id(void* id_out /* LOCGPU_COMM_ID_BYTES, made on one rank and handed to all */);
LOCGPU_API int locgpu_comm_init(locgpu_ctx* ctx, int rank, int world, const void* id);
LOCGPU_API int locgpu_comm_info(const locgpu_ctx* ctx, int* rank, int* world);
LOCGPU_API int locgpu_batch_create_sharded(locgpu_ctx* ctx, const void* const* srcs, const size_t* counts, size_t stride_bytes, int n_local,
                                           int first_scan, int n_total, locgpu_batch** out);
/* IcpRegistration::SetInputTarget, collective: rank `root` builds the KD-tree from ITS pts (the others' are ignored) and
 * broadcasts the packed tree — one host build per node instead of one per GPU. */
LOCGPU_API int locgpu_icp_set_target_bcast(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes, int root);

/* ---- Open-scan pool (round 5; no reference counterpart): the batched many-scans-vs-one-map mode as a continuous service.
 * The reference's loops stop per scan (icp_registration.cpp:358-376, ndt_registration.cpp:393-462): the late Gauss–Newton
 * iterations of a batch hold a handful of open scans, and a small batch pays every iteration's fixed costs for little work. A pool
 * owns `slots` scan slots in HBM and runs ONE launch sequence per iteration over the union of the open scans of every job admitted so
 * far; a job = a set of scans with their initial poses, submitted at any time (its points are copied into free source regions on
 * the copy stream while the pool iterates, ahead of the slots) and collected by ticket. Every `chunk` iterations the host reads the
 * flags: finished scans leave, waiting scans enter one by one as slots come free. A job of `scans_per_job` scans gets, bit for bit, the poses locgpu_*_align_batch gives a plain batch of those
 * scans (same kernels; the partial sums are split as that batch would split them).
 * The pool matches against the target (tree or NDT voxels) the context holds when its chunks run, with the options given here.
 * Calls on a pool follow the context's rule: one caller thread. The host clouds of a submit must stay valid until
 * locgpu_pool_wait has returned for its ticket (they are packed by the context's upload service beside the caller).
 * With a communicator on the context (locgpu_comm_init) a job is SHARDED like a sharded batch — n_total scans, this rank holds the
 * points of [first_scan, first_scan + n_local) — submit and wait are collective calls made in the same order on every rank, and
 * each pooled iteration has one all-reduce of [slots][32] doubles; every rank ends with every pose. */
typedef struct locgpu_pool locgpu_pool;
typedef struct locgpu_pool_opts {
    int32_t slots;          /* scans the pool iterates at a time                                                     */
    int32_t prefetch;       /* source regions beyond `slots`: scans whose points are in HBM ahead of a free slot     */
                            /* (-1 = as many as slots). A job is accepted as soon as it has regions.                 */
    int32_t scans_per_job;  /* the job size whose plain-batch bits a job gets (0: as a batch of `slots` scans)        */
    int32_t chunk;          /* iterations between two looks at the flags, 1..8 (0 = 4)                               */
    int32_t matcher;        /* 0 = ICP with `icp`; 1 = NDT against the context's NDT target (locgpu_ndt_set_target)  */
    uint64_t max_points;    /* per scan                                                                              */
    locgpu_icp_opts icp;
} locgpu_pool_opts;
LOCGPU_API void locgpu_pool_opts_default(locgpu_pool_opts* o);
LOCGPU_API int locgpu_pool_create(locgpu_ctx* ctx, const locgpu_pool_opts* opts, locgpu_pool** out);
LOCGPU_API void locgpu_pool_destroy(locgpu_pool* pool);
/* init_poses: n_total × 7. Returns once the job has source regions (it lets running scans finish when there are none) and its copy
 * has been started; *ticket identifies it. Unsharded: n_local = n_total, first_scan = 0. */
LOCGPU_API int locgpu_pool_submit(locgpu_pool* pool, const void* const* srcs, const size_t* counts, size_t stride_bytes, int n_local, int first_scan,
                                  int n_total, const double* init_poses, int64_t* ticket);
/* Runs the pool until every scan of the job has finished; out_poses n_total × 7, stats (optional) n_total. A ticket is good once. */
LOCGPU_API int locgpu_pool_wait(locgpu_pool* pool, int64_t ticket, double* out_poses, locgpu_align_stats* stats);
/* One turn of the pool without collecting anything: look at the chunk in flight (block != 0: wait for it; with several ranks a
 * non-blocking look is a no-op), let finished scans out and waiting jobs in, enqueue the next chunk. For callers that keep the pool
 * full — submit whenever locgpu_pool_info reports room — instead of waiting for the oldest ticket. *done: every scan of the job has
 * finished (locgpu_pool_wait returns at once). */
LOCGPU_API int locgpu_pool_step(locgpu_pool* pool, int block);
LOCGPU_API int locgpu_pool_done(const locgpu_pool* pool, int64_t ticket, int* done);
/* out = {slots, free slots, jobs not collected, pooled iterations launched, Σ over them of the open scans this rank held, open scans,
 *        source regions, free source regions} */
LOCGPU_API int locgpu_pool_info(const locgpu_pool* pool, int64_t out[8]);
/* With locgpu_profile_enable on: out[0] = device ms of the chunks run since the last reset (HIP events on the pool's stream), out[1] = chunks. */
LOCGPU_API int locgpu_pool_profile_read(locgpu_pool* pool, double out[2], int reset);

/* ---- NDT target: NdtRegistration::SetInputTarget → SetDirectNdtTargetCloud (ndt_registration.cpp:65-85, 87-148), or with
 * opts->method == 2 → SetIncNdtTargetCloud (:150-183): the voxel set then PERSISTS across calls (LRU of opts->capacity voxels,
 * statistics of a voxel recomputed from the points the latest call put into it); switching method, voxel_size or capacity,
 * or a direct call, starts from an empty set. */
LOCGPU_API int locgpu_ndt_set_target(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes, const locgpu_ndt_opts* opts);
/* out[0]=voxels kept, out[1]=hash-table capacity, out[2]=bytes in HBM */
LOCGPU_API int locgpu_ndt_target_info(const locgpu_ctx* ctx, int64_t out[3]);
/* Read the voxel table back (tests): keys n×3 int32, mu n×3 f64, info n×9 f64 row-major; returns count through *n_out. */
LOCGPU_API int locgpu_ndt_dump(locgpu_ctx* ctx, int32_t* keys, double* mu, double* info, size_t cap, size_t* n_out);
/* Debug / test read-back (like locgpu_debug_batch_nn) of the open-addressing SLOT array of whichever NDT target the context holds —
 * the direct table (the grids_ map of SetDirectNdtTargetCloud, ndt_registration.cpp:87-148), a voxel set (locgpu_ndt_set_target_set) or
 * the incremental key -> voxel table of the last call (SetIncNdtTargetCloud, :150-183): *n_slots = slots of the table (a power of two);
 * keys[i] = the raw 64-bit key in slot i, all ones = free; vid[i] = the index of that voxel's record (direct and set: the row of
 * locgpu_ndt_dump / of the set's records in (target, key) order; incremental: the voxel's storage slot), -1 for a free slot. The first
 * min(cap, *n_slots) entries are written; NULL arrays: the count only. Copies, nothing else: no alignment depends on it. */
LOCGPU_API int locgpu_debug_ndt_slots(locgpu_ctx* ctx, uint64_t* keys, int32_t* vid, size_t cap, size_t* n_slots);
/* ---- NdtRegistration::ScanMatch minus the output cloud (ndt_registration.cpp:238-257 → AlignNdt :374-464).
 * When stats->status == 1 the reference leaves result_pose unassigned; out_pose then holds init_pose. */
LOCGPU_API int locgpu_ndt_align(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double init_pose[7],
                                double out_pose[7], locgpu_align_stats* stats);
/* One evaluation of the sums AlignNdt / AlignIncNdt form per iteration (ndt_registration.cpp:399-433, :286-347) at `pose`, without the
 * update, against the current NDT target, direct or incremental — what locgpu_icp_hb is for the ICP methods (tests and tools read the
 * normal equations of an NDT iteration through it). H 6×6 row-major, B, effective_num (direct: source points, :432; incremental:
 * accepted residuals, :347); *ok: direct det(H) != 0 && effective_num >= min_effective_pts (:435-440), incremental effective_num >=
 * min_effective_pts (:349). Changes nothing an alignment depends on. */
LOCGPU_API int locgpu_ndt_hb(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double pose[7], double H[36], double B[6],
                             int64_t* effective_num, int* ok);
/* The same for every scan of a batch at its pose. hb: n_scans × 44 doubles = H36, B6, effective_num, ok (the row of locgpu_icp_hb_batch). */
LOCGPU_API int locgpu_ndt_hb_batch(locgpu_ctx* ctx, locgpu_batch* b, const double* poses, double* hb);

/* ---- NdtRegistration::GetFitnessScore, which the reference leaves a stub that returns 0 (ndt_registration.cpp:466-471): how good an
 * alignment is against the DIRECT NDT target, in the terms of the alignment itself — the χ² residual AlignNdt forms for its gate
 * (ndt_registration.cpp:416-421) and then drops. For a source cloud, a pose T and the target's voxel_size, nearby_type and
 * res_outlier_th (locgpu_ndt_set_target):
 *   a point with a non-finite coordinate is skipped and not counted (the rule of the ICP score above);
 *   qs    = T·p in FP64; its voxel key is (int)(qs · inv_voxel_size) per axis, truncation toward zero (ndt_registration.cpp:404);
 *   the voxels looked up are key + nearby_grids_ (ndt_registration.cpp:57-58): 1 for CENTER, 7 for NEARBY6. A key outside ±2^20 or a
 *           voxel that is not in the table contributes nothing;
 *   for every voxel found: e = qs − μ, res = ((e·info[:,0])·e.x + (e·info[:,1])·e.y) + (e·info[:,2])·e.z with
 *           e·info[:,c] = (e.x·info[0][c] + e.y·info[1][c]) + e.z·info[2][c] — eᵀ·info·e as the alignment's kernel associates it;
 *   a voxel is accepted iff !(isnan(res) || res > res_outlier_th) (AlignNdt's gate, ndt_registration.cpp:417-421);
 *   a point with at least one accepted voxel is an inlier, and its value is the MINIMUM accepted res — the voxel that explains the
 *           point best, whatever the order of the probes;
 *   score = Σ_inliers min res / inliers, +infinity when there is no inlier.
 * In the locgpu_fitness of these four entry points `score` is therefore a mean χ² residual, DIMENSIONLESS (not m²), `inliers` the
 * points with an accepted voxel and `finite_points` the points that were looked up at all. Same determinism as the ICP score: no
 * atomics on the sums and a fixed split that does not depend on the batch — a cloud and a pose give the same bits alone, among
 * other poses, in a batch of any size, from a shared-source batch and in any chunk of a search.
 * All four: LOCGPU_ERR_NO_TARGET before locgpu_ndt_set_target; LOCGPU_ERR_INVALID when the current NDT target is the incremental
 * one (method 2: another table, residuals weighted differently — not scored), and for NULL arguments. */
/* Score of ONE cloud under n_poses >= 1 poses (n_poses × 7 doubles; out: n_poses entries; score: mean χ², dimensionless). The cloud is
 * uploaded once; with more than one pose the call goes through the context's shared-source batch (locgpu_icp_init_search says what
 * that retains). LOCGPU_ERR_INVALID for n == 0 or n_poses < 1. */
LOCGPU_API int locgpu_ndt_fitness(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double* poses, int n_poses,
                                  locgpu_fitness* out);
/* Score of every scan of a batch under its own pose (poses: n_scans × 7; out: n_scans entries; score: mean χ², dimensionless).
 * Ordinary and shared-source batches; a sharded batch is refused with LOCGPU_ERR_INVALID. Equals locgpu_ndt_fitness of each scan
 * bit for bit. */
LOCGPU_API int locgpu_ndt_fitness_batch(locgpu_ctx* ctx, locgpu_batch* batch, const double* poses, locgpu_fitness* out);
/* Score (mean χ², dimensionless) of the source cloud that the context's most recent host-pointer single-scan call
 * (locgpu_ndt_scan_match, locgpu_ndt_align, ...) left in HBM, under `pose`: no second upload. This is what
 * NdtRegistration::GetFitnessScore binds to after EnableFitnessScore: nothing is added to ScanMatch itself
 * (ndt_registration.cpp:238-260). LOCGPU_ERR_INVALID when no such cloud is resident. */
LOCGPU_API int locgpu_ndt_fitness_resident(locgpu_ctx* ctx, const double pose[7], locgpu_fitness* out);
/* Initial-pose search with the NDT matcher (no reference counterpart; the flow the reference ships matches with direct NDT from
 * SetInitPose(SE3()) or a GNSS position with an IMU heading, lio_matching_flow.cpp:203-205,227-262). As locgpu_icp_init_search: each
 * of the m candidates runs exactly the loop locgpu_ndt_align_batch runs on a batch of m copies of the cloud, bit for bit; every result
 * is scored as above (out_fit[i].score: mean χ², dimensionless) and *best is the lowest score among the candidates with inliers >= 1
 * and inliers / finite_points >= sopts->min_inlier_ratio, ties to the lower index, -1 when none qualifies. sopts->max_range is NOT
 * used: the gate of the score is the target's res_outlier_th. A candidate whose alignment ended with status 1 (det(H) == 0) keeps
 * its initial pose, as in locgpu_ndt_align_batch, and is scored there. Chunks and retained workspace: those of
 * locgpu_icp_init_search (at most 256 candidates and 1 GiB per chunk, grow-only on the context).
 * LOCGPU_ERR_INVALID also for m < 1, n == 0, a negative or NaN min_inlier_ratio. */
LOCGPU_API int locgpu_ndt_init_search(locgpu_ctx* ctx, const void* src, size_t n, size_t stride_bytes, const double* candidates, int m,
                                      const locgpu_init_search_opts* sopts, double* out_poses, locgpu_fitness* out_fit,
                                      locgpu_align_stats* stats, int* best);

/* ---- hipGraph mode (BASELINE config 5, streaming loop). When on, an align call replays instantiated graphs of Gauss–Newton
 * iterations instead of launching kernel by kernel: one graph of the first eight iterations (with the state upload and
 * read-back) — the typical alignment ends inside it: one graph launch, one host synchronisation — and a four-iteration graph
 * replayed while scans are still open. Kernels early-out per scan on a device-side flag, so the fixed node sequence equals the
 * reference's data-dependent loop (icp_registration.cpp:358-376). Graphs are captured once per batch, options and target and
 * re-captured when any of them changes. Results are bit-identical to the eager mode. */
LOCGPU_API int locgpu_graph_enable(locgpu_ctx* ctx, int on);

/* ---- Measurement hooks (bench.py / tests; no reference counterpart). */
/* Average device time in ms of each hot kernel over the calls since the last reset, measured with hipEvents on the
 * context's stream: out[0]=search, out[1]=fit+accumulate, out[2]=solve/update, out[3..5]=their launch counts.
 * Timing is only collected when enabled (it serialises launches with events): on = 1 times all three stages (four event
 * records per iteration), on = 2 only the search stage (two records per iteration; out[1], out[2] and their counts stay 0). */
LOCGPU_API int locgpu_profile_enable(locgpu_ctx* ctx, int on);
LOCGPU_API int locgpu_profile_read(locgpu_ctx* ctx, double out[6], int reset);
/* Total tree nodes / leaves visited by the search kernel of the NEXT align/hb call(s) when counting is on
 * (separate instrumented kernel; never on in timed runs). out[0]=nodes, out[1]=leaves, out[2]=queries, out[3]=distinct 8-byte
 * tree slots a search launch read at all, summed over the launches (the compulsory tree traffic of the search stage). */
LOCGPU_API int locgpu_visit_count_enable(locgpu_ctx* ctx, int on);
LOCGPU_API int locgpu_visit_count_read(locgpu_ctx* ctx, uint64_t out[4], int reset);

/* Search bookkeeping since the last reset (enabled by the first call): out[0] = queries handled by the fast search
 * kernel's launches, out[1] = queries it handed to the exact redo kernel (distance ties / near-misses on the top tree levels),
 * out[2] = grid mode: queries the tile kernel handed to the ring-walk kernel, out[3] = diagnostic build (LOCGPU_STAMP=1) only: queries of the
 * fast tree search that had to walk the un-stored top levels of their first descent again ("replays"); 0 otherwise. */
LOCGPU_API int locgpu_search_stats_read(locgpu_ctx* ctx, uint64_t out[4], int reset);
/* Test hook: the neighbour lists the batch's most recent search stage left behind (the one inside the last locgpu_icp_hb_batch /
 * align call on it; k = 5, or 1 for P2P), as ORIGINAL point indices of the target cloud in ascending distance — the order
 * KdTree::GetClosestPoint returns (kdtree.cpp:160-165). out[(scan * max_points + i) * k + j]; -1 where there is none
 * (points beyond a scan's count hold stale values). This is how the tests compare the HOT search kernel's lists with the oracle's. */
LOCGPU_API int locgpu_debug_batch_nn(locgpu_ctx* ctx, locgpu_batch* batch, int k, int32_t* out);
/* Test hook: the run flags of the search stage of the batch's last Gauss-Newton iteration (an alignment or an H/B evaluation; a
 * fitness score's search does not count) — out[n_scans * ceil(max_n / 64)], one 64-bit word per 64 points of a
 * scan, bit j of word w set: point 64 w + j is a leader of the plane fit (its neighbour set is not known to equal the previous
 * point's), clear: a follower. *written = 1 when that stage wrote flags (the 64-lane walk kernel of a P2Plane search with
 * LOCGPU_PLANE_RUNFLAGS on), 0 when it did not (the words are then stale or undefined). Words of 64-point groups that lie wholly
 * past a scan's count are never written. */
LOCGPU_API int locgpu_debug_batch_run_flags(locgpu_ctx* ctx, locgpu_batch* batch, uint64_t* out, int* written);
/* Test hook: which of the context's compute streams (0, 1 or 2) the batch's current — begun and not ended — or last alignment runs on.
 * A stream is leased per alignment: locgpu_*_align_batch_begin keeps the batch on its stream while no other alignment in flight uses
 * it and otherwise moves it to the least-loaded one, so that a caller who rotates more batches than there are streams (three in flight
 * over four batches) still has every alignment in flight on a stream of its own. Before the first alignment: the stream the batch was
 * dealt when it was created. -1 for NULL. */
LOCGPU_API int locgpu_debug_batch_slot(const locgpu_batch* batch);
/* Test hooks: the SOLVE stage that ends every Gauss-Newton iteration, on normal equations the caller chooses — the production
 * launchers of gn_solve_kernel, sum_partials_kernel and loam_solve_kernel (csrc/icp_fit.hip), not copies: the fixed-order sum of the
 * block partials, the 6×6 pivoted LU, the accept / abort rules (ICP: icp_registration.cpp:204-211, 362-375, "/16" for P2P :287; direct
 * NDT tests det(H) == 0 first and ends the alignment, ndt_registration.cpp:435-459; incremental NDT tests effective_num alone,
 * ndt_registration.cpp:349-353; LOAM: each class by its own count and det, surface first, then the sum, loam_registration.cpp:47-90),
 * the SE3 update with the refresh of R, and the stop tests. Both calls block, own their device memory for the call and touch neither
 * the context's targets nor any batch.
 *   partials   host, the kernels' own layout [n_scans][blocks_per_scan][32] doubles: 21 H (upper triangle, row by row), 6 B,
 *              effective_num, 4 spare (never read)
 *   method     a locgpu_icp_method, or 3 = direct NDT, 4 = incremental NDT (the values the library uses inside)
 *   state_in / state_out   n_scans rows of 160 bytes, the whole per-scan state: double q[4] (x y z w) at byte 0, double t[3] at 32,
 *              double R[9] (row-major) at 56, double last_dx_norm at 128, int64 last_eff at 136, then int32 iterations (144),
 *              converged (148), done (152), status (156; 0 ok, 1 direct NDT det(H) == 0, 2 incremental NDT too few, 3 / 4 LOAM surface /
 *              edge class false). state_in seeds every row; state_out receives every row as the kernels left it.
 *   do_update  0: H/B evaluation only (hb and last_eff are written)
 *   two_stage  1: the route of a sharded batch — launch_sum_partials (first = 0, n_local = n_scans) into one row per scan, then the
 *              solve on those rows with blocks_per_scan = 1
 *   scans / n_launch   optional (NULL: every scan): the scan pool's indirection — n_launch blocks, block i solves scan scans[i]
 *   hb_out     n_scans × 44 doubles = H36, B6, effective_num, ok (LOAM: n_scans × 46 = H36 and B6 of the SUM, effective_num[2], ok[2]);
 *              read first: rows no block writes (finished or unlisted scans) come back as they went in
 * locgpu_debug_loam_solve: NULL partials = the class is switched off (not both). LOCGPU_ERR_INVALID, and nothing is launched, for a
 * NULL argument, n_scans outside [1, 1024], blocks_per_scan outside [1, 4096], an unknown method, a scans entry out of range or listed
 * twice. (The rules restated: icp_registration.cpp:204-211, 362-375; ndt_registration.cpp:349-353, 435-459; loam_registration.cpp:47-90.) */
LOCGPU_API int locgpu_debug_gn_solve(locgpu_ctx* ctx, const double* partials, int n_scans, int blocks_per_scan, int method, int min_effective_pts,
                                     double eps, int max_iteration, int do_update, int two_stage, const int* scans, int n_launch,
                                     const void* state_in, void* state_out, double* hb_out);
LOCGPU_API int locgpu_debug_loam_solve(locgpu_ctx* ctx, const double* partials_surf, int blocks_surf, const double* partials_edge, int blocks_edge,
                                       int n_scans, const int min_effective_pts[2], double eps, int max_iteration, int do_update,
                                       const void* state_in, void* state_out, double* hb_out);

/* =====================================================================================================================
 * Clouds resident in HBM and the filters either side of the matcher.
 *
 * In the reference every scan passes RemoveNanPoint → VoxelFilter::Filter → ScanMatch (loc.cpp:217-224, lio.cpp:236,257),
 * the global map passes BoxFilter::Filter → SetInputTarget (loc.cpp:187-194) and every keyframe passes
 * pcl::transformPointCloud → operator+= → VoxelFilter::Filter → SetInputTarget (lio.cpp:268-306). All of these are thin
 * wrappers over PCL 1.8 (pcl::removeNaNFromPointCloud, pcl::VoxelGrid, pcl::CropBox, pcl::transformPointCloud). The entry
 * points below run the same steps on the GPU; a locgpu_cloud keeps a cloud in HBM between them so that a scan crosses PCIe
 * once. A cloud is {x, y, z, intensity} per point plus PCL's `is_dense` flag, which the PCL filters trust (a cloud flagged
 * dense is never tested for NaN) and which therefore travels with the data.
 *
 * Results equal PCL's: the same points in the same order (VoxelGrid: centroids in ascending voxel index; CropBox and
 * removeNaN: survivors in input order). VoxelGrid's float32 centroid sums run in input order (PCL's order inside a voxel is
 * whatever its unstable std::sort leaves, so the last bits of a centroid are not defined by PCL itself).
 * `intensity_offset` = byte offset of the float32 intensity inside a point (pcl::PointXYZI: 16), or LOCGPU_NO_INTENSITY.
 *
 * Two contexts on one GPU as a two-stage front-end (round 4): the calls of one context are strictly sequential (one caller thread,
 * like the reference's matcher), but a cloud of context A may be the SOURCE of locgpu_icp_align_cloud / locgpu_ndt_align_cloud and
 * the scan of locgpu_submap_add_keyframe on context B of the same GPU (B's stream is ordered behind what A has enqueued; A must
 * not modify the cloud while B uses it). A caller thread that uploads and filters scan i+1 on A while another matches scan i on B
 * overlaps the two stages — the poses are the sequential loop's, bit for bit (tests/test_gpu_filters.py, pipelined streaming loop).
 * ===================================================================================================================== */
typedef struct locgpu_cloud locgpu_cloud;
typedef struct locgpu_submap locgpu_submap;
#define LOCGPU_NO_INTENSITY ((size_t)-1)

LOCGPU_API int locgpu_cloud_create(locgpu_ctx* ctx, locgpu_cloud** out);
LOCGPU_API void locgpu_cloud_destroy(locgpu_cloud* c);
/* Host → HBM (deep copy, like every reference call that takes a CloudPtr). */
LOCGPU_API int locgpu_cloud_upload(locgpu_cloud* c, const void* pts, size_t n, size_t stride_bytes, size_t intensity_offset, int is_dense);
LOCGPU_API int locgpu_cloud_info(const locgpu_cloud* c, size_t* n, int* is_dense);
/* HBM → host: writes x, y, z (and intensity unless LOCGPU_NO_INTENSITY) of each point, leaves the other bytes of the
 * caller's points alone. Fails with LOCGPU_ERR_INVALID when capacity < the cloud's size. */
LOCGPU_API int locgpu_cloud_download(const locgpu_cloud* c, void* out, size_t capacity, size_t stride_bytes, size_t intensity_offset);
LOCGPU_API int locgpu_cloud_copy(const locgpu_cloud* in, locgpu_cloud* out);

/* RemoveNanPoint, LocUtils/include/LocUtils/common/point_cloud_utils.h:13-20 (pcl::removeNaNFromPointCloud). out may be in. */
LOCGPU_API int locgpu_cloud_remove_nan(const locgpu_cloud* in, locgpu_cloud* out);
/* VoxelFilter::Filter, LocUtils/src/model/cloud_filter/voxel_filter.cpp:19-25 (pcl::VoxelGrid, leaf = (v, v, v), defaults).
 * *passthrough (optional) = 1 when PCL's "leaf size is too small for the input dataset" rule copied the input unchanged.
 * out may be in (the reference filters local_map_ in place, lio.cpp:300). */
LOCGPU_API int locgpu_cloud_voxel_filter(const locgpu_cloud* in, float leaf, locgpu_cloud* out, int* passthrough);
/* BoxFilter::Filter, LocUtils/src/model/cloud_filter/box_filter.cpp:25-32 (pcl::CropBox, inclusive bounds). The caller
 * computes the edges as BoxFilter::CalculateEdge does (:59-66): min = origin − size, max = origin + size in float32. */
LOCGPU_API int locgpu_cloud_crop_box(const locgpu_cloud* in, const float min_xyz[3], const float max_xyz[3], locgpu_cloud* out);
/* pcl::transformPointCloud(in, out, pose.matrix()) with the double-precision matrix of lio.cpp:244,279. out may be in. */
LOCGPU_API int locgpu_cloud_transform(const locgpu_cloud* in, const double pose[7], locgpu_cloud* out);
/* pcl::PointCloud::operator+= (lio.cpp:245,291,297). */
LOCGPU_API int locgpu_cloud_append(locgpu_cloud* dst, const locgpu_cloud* src);

/* The matcher entry points on resident clouds (same semantics as their host-pointer versions above). */
LOCGPU_API int locgpu_icp_set_target_cloud(locgpu_ctx* ctx, const locgpu_cloud* target);
/* The same SetInputTarget (icp_registration.cpp:14-22; Lio re-ingests its local map every keyframe, lio.cpp:296-305) with the host
 * tree build on a worker thread: returns once the cloud has been copied out (the caller may change or free it), the build runs while
 * the caller uploads and filters the next scan, and the first entry point that reads the ICP target — an align, H/B, k-NN,
 * target_info — completes the ingest (device buffers, copy) on the caller's thread and reports its errors. Until then the previous
 * target stays in place; another SetInputTarget supersedes a pending one. Like every SetInputTarget it must not be called between a
 * locgpu_*_align_batch_begin and its end. Results are those of locgpu_icp_set_target_cloud. */
LOCGPU_API int locgpu_icp_set_target_cloud_async(locgpu_ctx* ctx, const locgpu_cloud* target);
LOCGPU_API int locgpu_ndt_set_target_cloud(locgpu_ctx* ctx, const locgpu_cloud* target, const locgpu_ndt_opts* opts);
LOCGPU_API int locgpu_icp_align_cloud(locgpu_ctx* ctx, const locgpu_cloud* src, const double init_pose[7], const locgpu_icp_opts* opts,
                                      double out_pose[7], locgpu_align_stats* stats);
LOCGPU_API int locgpu_ndt_align_cloud(locgpu_ctx* ctx, const locgpu_cloud* src, const double init_pose[7], double out_pose[7],
                                      locgpu_align_stats* stats);

/* Host-pointer one-shots (upload → filter → download), what VoxelFilter::Filter / BoxFilter::Filter / RemoveNanPoint bind to.
 * `out` needs room for n points; *out_n receives the count, *out_is_dense (optional) the flag of the result. out may be pts. */
LOCGPU_API int locgpu_voxel_filter(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes, size_t intensity_offset, int is_dense, float leaf,
                                   void* out, size_t* out_n, int* out_is_dense);
LOCGPU_API int locgpu_crop_box(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes, size_t intensity_offset, int is_dense,
                               const float min_xyz[3], const float max_xyz[3], void* out, size_t* out_n, int* out_is_dense);
LOCGPU_API int locgpu_remove_nan(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes, size_t intensity_offset, int is_dense, void* out,
                                 size_t* out_n, int* out_is_dense);

/* ---- The front-end on a whole BATCH (csrc/batch_filters.hip). The reference runs RemoveNanPoint → VoxelFilter::Filter on every scan
 * before ScanMatch (loc.cpp:217-218, lio.cpp:236; voxel_filter.cpp:19-25, point_cloud_utils.h:13-20); locgpu_batch_preprocess does
 * that for every scan of `src` in one pass — one set of launches, one sort, one read-back of n_scans {count, status} pairs:
 *   dst's scan s = x, y, z of locgpu_cloud_voxel_filter(locgpu_cloud_remove_nan(scan s of src), leaf),
 * byte for byte: the same points, count and order (centroids in ascending voxel index, float32 sums in input order), the fourth lane
 * 0. A scan is always tested for non-finite points (a batch carries no is_dense flag). Each scan has its own bounding box, min_b,
 * div_b and overflow test; equal coordinates in different scans never share a voxel; results do not depend on n_scans or on the run.
 * out_status[s] (n_scans entries or NULL) is the single-cloud filter's outcome: 0 filtered; 1 PCL's "leaf size is too small" rule —
 * the scan comes out as its finite points in input order, bits unchanged; 2 no finite point — count 0. out_counts[s] (n_scans or
 * NULL) = the filtered counts.
 * dst is an ordinary batch of the same context and n_scans — typically locgpu_batch_create_empty(ctx, n_scans, M) with M far below
 * src's capacity, so that the alignment's work lists and partial sums are sized by the FILTERED scans; dst == src works in place.
 * When a filtered scan has more than dst's max_points_per_scan points the call returns LOCGPU_ERR_INVALID, out_counts holds the
 * needed counts, locgpu_last_error names the largest, and dst is exactly as it was (points and counts). LOCGPU_ERR_INVALID, with a
 * text, also for sharded or shared-source batches, a batch whose alignment is begun and not ended, batches of different contexts or
 * n_scans, a leaf that is <= 0 or not finite, and NULL batches. A pending upload of src (and of dst) is waited for, as by every align
 * call. The call returns when the pass has run and dst's counts are known on the host; a captured graph of dst stays valid (it reads
 * the counts on the device). Scratch is grow-only on the context: about 44 B per point slot of src (60 B in place). */
LOCGPU_API int locgpu_batch_preprocess(locgpu_batch* src, float leaf, locgpu_batch* dst, int32_t* out_counts /* n_scans or NULL */,
                                       int32_t* out_status /* n_scans or NULL */);
/* Fills the batch's scans from n = n_scans resident clouds by a device-to-device copy that writes {x, y, z, 0}: the batched resident
 * form of n different scans for ICP and NDT. Clouds of any context on the batch's GPU are accepted (the copy is ordered behind what
 * their contexts have enqueued; the call is blocking, the clouds are free again when it returns). Counts are left as
 * locgpu_batch_upload_async + locgpu_batch_upload_wait leave them. Refusals: those of locgpu_batch_upload_async, a cloud with more
 * points than the batch was created for, a cloud on another GPU, n != n_scans. */
LOCGPU_API int locgpu_batch_upload_clouds(locgpu_batch* b, const locgpu_cloud* const* clouds, int n);
/* Reads scan `scan` of a batch back: *n (optional) = its count; out == NULL returns the count only. Otherwise x, y, z of each point
 * go to out + i * stride_bytes (stride_bytes >= 12; with stride_bytes >= 16 the fourth lane, which no kernel of the matcher reads,
 * is written too). LOCGPU_ERR_INVALID for a scan index outside [0, n_scans), capacity < the count, a shared-source batch or a batch
 * whose alignment is begun and not ended. */
LOCGPU_API int locgpu_batch_download_scan(locgpu_batch* b, int scan, void* out, size_t capacity, size_t stride_bytes, size_t* n);

/* LoamFeatureExtract::Extract + ExtractFromSector, LocUtils/src/model/feature_extract/loam_feature_extract.cpp:19-151 (called on every
 * scan by Lio::AddCloud(FullCloudPtr), lio.cpp:323): per-ring curvature, six sectors per ring, at most 20 edge points per sector,
 * every unmarked point a surface point; outputs ring by ring, sector by sector, edges in descending and surface points in
 * ascending curvature. `ring` = one byte per point (FullPointType::ring, point_types.h:70). Equal curvatures (an order the
 * reference's std::sort leaves open) are ordered by ring position. edge and surf must be distinct clouds of in's context.
 * Limits: num_scan ≤ 256, rings of at most 6 × 2048 points. */
LOCGPU_API int locgpu_cloud_loam_extract(const locgpu_cloud* in, const uint8_t* ring, int num_scan, locgpu_cloud* edge, locgpu_cloud* surf);
/* Host-pointer one-shot on the reference's FullPointType layout (point_types.h:65-78: x,y,z at 0, uint8 intensity at 24, uint8 ring
 * at 25, stride 64): intensity_is_u8 = 1 converts like `p.intensity = pt.intensity` (:33). Both outputs need room for n points. */
LOCGPU_API int locgpu_loam_extract(locgpu_ctx* ctx, const void* pts, size_t n, size_t stride_bytes, size_t intensity_offset, int intensity_is_u8,
                                   size_t ring_offset, int num_scan, void* edge_out, size_t* n_edge, void* surf_out, size_t* n_surf,
                                   size_t out_stride_bytes, size_t out_intensity_offset);

/* ---- LOAM on a whole BATCH (csrc/batch_loam.hip, csrc/loam_align.hip): Lio::AddCloud(FullCloudPtr)'s step — the feature picker
 * (LoamFeatureExtract::Extract, loam_feature_extract.cpp:19-151, called at lio.cpp:323), the voxel filter of both feature clouds
 * (lio.cpp:485-486: locgpu_batch_preprocess in place on each feature batch) and the match — for n DIFFERENT scans that stay in HBM.
 * locgpu_batch_loam_extract: scan s of `edge` and of `surf` becomes x, y, z of
 *   locgpu_cloud_loam_extract(scan s of src, rings[s], num_scan),
 * byte for byte: the same points, counts and order, the fourth lane +0 as locgpu_batch_preprocess leaves it. rings[s] = one byte per
 * point of scan s (host memory, read before the call returns). Every rule of the single-cloud picker holds per scan: rings shorter
 * than 131 points are skipped, rings >= num_scan are ignored, each sector goes without its last element, at most 20 edges per sector
 * (the 21st pick is marked, not emitted), the +-5 marking stops at a gap^2 > 0.05, equal curvatures are ordered by ring position. A
 * scan's result does not depend on n_scans, on its position in the batch, or on the run; the pass uses no atomics.
 * One pass — one stable sort keyed scan * num_scan + ring, one set of launches, one read-back of n_scans {edge count, surface count,
 * status} — where the single-cloud call makes seven launches, a sort and two synchronisations per scan.
 * src, edge and surf are three DISTINCT ordinary batches of one context with one n_scans. Limits: 1 <= num_scan <= 256 and
 * n_scans * num_scan <= 65535 (checked before anything is allocated; it bounds the grids and the per-sector scratch).
 * out_edge_counts / out_surf_counts / out_status: n_scans entries each, or NULL. Capacity: when a scan's edge (surface) count exceeds
 * edge's (surf's) max_points_per_scan the call returns LOCGPU_ERR_INVALID, the out arrays hold the needed counts, and BOTH
 * destinations are exactly as they were, points and counts. A scan with a ring of more than 6 x 2048 points gets out_status[s] = 1
 * (otherwise 0): the call returns LOCGPU_ERR_INVALID, locgpu_last_error names the first such scan, both destinations are untouched
 * — the single-cloud picker's refusal, per scan. LOCGPU_ERR_INVALID, with a text, also for sharded or shared-source batches, a batch
 * whose alignment is begun and not ended, batches of different contexts or n_scans, a NULL batch, NULL rings, and a NULL rings[s] for
 * a scan with points. A pending upload of any of the three batches is waited for. The call returns when the pass has run and the
 * counts of edge and surf are known on the host (device counts, locgpu_batch_download_scan and the next upload agree, as after
 * locgpu_batch_preprocess). Scratch is grow-only on the context: about 65 B per point slot of src and 340 B per sector. */
LOCGPU_API int locgpu_batch_loam_extract(locgpu_batch* src, const uint8_t* const* rings /* n_scans host arrays, counts[s] bytes each */,
                                         int num_scan, locgpu_batch* edge, locgpu_batch* surf, int32_t* out_edge_counts,
                                         int32_t* out_surf_counts, int32_t* out_status /* each n_scans or NULL */);
/* locgpu_loam_align_batch (LoamRegistration::ScanMatch per scan, loam_registration.cpp:38-99) on two RESIDENT batches: scan i is scan i
 * of `edge` with scan i of `surf`. Poses and stats are bit for bit those of locgpu_loam_align_batch on the scans that
 * locgpu_batch_download_scan returns, whatever the two batches' max_points_per_scan are: the handle's storage batches are shaped by
 * the largest COUNT of each class and the rows are brought over by one strided device-to-device copy per class (counts device to
 * device). The batches may belong to any context on the handle's GPU and are not modified. The call is blocking: pending uploads are
 * waited for and the handle's stream is ordered behind the batches' contexts. A switched-off class's batch may be NULL; the two
 * batches must have equal n_scans (1..65535). LOCGPU_ERR_INVALID for sharded and shared-source batches, a batch whose alignment is
 * begun and not ended, a NULL batch of an enabled class, a batch on another GPU. Afterwards nothing of a single scan is resident:
 * locgpu_loam_fitness_resident is refused until the next single-scan call, as after locgpu_loam_align_batch. Eager only. */
LOCGPU_API int locgpu_loam_align_batches(locgpu_loam* l, locgpu_batch* edge, locgpu_batch* surf, const double* init_poses, double* out_poses,
                                         locgpu_align_stats* stats);

/* ---- Range-image ingest (csrc/range_ingest.hip): sensor-native scans decoded in HBM. The reference's step from the driver's cloud to
 * the library's cloud is CloudConver::Conver (LocUtils/src/subscriber/cloud_subscriber.cpp:7-29): it drops non-finite points, drops
 * points with PointDistance(p) < 4.0 (LocUtils/include/LocUtils/common/point_cloud_utils.h:41-44) and keeps the survivors in input
 * order. A spinning LiDAR delivers that cloud as a RANGE IMAGE — 2 B per cell instead of 16 B per point over PCIe — and these entry
 * points take the images on the host, decode them on the device and apply Conver's two rules there.
 *
 * Sensor model: n_rings (1..256), n_cols (1..12 288, the LOAM picker's ring limit of 6 x 2048), range_scale (float32, finite, > 0,
 * metres per count), min_range (float32, finite, >= 0; the reference's value is 4.0f, 0 keeps everything) and caller-supplied float32
 * tables cos_el[n_rings], sin_el[n_rings], cos_az / sin_az with n_cols entries (az_per_ring = 0) or n_rings * n_cols entries, ring-major
 * (az_per_ring = 1: per-laser azimuth offsets). The library computes no trigonometry; locgpu_sensor_create copies the tables into HBM once.
 * Image: one per scan, uint16_t[n_rings * n_cols], ring-major, columns in acquisition order.
 * Decode of cell (ring g, column c) with count k, a = c (or g * n_cols + c with az_per_ring): k == 0 is "no return" and yields no
 * point; otherwise, each line ONE IEEE float32 operation, round to nearest, nothing fused:
 *   r = (float)k * range_scale;  h = r * cos_el[g];  x = h * cos_az[a];  y = h * sin_az[a];  z = r * sin_el[g]
 * Conver's rules: the point is dropped if x, y or z is not finite, and if sqrtf((x*x + y*y) + z*z) < min_range (products and sums each
 * rounded to float32, the comparison as the reference's float < 4.0).
 * Output of a scan: its survivors in ring-ascending, then column-ascending order as {x, y, z, +0.0f}, with one ring byte g per
 * survivor — byte for byte what the rules above, restated in numpy float32 (tests/range_image_ref.py), give. Counts, order and bits
 * do not depend on n_scans, on a scan's position in the batch or on the run; no atomics decide an output position.
 * Out of scope: an asynchronous, double-buffered form (every call here is blocking); intensity or reflectivity images (a batch's
 * fourth lane stays 0); sharded and shared-source batches; the C++ façade (the reference's Conver lives in its ROS subscriber, which
 * is not shadowed); bench.py. */
typedef struct locgpu_sensor locgpu_sensor;
typedef struct locgpu_sensor_model {
    int32_t n_rings, n_cols;
    float range_scale, min_range;
    int32_t az_per_ring, reserved;
    const float* cos_el;
    const float* sin_el;
    const float* cos_az;
    const float* sin_az;
} locgpu_sensor_model;
/* The resident form of a sensor model (Conver's constants, cloud_subscriber.cpp:7-29, point_cloud_utils.h:41-44, beside the tables).
 * The tables are read before the call returns. The sensor belongs to ctx, which frees the sensors that are still alive when it is
 * destroyed (do not destroy a sensor after its context). LOCGPU_ERR_INVALID, with a text, for out-of-range sizes, a non-finite or
 * non-positive range_scale, a negative or NaN min_range, an az_per_ring other than 0 or 1, NULL tables, a NULL model or out. */
LOCGPU_API int locgpu_sensor_create(locgpu_ctx* ctx, const locgpu_sensor_model* model, locgpu_sensor** out);
LOCGPU_API void locgpu_sensor_destroy(locgpu_sensor* s);
/* Decodes n_scans images into the batch and applies Conver's rules (cloud_subscriber.cpp:7-29, point_cloud_utils.h:41-44): scan i
 * becomes the output defined above for images[i], and the ring bytes stay resident with the batch. Blocking, like
 * locgpu_batch_upload_clouds: the images are free again when it returns. One pass for all scans: the images go through pinned staging
 * to HBM on the context's copy stream, then count, exclusive sum, verdict and scatter kernels and one read-back of n_scans counts.
 * It replaces the batch's scans; counts are left as locgpu_batch_upload_async + locgpu_batch_upload_wait leave them (device counts,
 * locgpu_batch_download_scan and the next upload agree). out_counts (n_scans entries or NULL) = the survivors per scan.
 * Capacity: when a scan has more survivors than the batch's max_points_per_scan the call returns LOCGPU_ERR_INVALID, out_counts holds
 * the needed counts, locgpu_last_error names the largest, and the batch is exactly as it was: points, counts and rings.
 * Refusals (LOCGPU_ERR_INVALID, with a text): those of locgpu_batch_upload_async — sharded and shared-source batches, an alignment
 * begun and not ended — a sensor of another context, a NULL sensor, NULL images or a NULL images[i].
 * The resident rings are dropped by any later upload into the batch (locgpu_batch_upload_async, locgpu_batch_upload_clouds), by a
 * locgpu_batch_preprocess with this batch as dst and by a locgpu_batch_loam_extract* that writes it as edge or surf. */
LOCGPU_API int locgpu_batch_upload_ranges(locgpu_batch* b, const locgpu_sensor* s, const uint16_t* const* images /* n_scans */,
                                          int32_t* out_counts /* n_scans or NULL */);
/* The resident ring bytes of scan `scan` (Conver's survivors, cloud_subscriber.cpp:7-29, point_cloud_utils.h:41-44): *n (optional) =
 * the scan's count, out == NULL returns the count only. LOCGPU_ERR_INVALID when the batch holds no resident rings, for a scan index
 * out of range, capacity < the count, or an alignment begun and not ended. */
LOCGPU_API int locgpu_batch_download_rings(locgpu_batch* b, int scan, uint8_t* out, size_t capacity, size_t* n);
/* locgpu_batch_loam_extract reading the rings that locgpu_batch_upload_ranges left in src (Conver's survivors, cloud_subscriber.cpp:7-29,
 * point_cloud_utils.h:41-44) instead of host arrays: the same pass, so results are byte for byte those of locgpu_batch_loam_extract
 * given the same rings from the host, and every limit, refusal and "destinations untouched" rule of that call holds.
 * LOCGPU_ERR_INVALID also when src has no resident rings. */
LOCGPU_API int locgpu_batch_loam_extract_resident(locgpu_batch* src, int num_scan, locgpu_batch* edge, locgpu_batch* surf,
                                                  int32_t* out_edge_counts, int32_t* out_surf_counts, int32_t* out_status /* each n_scans or NULL */);
/* The same decode pass (cloud_subscriber.cpp:7-29, point_cloud_utils.h:41-44) for ONE image into a resident cloud — the streaming Lio
 * case: the cloud becomes the scan's survivors with intensity 0 and is_dense = 1, equal to the batch form's scan byte for byte; *n
 * (optional) = their number. ring_out (n_rings * n_cols bytes of room, or NULL) receives the survivors' ring bytes, which
 * locgpu_cloud_loam_extract takes unchanged. Blocking. LOCGPU_ERR_INVALID for a NULL cloud, sensor or image and a sensor of another
 * context. */
LOCGPU_API int locgpu_cloud_upload_ranges(locgpu_cloud* c, const locgpu_sensor* s, const uint16_t* image, uint8_t* ring_out /* n_rings * n_cols or NULL */,
                                          size_t* n);

/* Measurement (tools/range_ingest_time.py): with locgpu_profile_enable on, out_ms[0] = the time on the copy stream from the first to
 * the last H2D of the images of the most recent locgpu_*_upload_ranges (host staging included: it runs under the copies), out_ms[1] =
 * the time of its four kernels — the decode of cloud_subscriber.cpp:7-29 / point_cloud_utils.h:41-44 alone. Zeros before the first
 * profiled call. */
LOCGPU_API int locgpu_range_ingest_times(locgpu_ctx* ctx, double out_ms[2]);

/* ---- Range-image ingest, motion-compensated (csrc/range_ingest.hip: rd_pose_kernel, rd_scatter_kernel). The entry points above treat a
 * scan as if the sensor stood still while it turned. In a range image a column is a firing instant, so the decode can undo the
 * sensor's motion per column at no extra pass over the points. The reference carries per-point firing times and has the poses at IMU
 * rate (lio.cpp:428-433) and the interpolation helper math::PoseInterp (LocUtils/include/LocUtils/common/math_utils.h:470-517), but
 * never applies the helper to a scan; this block does, with the caller's track.
 *
 * Sensor timing: col_time[n_cols], seconds from the scan's time origin, one per column, finite, in any order (a sensor may start
 * mid-turn). Motion of a call: K = n_knots knots per scan (2 <= K <= 256, the same K for every scan of the call); knot_times
 * [n_scans][K], seconds on the clock of col_time, finite and strictly increasing per scan; knot_poses [n_scans][K][7], the SENSOR's
 * pose in any fixed frame at each knot, quaternion xyzw then translation, the quaternion taken as given (expected unit, not
 * normalised); ref_times [n_scans], the instant whose sensor frame scan i is expressed in.
 * Pose at time q of a scan with knot times t[0..K-1] (PoseInterp's rule, math_utils.h:470-517), everything FP64:
 *   q > t[K-1]: knot K-1's pose as given. Otherwise j = the first index with t[j] < q <= t[j+1], or 0 when there is none (q == t[0]);
 *   dt = t[j+1] - t[j]; fabs(dt) < 1e-6: knot j's pose as given (:505-508). Otherwise s = (q - t[j]) / dt, translation
 *   t_j * (1 - s) + t_{j+1} * s, and the quaternion Eigen's slerp(s, .) (:513): d = a.b (summed left to right), ad = |d|;
 *   ad >= 1 - DBL_EPSILON: s0 = 1 - s, s1 = s; otherwise th = acos(ad), s0 = sin((1 - s) * th) / sin(th), s1 = sin(s * th) / sin(th);
 *   d < 0: s1 = -s1; the result s0 * a + s1 * b, not normalised.
 * Matrix of column c of scan i: (q_r, t_r) = the pose at ref_times[i], (q_c, t_c) = the pose at col_time[c], R = Eigen's
 * toRotationMatrix; M = [ R_r^T R_c | R_r^T (t_c - t_r) ], row-major 3 x 4 doubles, each dot product summed left to right.
 * Output of a scan: Conver's two rules (cloud_subscriber.cpp:7-29, point_cloud_utils.h:41-44) and the decode are applied to the RAW
 * cell exactly as by locgpu_batch_upload_ranges, so the survivors, their order, the counts and the ring bytes are those of the plain
 * call; the survivor p of cell (g, c) is stored as locgpu_cloud_transform's arithmetic gives it with M[i][c] — per row
 * (float)(((m0 * x + m1 * y) + m2 * z) + m3) in double — with the w lane +0. Only acos and sin may differ from a host restatement of
 * the above (tests/range_deskew_ref.py); given the matrices, the points are byte for byte the restatement's.
 * With every knot the pose (0,0,0,1, 0,0,0) the call leaves the bytes of locgpu_batch_upload_ranges (R of x = y = z = 0 is exactly I
 * whatever w the slerp leaves). A constant track that is NOT the identity is not expected to: R_r^T R_c is then I only to rounding.
 * Refusals, decided on the host before anything is written, so that the batch or cloud is exactly as it was (points, counts and rings):
 * LOCGPU_ERR_INVALID with a text when a col_time[c] or ref_times[i] lies before t[i][0] (nothing is extrapolated the way the
 * reference's loop would for an early query) or more than 0.5 s behind t[i][K-1] (PoseInterp's time_th) — compared through the
 * minimum and maximum of col_time, O(n_scans) — for a sensor without column times, K out of range, knot times that are not finite or
 * do not increase, a reference time that is not finite, a NULL motion or a NULL array inside it; and every refusal of the plain call,
 * the capacity one included.
 * Out of scope: clouds with per-point time fields (a per-point slerp kernel would be a later entry point on the same device
 * function); per-laser time offsets inside a column; for the cloud forms, estimating the motion and compensating a scan again once it
 * is decoded (batches: locgpu_motion_from_poses and locgpu_batch_deskew, "Deskew of a resident batch" below); an asynchronous form;
 * sharded and shared-source batches; the C++ facade; bench.py. */
typedef struct locgpu_sweep_motion {
    int32_t n_knots, reserved;
    const double* knot_times;
    const double* knot_poses;
    const double* ref_times;
} locgpu_sweep_motion;
/* The firing time of every column, for the pose lookup of math_utils.h:470-517 at decode (cloud_subscriber.cpp:7-29): the table is
 * copied into HBM before the call returns and replaces an earlier one. LOCGPU_ERR_INVALID, with a text, for a NULL sensor or table and
 * an entry that is not finite (the sensor then keeps the table it had). */
LOCGPU_API int locgpu_sensor_set_col_times(locgpu_sensor* s, const double* col_time /* n_cols */);
/* locgpu_batch_upload_ranges (Conver's survivors, cloud_subscriber.cpp:7-29) with every survivor moved into the sensor frame of
 * ref_times[i] by its column's matrix (PoseInterp, math_utils.h:470-517), as defined above. Everything the plain call promises holds:
 * blocking, one pass for all scans, the rings stay resident, no atomics decide a position, and results do not depend on n_scans or on
 * a scan's place in the batch. One more kernel ahead of the four: rd_pose_kernel writes n_scans * n_cols matrices (96 B each) into a
 * grow-only table on the context; the scatter applies them to survivors only. */
LOCGPU_API int locgpu_batch_upload_ranges_deskew(locgpu_batch* b, const locgpu_sensor* s, const uint16_t* const* images /* n_scans */,
                                                 const locgpu_sweep_motion* motion, int32_t* out_counts /* n_scans or NULL */);
/* The streaming Lio form: locgpu_cloud_upload_ranges (cloud_subscriber.cpp:7-29) with the motion of ONE scan (math_utils.h:470-517;
 * knot_times [K], knot_poses [K][7], ref_times [1]); equal to the batch form's scan byte for byte, ring_out included. A refusal leaves
 * the cloud as it was. */
LOCGPU_API int locgpu_cloud_upload_ranges_deskew(locgpu_cloud* c, const locgpu_sensor* s, const uint16_t* image, const locgpu_sweep_motion* motion,
                                                 uint8_t* ring_out /* n_rings * n_cols or NULL */, size_t* n);
/* For tests and tools, as locgpu_ndt_dump: the matrices of scan `scan` (PoseInterp at every column, math_utils.h:470-517, for the decode
 * of cloud_subscriber.cpp:7-29) as the context's most recent deskewed call computed them, n_cols * 12 doubles. *n_cols_out (optional) =
 * the number of columns; out == NULL returns it alone. LOCGPU_ERR_INVALID before any such call, for a scan index out of range and
 * capacity < n_cols * 12. */
LOCGPU_API int locgpu_range_deskew_matrices(locgpu_ctx* ctx, int scan, double* out /* n_cols * 12 */, size_t capacity, size_t* n_cols_out);
/* Measurement (tools/range_deskew_time.py): with locgpu_profile_enable on, the most recent deskewed call's out_ms[0] = copy stream,
 * motion and images; out_ms[1] = rd_pose_kernel (math_utils.h:470-517); out_ms[2] = the four decode kernels (cloud_subscriber.cpp:7-29).
 * Zeros before the first profiled call. locgpu_range_ingest_times keeps reporting the most recent plain call. */
LOCGPU_API int locgpu_range_deskew_times(locgpu_ctx* ctx, double out_ms[3]);

/* ---- Point-record ingest (csrc/record_ingest.hip: rec_count_kernel, rec_scatter_kernel). The reference never sees a range image: its
 * scans arrive as sensor_msgs::PointCloud2 blobs of driver-specific point records — velodyne_ros::Point (float time, uint16 ring),
 * ouster_ros::Point (uint32 t, uint8 ring), rslidar_ros::Point (double timestamp, uint16 ring), LocUtils/include/LocUtils/common/
 * point_types.h:99-169 — and CloudConver::Conver (LocUtils/src/subscriber/cloud_subscriber.cpp:7-29 and :31-58) turns them into the
 * library's clouds: it drops non-finite points and points with PointDistance < 4.0, keeps the rest in input order and carries ring as
 * one byte (:51). These entry points take the raw record blob as it is — the host copies it once and never touches a field — and do
 * that on the device, for all scans of a batch in one pass; the *_deskew forms also move every survivor into the sensor frame of a
 * reference instant by math::PoseInterp (LocUtils/include/LocUtils/common/math_utils.h:470-517) at THAT POINT's own time: the rule of
 * the block above, per point instead of per column.
 *
 * Field reads. A layout says where the fields of a record are. A field may sit at any byte offset in a record of any stride (22-byte
 * packed Velodyne records put a float32 at offset 18); it is read as memcpy would read it, little-endian. A U16 ring becomes
 * (uint8_t)ring as cloud_subscriber.cpp:51 does, which keeps the low byte.
 * Raw point: the three consecutive float32 at xyz_offset.
 * Conver's rules (cloud_subscriber.cpp:7-29): a point is dropped if x, y or z is not finite, or if sqrtf((x*x + y*y) + z*z) < min_range,
 * every product and sum rounded to float32 — the one device copy of the rule that the range-image decode uses.
 * Output of a scan: its survivors IN INPUT ORDER as {x, y, z, +0.0f}. With ring_kind != LOCGPU_RING_NONE one ring byte per survivor
 * stays resident with the batch under the contract of locgpu_batch_upload_ranges: locgpu_batch_download_rings and
 * locgpu_batch_loam_extract_resident work on them and the same later calls drop them; with LOCGPU_RING_NONE the batch holds no rings.
 * The cloud forms also carry intensity in the fourth lane (F32 as it is, U8 converted to float, NONE gives +0) and set is_dense = 1.
 * A survivor's position is the number of survivors before it in input order — integer sums in a fixed order, no atomics — so counts,
 * order and bits depend neither on n_scans, nor on a scan's place in the batch, nor on the run.
 * Point time (deskew forms): tp = (double)field * time_scale + time_offsets[i], two IEEE double operations, not fused; that float64
 * value IS the point's time. velodyne_ros::Point: F32, scale 1, offset = the scan's stamp on the knots' clock; ouster_ros::Point: U32,
 * scale 1e-9; rslidar_ros::Point: F64, scale 1, offset 0 or minus an epoch.
 * Pose and matrix: the pose at tp and at ref_times[i] is PoseInterp's rule as the block above states it (math_utils.h:470-517) with tp in
 * place of a column time; M = [ R_r^T R_p | R_r^T (t_p - t_r) ] as there; the survivor is stored as locgpu_cloud_transform's arithmetic
 * gives it with M. Conver's rules see the RAW point, so survivors, order, counts and ring bytes are those of the plain call on the same
 * records. With every knot the pose (0,0,0,1, 0,0,0) the deskew call leaves the plain call's bytes.
 * Time refusals: the host does not walk the points, so the count kernel decides. A SURVIVOR is bad if tp is not finite, if
 * tp < t[i][0], or if tp - t[i][K-1] > 0.5 (PoseInterp's time_th); dropped points may hold any garbage in their time field. If a scan has
 * a bad survivor, out_status[i] = 1, the call returns LOCGPU_ERR_INVALID, the text names the first such scan and how many of its
 * survivors were bad, and the destination is exactly as it was (points, counts and rings): nothing is scattered when the verdict is 0,
 * the mechanism of the capacity refusal. The reference-time bounds are decided on the host, as in the block above.
 * Other refusals (LOCGPU_ERR_INVALID, with a text), all decided on the host before any launch: every refusal of
 * locgpu_batch_upload_ranges (sharded and shared-source batches, an alignment begun and not ended, capacity — out_counts returned,
 * batch untouched); a NULL layout; stride_bytes outside 12..64; a field with offset + size > stride_bytes; a field that overlaps xyz; an
 * unknown kind; LOCGPU_TIME_NONE with a deskew call; a min_range that is not finite or negative; a time_scale that is not finite or 0;
 * n_points[i] < 0 or above 16 x the batch's max_points_per_scan (a sanity bound before staging is sized, not the capacity rule); NULL
 * records, or a NULL records[i] with n_points[i] > 0; a non-finite time_offsets[i]; and the motion's refusals (K out of 2..256, knot
 * times not finite or not strictly increasing, a reference time that is not finite, before the first knot or more than 0.5 s behind
 * the last, NULL members), decided by the host function the range-image path uses.
 * Out of scope: an asynchronous form; sharded and shared-source batches; the C++ facade (Conver lives in the ROS subscriber,
 * cloud_subscriber.cpp, which is not shadowed); bench.py; for the cloud forms, estimating the motion and compensating a scan again once
 * it is decoded (batches: "Deskew of a resident batch" below); big-endian blobs; strides above 64. */
enum { LOCGPU_TIME_NONE = 0, LOCGPU_TIME_F32 = 1, LOCGPU_TIME_F64 = 2, LOCGPU_TIME_U32 = 3 };
enum { LOCGPU_RING_NONE = 0, LOCGPU_RING_U8 = 1, LOCGPU_RING_U16 = 2 };
enum { LOCGPU_INTENSITY_NONE = 0, LOCGPU_INTENSITY_F32 = 1, LOCGPU_INTENSITY_U8 = 2 };
typedef struct locgpu_point_layout {
    uint32_t stride_bytes;                     /* 12..64, any value (PointCloud2::point_step) */
    uint32_t xyz_offset;                       /* three consecutive little-endian float32 */
    uint32_t time_offset, time_kind;
    uint32_t ring_offset, ring_kind;
    uint32_t intensity_offset, intensity_kind; /* cloud forms only; a batch's fourth lane stays +0 */
    float    min_range;                        /* finite, >= 0; the reference's value is 4.0f */
    uint32_t reserved;
    double   time_scale;                       /* finite, != 0: seconds per unit of the time field */
} locgpu_point_layout;
/* Conver on the device for n_scans record blobs (cloud_subscriber.cpp:7-29 and :31-58; PoseInterp, math_utils.h:470-517, is not
 * applied): scan i becomes the output defined above for the n_points[i] records at records[i]. Blocking: the blobs are free again when
 * it returns. One pass for all scans — raw bytes through pinned staging to HBM on the context's copy stream, then count, exclusive sum,
 * verdict and scatter kernels and one read-back. out_counts (n_scans entries or NULL) = the survivors per scan. */
LOCGPU_API int locgpu_batch_upload_records(locgpu_batch* b, const locgpu_point_layout* layout, const void* const* records /* n_scans */,
                                           const int64_t* n_points /* n_scans */, int32_t* out_counts /* n_scans or NULL */);
/* locgpu_batch_upload_records (Conver's survivors, cloud_subscriber.cpp:7-29) with every survivor moved into the sensor frame of
 * ref_times[i] by the pose at its own time (PoseInterp, math_utils.h:470-517), as defined above. time_offsets: n_scans doubles.
 * out_status (n_scans entries or NULL): 1 for a scan with a refused survivor time, else 0. */
LOCGPU_API int locgpu_batch_upload_records_deskew(locgpu_batch* b, const locgpu_point_layout* layout, const void* const* records /* n_scans */,
                                                  const int64_t* n_points /* n_scans */, const double* time_offsets /* n_scans */,
                                                  const locgpu_sweep_motion* motion, int32_t* out_counts /* n_scans or NULL */,
                                                  int32_t* out_status /* n_scans or NULL */);
/* The streaming Lio form (cloud_subscriber.cpp:7-29 and :31-58; no PoseInterp, math_utils.h:470-517): ONE blob of n records into a
 * resident cloud, equal to the batch form's scan byte for byte in x, y, z, with the intensity in the fourth lane and is_dense = 1.
 * ring_out (n bytes of room, or NULL) receives the survivors' ring bytes (it is not written with LOCGPU_RING_NONE); *n_out (optional) = their
 * number. The cloud has room for every record: this form has no capacity refusal; n must not exceed 2^31 - 1. */
LOCGPU_API int locgpu_cloud_upload_records(locgpu_cloud* c, const locgpu_point_layout* layout, const void* records, int64_t n, uint8_t* ring_out /* n or NULL */,
                                           size_t* n_out);
/* locgpu_cloud_upload_records (cloud_subscriber.cpp:7-29) with the motion of ONE scan (math_utils.h:470-517; knot_times [K], knot_poses
 * [K][7], ref_times [1]); equal to the batch form's scan byte for byte. A refusal leaves the cloud as it was. */
LOCGPU_API int locgpu_cloud_upload_records_deskew(locgpu_cloud* c, const locgpu_point_layout* layout, const void* records, int64_t n, double time_offset,
                                                  const locgpu_sweep_motion* motion, uint8_t* ring_out /* n or NULL */, size_t* n_out);
/* For tests and tools, as locgpu_range_deskew_matrices: with on != 0 the context's next locgpu_*_upload_records_deskew calls also store
 * each survivor's matrix (PoseInterp at the point's time, math_utils.h:470-517, for Conver's survivors, cloud_subscriber.cpp:7-29), 12
 * doubles = 96 B per point slot of the destination, in a grow-only table on the context. Off (the default): nothing is stored or
 * allocated. */
LOCGPU_API int locgpu_records_deskew_debug(locgpu_ctx* ctx, int on);
/* The matrices of scan `scan` of the context's most recent deskewed record call that ran with the debug switch on (math_utils.h:470-517,
 * cloud_subscriber.cpp:7-29), one per survivor in output order, n * 12 doubles. *n_out (optional) = n; out == NULL returns it alone.
 * LOCGPU_ERR_INVALID before any such call, for a scan index out of range and capacity < n * 12. */
LOCGPU_API int locgpu_records_deskew_matrices(locgpu_ctx* ctx, int scan, double* out /* n * 12 */, size_t capacity, size_t* n_out);
/* Measurement (tools/record_ingest_time.py): with locgpu_profile_enable on, out_ms[0] = the copy stream's time and out_ms[1] = the
 * kernels' time of the most recent locgpu_*_upload_records[_deskew] (Conver, cloud_subscriber.cpp:7-29; PoseInterp, math_utils.h:470-517).
 * Zeros before the first profiled call. locgpu_range_ingest_times and locgpu_range_deskew_times are left alone. */
LOCGPU_API int locgpu_records_ingest_times(locgpu_ctx* ctx, double out_ms[2]);

/* ---- Deskew of a resident batch (csrc/resident_deskew.hip: rsd_check_kernel, rsd_move_kernel). The two deskewed ingest blocks above
 * need the sweep motion BEFORE the scan is uploaded, and the caller has it only afterwards: it is what the alignment of that same scan
 * yields. The reference forms it from the last two results, predict_pos = result_pos * last_pose.inverse() * result_pos (loc.cpp:232,
 * lio.cpp:465). So the standard two-pass — align the skewed scan, derive the motion, compensate, re-align or merge — had to send the
 * raw bytes over PCIe twice, and that copy is the whole cost of an ingest call. The raw survivors are already resident; what a plain
 * ingest throws away is 8 bytes per point, its time. This block keeps them on request, adds the pass that uses them and the host
 * function that turns a pose sequence into a locgpu_sweep_motion: ingest once, align, compensate, re-align or locgpu_batch_merge,
 * without a second host-to-device copy. A caller who does not opt in sees no change: nothing is allocated, every call leaves the
 * bytes it left before.
 *
 * Resident times. locgpu_batch_keep_times(b, 1) turns time keeping on for a batch (off by default). With it on, the PLAIN ingest calls
 * leave one float64 time KEY per survivor beside the ring bytes, [n_scans][max_points_per_scan], allocated on first use:
 *   locgpu_batch_upload_records with time_kind != LOCGPU_TIME_NONE: key = (double)field * time_scale, the first of the two IEEE
 *     operations of "Point time" above; the offset is added by the pass;
 *   locgpu_batch_upload_ranges with a sensor that has column times (locgpu_sensor_set_col_times): key = col_time[c] of the survivor's
 *     column c.
 * A layout without a time field or a sensor without column times leaves no times (the ingest itself succeeds as before); the *_deskew
 * ingest forms never leave times: their points are no longer raw. Everything that drops the resident rings drops the times too (any
 * other upload, locgpu_batch_preprocess into the batch, the feature picker's destinations), and so does a later ingest that leaves none.
 * The pass, for every survivor of every scan i of src: tp = key + time_offsets[i] (one IEEE double addition; time_offsets == NULL:
 * tp = key and nothing is added); the pose at tp and at ref_times[i] by PoseInterp's rule (math_utils.h:470-517) as "Range-image ingest,
 * motion-compensated" states it; M = [ R_r^T R_p | R_r^T (t_p - t_r) ] as there; the point stored as locgpu_cloud_transform's
 * arithmetic gives it with M, the w lane +0 — through the SAME device function as the per-point deskew of the record ingest, so the
 * bytes are those of locgpu_batch_upload_records_deskew (locgpu_batch_upload_ranges_deskew) for the same scans, offsets and motion. A
 * point keeps its place: no atomics, and nothing depends on n_scans or on a scan's place in the batch.
 * dst == src compensates in place. Otherwise dst must hold the same number of scans and have room for every count of src; it receives
 * the counts and, when src holds them, the ring bytes of src, so locgpu_batch_loam_extract_resident(dst, ...) works, and src keeps its
 * raw points and times: it can be compensated again with a better motion. After the call dst never holds times: compensating
 * compensated points is refused.
 * Time refusals follow the ingest's mechanism: a check kernel counts the bad survivors of every scan first — tp not finite,
 * tp < t[i][0], or tp - t[i][K-1] > 0.5 (PoseInterp's time_th) — and if any scan has one, out_status[i] = 1 for each such scan, the call
 * returns LOCGPU_ERR_INVALID, the text names the first such scan and its count, and dst is exactly as it was (points, counts and
 * rings), also when dst == src.
 * Other refusals (LOCGPU_ERR_INVALID, with a text), decided on the host before any launch: a NULL batch; batches of different
 * contexts; sharded or shared-source batches; an alignment begun and not ended on either batch; no resident times in src; different
 * numbers of scans; every motion refusal of locgpu_batch_upload_ranges_deskew (the same host function; the reference times are bounded
 * there); a non-finite time_offsets[i]; a scan of src with more points than dst has room for (dst is unchanged).
 * Out of scope: the locgpu_cloud_* forms; the C++ facade; bench.py; an asynchronous form; sharded batches; estimating the motion from
 * anything but poses. */
/* Time keeping of a batch on (on != 0) or off (the default), for the survivors Conver keeps (cloud_subscriber.cpp:7-29) and PoseInterp's
 * later use of their times (math_utils.h:470-517). Off: the times the batch holds are freed. LOCGPU_ERR_INVALID for a NULL, sharded or
 * shared-source batch and for one whose alignment has been begun and not ended. */
LOCGPU_API int locgpu_batch_keep_times(locgpu_batch* b, int on);
/* For tests and tools, as locgpu_batch_download_rings: the resident time keys of scan `scan` (the times PoseInterp is asked at,
 * math_utils.h:470-517, of Conver's survivors, cloud_subscriber.cpp:7-29), one double per point. *n (optional) = the scan's size;
 * out == NULL returns it alone. LOCGPU_ERR_INVALID when the batch holds no times, for a scan index out of range and capacity < n. */
LOCGPU_API int locgpu_batch_download_times(locgpu_batch* b, int scan, double* out, size_t capacity, size_t* n);
/* The pass defined above: every survivor of src (Conver's, cloud_subscriber.cpp:7-29) moved into the sensor frame of ref_times[i] by the
 * pose at its own time (PoseInterp, math_utils.h:470-517), into dst (dst == src: in place). The motion is typically
 * locgpu_motion_from_poses' (loc.cpp:232). Blocking. Two kernels of this file round the ingest's sum and verdict kernels: the check
 * (8 B per point in) and the move (16 B + 8 B in, 16 B out per point; the scan's knots staged in LDS). */
LOCGPU_API int locgpu_batch_deskew(locgpu_batch* src, locgpu_batch* dst, const double* time_offsets /* n_scans or NULL */,
                                   const locgpu_sweep_motion* motion, int32_t* out_status /* n_scans or NULL */);
/* Measurement (tools/resident_deskew_time.py): with locgpu_profile_enable on, out_ms[0] = the check kernel's time and out_ms[1] = the
 * move kernel's time (PoseInterp, math_utils.h:470-517, on Conver's survivors, cloud_subscriber.cpp:7-29) of the most recent
 * locgpu_batch_deskew. Zeros before the first profiled call. */
LOCGPU_API int locgpu_batch_deskew_times(locgpu_ctx* ctx, double out_ms[2]);
/* The motion of n consecutive scans from their poses — host only, no launch, FP64, nothing normalised. poses [n][7] (quaternion xyzw,
 * then translation: the matcher's results) and stamps [n] (strictly increasing) in; knot_times [n][3] and knot_poses [n][3][7] out:
 * scan i gets K = 3 knots, the poses and stamps of scans i-1, i, i+1, which cover start-stamped and end-stamped sensors alike
 * (PoseInterp, math_utils.h:470-517, then interpolates between them; the points are Conver's, cloud_subscriber.cpp:7-29). A missing
 * neighbour is extrapolated at constant velocity with the reference's own expression predict_pos = result_pos * last_pose.inverse() *
 * result_pos (loc.cpp:232): after the last scan the pose (T[n-1] * inv(T[n-2])) * T[n-1] at time 2.0 * t[n-1] - t[n-2]; before the
 * first the pose (T[0] * inv(T[1])) * T[0] at time 2.0 * t[0] - t[1]. The caller fills ref_times itself.
 * Arithmetic, one IEEE double operation per written operation, in this order (q = x, y, z, w; R(q) = Eigen's toRotationMatrix:
 *   tx = 2 x, ty = 2 y, tz = 2 z; twx = tx w, twy = ty w, twz = tz w; txx = tx x, txy = ty x, txz = tz x; tyy = ty y, tyz = tz y,
 *   tzz = tz z; R = [1 - (tyy + tzz), txy - twz, txz + twy; txy + twz, 1 - (txx + tzz), tyz - twx; txz - twy, tyz + twx, 1 - (txx + tyy)]):
 *   a (x) b:  w = ((aw bw - ax bx) - ay by) - az bz;  x = ((aw bx + ax bw) + ay bz) - az by;
 *             y = ((aw by + ay bw) + az bx) - ax bz;  z = ((aw bz + az bw) + ax by) - ay bx;
 *   R v:      row r = (R[r][0] v0 + R[r][1] v1) + R[r][2] v2;
 *   inv(q, t) = (c, -(R(c) t)) with c = (-x, -y, -z, w);
 *   (q1, t1) * (q2, t2) = (q1 (x) q2, t1 + R(q1) t2), each component t1[r] + (R(q1) t2)[r].
 * LOCGPU_ERR_INVALID, with a text (locgpu_last_error(NULL)), for n < 2, a NULL array, or stamps that are not finite or not increasing. */
LOCGPU_API int locgpu_motion_from_poses(const double* poses /* n * 7 */, const double* stamps /* n */, int n, double* knot_times /* n * 3 */,
                                        double* knot_poses /* n * 3 * 7 */);

/* The local map of Lio::AddCloud's keyframe branch (lio.cpp:268-306), kept in HBM: a queue of at most num_kfs world-frame
 * keyframe clouds (scans_in_local_map_) and the voxel-filtered local map (local_map_) that is the next matching target.
 * add_keyframe(scan, pose): key_frame_scan = transform(scan, pose) (pose NULL: scan is already in the world frame); push;
 * when the queue exceeds num_kfs drop the oldest and rebuild the map from the retained keyframes, otherwise append the new
 * one to the (already filtered) map; then voxel-filter the map in place. The caller then hands locgpu_submap_cloud() to
 * locgpu_icp_set_target_cloud / locgpu_ndt_set_target_cloud (or the new keyframe alone for INCREMENTAL_NDT, lio.cpp:301-304). */
LOCGPU_API int locgpu_submap_create(locgpu_ctx* ctx, int num_kfs, float leaf, locgpu_submap** out);
LOCGPU_API void locgpu_submap_destroy(locgpu_submap* m);
LOCGPU_API int locgpu_submap_add_keyframe(locgpu_submap* m, const locgpu_cloud* scan, const double pose[7]);
LOCGPU_API int locgpu_submap_cloud(locgpu_submap* m, locgpu_cloud** map);          /* borrowed: owned by the submap */
LOCGPU_API int locgpu_submap_last_keyframe(locgpu_submap* m, locgpu_cloud** kf);   /* borrowed: the newest world-frame keyframe */
LOCGPU_API int locgpu_submap_info(const locgpu_submap* m, int* n_keyframes, size_t* map_points);

/* ---- The LOAM matcher on resident clouds: Lio::AddCloud(FullCloudPtr) (lio.cpp:311-410) with AlignWithLocalMap(edge, surf) (:475-502)
 * without a PCIe hop between the feature picker (locgpu_cloud_loam_extract), the voxel filter, the match and the pair of local maps.
 * Every cloud argument may belong to ANY context on the handle's GPU — a plain locgpu_ctx front-end context included: the rule
 * "a cloud of context A may be the source on context B" above. The handle's stream is ordered behind the call that produced each
 * cloud; a cloud on another GPU is refused with LOCGPU_ERR_INVALID. Eager only, like every LOAM entry point: no graph argument. */
/* LoamRegistration::SetInputTarget (loam_registration.cpp:22-36) from resident clouds: every ENABLED class's
 * locgpu_icp_set_target_cloud. Semantics of locgpu_loam_set_target: a switched-off class's cloud may be NULL, LOCGPU_OK only if every
 * enabled class was ingested, a class that failed has no target afterwards. */
LOCGPU_API int locgpu_loam_set_target_cloud(locgpu_loam* l, const locgpu_cloud* edge_map, const locgpu_cloud* surf_map);
/* The same (loam_registration.cpp:22-36; Lio re-ingests both maps every keyframe, lio.cpp:408) with both host tree builds on worker
 * threads, under the rules of locgpu_icp_set_target_cloud_async: returns once the clouds are copied out, the previous targets stay in
 * place until the ingest finishes inside the next call that reads the target (match, H/B, fitness), which also reports its errors. */
LOCGPU_API int locgpu_loam_set_target_cloud_async(locgpu_loam* l, const locgpu_cloud* edge_map, const locgpu_cloud* surf_map);
/* LoamRegistration::ScanMatch WHOLE (loam_registration.cpp:38-99) on resident feature clouds: locgpu_loam_scan_match without the
 * upload — the scans are NOT copied, the kernels read them where the clouds hold them (they must not be modified during the call).
 * result_pose is IN-OUT and stats are as there: with status 3 / 4 the caller's result_pose and `out` are left untouched and the call
 * returns LOCGPU_OK. out (optional): receives n_edge + n_surf points, the edge points followed by the surface points (:93-95), x, y, z
 * under pose.matrix().cast<float>() (:96) in the rounding order of locgpu_loam_scan_match's output cloud, the intensity lane carried
 * through, is_dense = the AND of the inputs' flags; written on the device, never staged on the host. out must be distinct from edge
 * and surf. A switched-off class's cloud may be NULL; when it is given its points still join `out`. */
LOCGPU_API int locgpu_loam_scan_match_cloud(locgpu_loam* l, const locgpu_cloud* edge, const locgpu_cloud* surf, const double init_pose[7],
                                            double result_pose[7], locgpu_align_stats* stats, locgpu_cloud* out);
/* MatchingInterface::GetFitnessScore for the LOAM matcher (the reference's ScanMatch, loam_registration.cpp:38-99, computes none):
 * out[0] = surface, out[1] = edge, each exactly locgpu_icp_fitness of that class's scan against that class's map under `pose` —
 * exact nearest neighbour, fixed reduction order. No joint number here (locgpu_loam_fitness defines and gives one). The scans are the ones
 * the handle's most recent single-scan call left in HBM: locgpu_loam_scan_match / locgpu_loam_hb (the handle's own copies) or
 * locgpu_loam_scan_match_cloud — which keeps REFERENCES, so those two clouds must still be alive and unmodified. A switched-off
 * class (and an empty scan) reports {+inf, 0, 0}. LOCGPU_ERR_INVALID when nothing is resident (no such call yet, or a
 * locgpu_loam_align_batch / locgpu_loam_align_batches since); LOCGPU_ERR_NO_TARGET without a target. */
LOCGPU_API int locgpu_loam_fitness_resident(locgpu_loam* l, const double pose[7], double max_range, locgpu_fitness out[2]);
/* locgpu_loam_fitness and locgpu_loam_init_search on resident feature clouds: the same bits without the uploads. The scans are NOT
 * copied — every entry of a class reads its cloud where it lies, so the clouds must not be modified during the call. A switched-off
 * class's cloud may be NULL; a cloud on another GPU is refused with LOCGPU_ERR_INVALID before anything is enqueued. This is the LOAM
 * matcher's shared-source resident form: one pair of scans under many poses (n different scans: locgpu_loam_align_batches below). */
LOCGPU_API int locgpu_loam_fitness_cloud(locgpu_loam* l, const locgpu_cloud* edge, const locgpu_cloud* surf, const double* poses, int n_poses,
                                         double max_range, locgpu_fitness* out /* n_poses × 3 */);
LOCGPU_API int locgpu_loam_init_search_cloud(locgpu_loam* l, const locgpu_cloud* edge, const locgpu_cloud* surf, const double* candidates, int m,
                                             const locgpu_init_search_opts* sopts, double* out_poses, locgpu_fitness* out_fit /* m × 3 */,
                                             locgpu_align_stats* stats, int* best);

/* The PAIR of local maps of Lio::AddCloud(FullCloudPtr) (lio.cpp:331-409) in HBM: local_map_edge_ / local_map_surf_ with their queues
 * edge_scans_in_local_map_ / surf_scans_in_local_map_ — one queue length (num_kfs) for both, pushed and popped together (:382-388) —
 * as two locgpu_submap. add_keyframe(edge, surf, pose): both clouds go through the DOUBLE-precision matrix (:343-344, :379-380; what
 * locgpu_cloud_transform does) and join their queues and maps. Two details of the reference, restated:
 *  (a) The FIRST keyframe seeds both maps UNFILTERED: :338-339 filter the still-empty maps, :348-349 then assign the transformed
 *      scans, and the first target is those scans (:346). So the first add_keyframe does not voxel-filter; every later one appends
 *      (:399-403) or drops the oldest and rebuilds (:385-398), then filters both maps in place (:405-406).
 *  (b) Which cloud a keyframe is made of is the CALLER's: the submap takes what it is handed. In the reference the first keyframe is
 *      made of the picker's UNFILTERED features (AddCloud returns at :356, before AlignWithLocalMap at :359), every later one of the
 *      voxel-FILTERED features, because AlignWithLocalMap filters edge_cloud and surf_cloud in place through the shared pointers
 *      (:485-486) before :379-380 transform them. A caller that mirrors Lio hands the picker's clouds first and the filtered ones
 *      (the clouds it matched) from then on.
 * pose NULL: the clouds are already in the world frame. Both clouds are required (an empty one is fine) and may belong to any context
 * on the submap's GPU. The caller then hands locgpu_loam_submap_clouds() to locgpu_loam_set_target_cloud[_async] (:346, :408). After a
 * failed add_keyframe the two queues may differ: destroy the submap. */
typedef struct locgpu_loam_submap locgpu_loam_submap;
LOCGPU_API int locgpu_loam_submap_create(locgpu_ctx* ctx, int num_kfs, float leaf, locgpu_loam_submap** out);
LOCGPU_API void locgpu_loam_submap_destroy(locgpu_loam_submap* m);
LOCGPU_API int locgpu_loam_submap_add_keyframe(locgpu_loam_submap* m, const locgpu_cloud* edge, const locgpu_cloud* surf, const double pose[7]);
LOCGPU_API int locgpu_loam_submap_clouds(locgpu_loam_submap* m, locgpu_cloud** edge_map, locgpu_cloud** surf_map); /* borrowed */
LOCGPU_API int locgpu_loam_submap_info(const locgpu_loam_submap* m, int* n_keyframes, size_t* edge_points, size_t* surf_points);

/* ---- The global map (csrc/cloud_merge.hip): Lio::GetGlobalMap (lio.cpp:550-614: the cloud form :550-580, the LOAM edge / surface pair
 * :582-614), which SaveGlobalMap (:131-207) calls — the product of a mapping run. The reference takes every saved keyframe (the RAW
 * scan: lio.cpp:254, :275) through pcl::transformPointCloud(kf, kf, estimated_poses_[i].matrix()) (:571, the DOUBLE 4x4), joins them
 * with `*global_map += *kf` and runs ONE VoxelFilter::Filter (voxel_filter.cpp:19-25) over the sum. locgpu_clouds_merge does that for n
 * resident clouds with one transform-and-join launch, whatever n is, and the existing filter: `out` is, byte for byte — x, y, z, the
 * intensity lane, the count, is_dense and *passthrough — what
 *     acc = a fresh cloud;  for i in 0..n-1: locgpu_cloud_append(acc, locgpu_cloud_transform(clouds[i], poses + 7 i));
 *     locgpu_cloud_voxel_filter(acc, leaf, out, passthrough)
 * leaves, without the n temporaries, the n launches and the n copies. The arithmetic is locgpu_cloud_transform's (one device function
 * serves both): per row (float)(((m0 x + m1 y) + m2 z) + m3) in double, a non-finite point of a cloud that is not flagged dense left
 * as it is, the intensity lane carried through — and then averaged per voxel by the filter, as PCL does.
 *   poses == NULL: the clouds are already in the world frame; no arithmetic touches them, the bits are carried through.
 *   leaf == 0: join only — `out` is the joined cloud (non-finite points kept, is_dense = the AND of the inputs' flags) and
 *     *passthrough = 0. SaveGlobalMap builds its LOAM edge-plus-surface cloud this way before it filters.
 * Clouds of any context on ctx's GPU are accepted (the rule of locgpu_batch_upload_clouds: ctx's stream is ordered behind what their
 * contexts have enqueued; the call is blocking and the clouds are free again when it returns). Empty clouds may stand anywhere in the
 * list. `out` belongs to ctx and is none of the inputs. The call returns when out's count is known on the host.
 * LOCGPU_ERR_INVALID, with a text and with `out` exactly as it was (points, count and flag), for a NULL ctx, clouds, out or clouds[i],
 * n < 1, leaf < 0 or not finite, out among the inputs or of another context, a cloud on another GPU, and more than 0x7FFFFF00 points
 * in total (a cloud's limit); all of these are checked before any device is touched. Scratch is grow-only on the context: the joined
 * cloud (16 B per point) and 124 B per cloud, beside the filter's own. */
LOCGPU_API int locgpu_clouds_merge(locgpu_ctx* ctx, const locgpu_cloud* const* clouds, const double* poses /* n x 7 or NULL */, int n, float leaf,
                                   locgpu_cloud* out, int* passthrough /* optional */);
/* The same for the scans of a batch — what closes the batched loop: scans registered against a prior map with locgpu_icp_align_batch,
 * locgpu_ndt_align_batch or locgpu_loam_align_batches are folded, under the poses that came out, into the next target
 * (locgpu_icp_set_target_cloud, locgpu_ndt_set_target_cloud, locgpu_loam_set_target_cloud) without a trip through host memory. The
 * result equals locgpu_clouds_merge on the clouds locgpu_batch_export_cloud makes of the scans, in scan order: scan s is a cloud of its
 * count points {x, y, z, 0} that is NOT flagged dense (a batch carries no flag — the rule of locgpu_batch_preprocess), so a batch
 * scan's intensity is 0: batches do not carry one, whereas a map built from clouds keeps and averages intensity as PCL does.
 * poses: n_scans x 7 (indexed by scan, whatever `use` says) or NULL. use (n_scans bytes or NULL): a scan with use[s] == 0 contributes
 * nothing — alignments that locgpu_icp_fitness_batch / locgpu_ndt_fitness_batch rejected stay out of the map; with no scan in use
 * `out` comes out empty and dense. `out` belongs to the batch's context. The batch is not modified; a pending upload is waited for.
 * Refusals (LOCGPU_ERR_INVALID, `out` as it was): those of locgpu_batch_download_scan (shared-source batch, alignment begun and not
 * ended), a sharded batch, a NULL batch or out, and the leaf and size rules above. */
LOCGPU_API int locgpu_batch_merge(locgpu_batch* b, const double* poses /* n_scans x 7 or NULL */, const uint8_t* use /* n_scans or NULL */, float leaf,
                                  locgpu_cloud* out, int* passthrough /* optional */);
/* Scan `scan` of a batch as a resident cloud: the device-to-device inverse of locgpu_batch_upload_clouds. `cloud`, of any context on the
 * batch's GPU, receives the scan's points {x, y, z, 0} with is_dense = 0; locgpu_batch_upload_clouds of the exported clouds reproduces
 * the scans' bytes and counts. It makes a batch scan usable as a keyframe of locgpu_submap_add_keyframe. Blocking. Refusals: those of
 * locgpu_batch_download_scan (scan index out of range, shared-source batch, alignment begun and not ended), a NULL batch or cloud, a
 * cloud on another GPU. */
LOCGPU_API int locgpu_batch_export_cloud(locgpu_batch* b, int scan, locgpu_cloud* cloud);

/* =====================================================================================================================
 * ---- Pairwise batch ICP: every scan of a batch against a target of its own.
 *
 * The reference's scan-to-scan odometry (slam_demo/src/apps/test_node.cpp:256-315; two PCD files: :437-460) runs, per scan,
 * SetInputTarget(last_cloud) (icp_registration.cpp:9-29), ScanMatch(current_cloud, SE3(), ...) (icp_registration.cpp:216-244) and
 * T_w_lc = T_w_lc * T_lc_ln. The initial pose is the identity every time, so the pairs (scan i, scan i-1) of a whole log are
 * independent of each other. Here n targets are ingested as a FOREST — n KD-trees, each slot for slot what locgpu_icp_set_target
 * builds for that cloud alone, packed behind one another in one device array — and one call aligns every scan of a batch against
 * the tree it names. The same call with a score per pair verifies k loop-closure candidates.
 *
 * Limits of a forest: 1 <= n_targets; every target is what locgpu_icp_set_target accepts (non-empty, stride >= 12, tree depth <= 64);
 * all trees together, with a two-slot sentinel leaf behind each and a slot of padding where a tree would start at an odd slot, stay
 * below 2^29 slots of 8 bytes (4 GiB: what ONE tree may hold), so 3 points' worth of slots per point: about 178 M points in all.
 * A refused ingest leaves the context exactly as it was and names the target's index in locgpu_last_error.
 *
 * A context that holds a forest answers only the calls of this block, and locgpu_icp_set_target* (any form), which replaces the
 * forest and makes the context ordinary again. Every other entry point that reads the ICP target — locgpu_knn, locgpu_icp_align*,
 * locgpu_icp_hb*, locgpu_icp_scan_match, locgpu_icp_fitness*, locgpu_icp_init_search, locgpu_pool_*, the map planes, the grid search
 * mode, locgpu_loam_create_on and the calls of a LOAM handle on such a context — returns LOCGPU_ERR_INVALID with a text that says
 * so; an ordinary context refuses locgpu_icp_align_pairs / locgpu_icp_fitness_pairs the same way. locgpu_icp_target_info reports the
 * forest's totals (depth: the largest). locgpu_debug_batch_nn after a pairs call reports point indices of each scan's OWN target.
 *
 * Not covered by this block: NDT and LOAM pairs (NDT pairs have the block behind this one; LOAM pairs are not covered at all),
 * scan pools, hipGraph replay, sharded and shared-source batches, the C++ facade, bench.py, an asynchronous (begin / end) form.
 * ===================================================================================================================== */

/* locgpu_align_stats::status of a scan that locgpu_icp_align_pairs was told not to align (target_of[i] == -1); used for nothing else. */
#define LOCGPU_STATUS_NO_PAIR_TARGET 5

/* SetInputTarget (icp_registration.cpp:9-29) of n_targets clouds at once, host pointers: pts[j] = n[j] points of stride_bytes each,
 * deep-copied before the call returns — the last_cloud of every pair of test_node.cpp:256-315. The trees are built on the host in
 * parallel across trees (each by one thread, in the reference's summation order) and go up in ONE host-to-device copy. Blocking.
 * LOCGPU_ERR_INVALID for NULL arrays, n_targets < 1, an empty target, stride < 12 and a forest beyond the size limit above;
 * LOCGPU_ERR_DEPTH for a tree deeper than 64 levels. */
LOCGPU_API int locgpu_icp_set_target_forest(locgpu_ctx* ctx, const void* const* pts, const size_t* n, int n_targets, size_t stride_bytes);
/* The same from a resident plain batch of this context: target j = scan j of `batch` (what locgpu_batch_preprocess left there, for
 * instance — the filtered clouds test_node.cpp:256-315 matches; SetInputTarget, icp_registration.cpp:9-29). The points reach the
 * host builder the way locgpu_icp_set_target_cloud brings a cloud's there: 16 B a point down, the packed trees up. The batch is not
 * modified and may be the source batch of the pairs call that follows. Refused (LOCGPU_ERR_INVALID): a NULL batch, a batch of another
 * context, sharded and shared-source batches, a batch with an alignment begun and not ended, an empty scan (its index is named). */
LOCGPU_API int locgpu_icp_set_target_forest_batch(locgpu_ctx* ctx, const locgpu_batch* batch);
/* *n_targets = trees of the forest; leaves[j] = KdTree::size_ of tree j (SetInputTarget, icp_registration.cpp:9-29), depth[j] = its
 * depth (root = level 1) — what locgpu_icp_target_info reports after locgpu_icp_set_target of that cloud alone. The two arrays have
 * n_targets entries each and may be NULL (call once with NULL arrays for the count). LOCGPU_ERR_INVALID (*n_targets = 0) when the
 * context holds an ordinary target, LOCGPU_ERR_NO_TARGET without any. */
LOCGPU_API int locgpu_icp_forest_info(const locgpu_ctx* ctx, int* n_targets, size_t* leaves, int* depth);
/* ScanMatch (icp_registration.cpp:216-244) of every scan of `batch` against target target_of[i] of the context's forest — the loop
 * body of test_node.cpp:256-315 (two clouds: :437-460) for all pairs in one call. init_poses: n_scans x 7, or NULL = the identity for
 * every scan, the reference's `SE3 init_pos` (test_node.cpp:289). target_of[i] == -1: scan i is not aligned — out_poses[i] is its
 * initial pose, stats[i].iterations = 0, stats[i].status = LOCGPU_STATUS_NO_PAIR_TARGET. Methods LOCGPU_P2P, LOCGPU_P2LINE,
 * LOCGPU_P2PLANE; `approximate` / ann_alpha as in locgpu_icp_align_batch; LOCGPU_P2PLANE_MAP and LOCGPU_SEARCH_GRID_EXACT are refused.
 * Scan i's pose and stats equal, bit for bit, row i of locgpu_icp_align_batch of the SAME batch on an ordinary context that holds
 * target target_of[i] alone (a batch splits its sums by its shape, so the shape matters). Blocking and eager: it runs eagerly whatever
 * locgpu_graph_enable was told and never touches the batch's captured graphs. Refused (LOCGPU_ERR_INVALID), with the batch untouched:
 * NULL arguments, a target_of entry < -1 or >= n_targets, sharded and shared-source batches, a batch of another context, a batch
 * with an alignment begun and not ended, an ordinary context. */
LOCGPU_API int locgpu_icp_align_pairs(locgpu_ctx* ctx, locgpu_batch* batch, const int* target_of, const double* init_poses /* n_scans x 7 or NULL */,
                                      const locgpu_icp_opts* opts, double* out_poses, locgpu_align_stats* stats /* n_scans or NULL */);
/* locgpu_icp_fitness_batch per pair: the score of scan i under poses[i] against target target_of[i] alone (the GetFitnessScore
 * definition above: exact nearest neighbour, k = 1), bit for bit what an ordinary context holding that target reports — the check a
 * caller makes after the ScanMatch of icp_registration.cpp:216-244 on each pair of test_node.cpp:256-315. target_of[i] == -1: {+inf, 0,
 * 0}. Refusals as locgpu_icp_align_pairs, and a NaN max_range. */
LOCGPU_API int locgpu_icp_fitness_pairs(locgpu_ctx* ctx, locgpu_batch* batch, const int* target_of, const double* poses, double max_range,
                                        locgpu_fitness* out);

/* =====================================================================================================================
 * ---- Pairwise batch NDT: every scan of a batch against a voxel grid of its own.
 *
 * The NDT form of the reference's scan-to-scan odometry (TestNdtMatching, slam_demo/src/apps/test_node.cpp:317-374) runs, per scan,
 * SetInputTarget(last_cloud) (:354; SetDirectNdtTargetCloud, ndt_registration.cpp:65-85, 87-148), ScanMatch(current_cloud, SE3(), ...)
 * (:356; ndt_registration.cpp:238-261, AlignNdt :374-464) and T_w_lc = T_w_lc * T_lc_ln. The initial pose is the identity every time
 * (:348), so the pairs of a whole log are independent. Here n targets are ingested as a voxel SET — one table in the layout of an
 * ordinary direct target whose 64-bit keys carry the target's index above the voxel (target:16 | x:16 | y:16 | z:16) — built ON THE
 * DEVICE in one pass for all targets, and one call aligns every scan of a batch against the grid it names. From a resident batch no
 * point crosses PCIe and nothing is built on the host.
 *
 * One locgpu_ndt_opts serves the whole set (voxel_size, min_pts_in_voxel, nearby_type, res_outlier_th and the loop's options);
 * method 1 (direct) only, the incremental method is refused. Every voxel of target j has, bit for bit, the mean and information
 * matrix locgpu_ndt_set_target of that cloud alone gives it. Limits of a set: 1 <= n_targets <= 65535; every target non-empty;
 * voxel coordinates strictly inside +-2^15 = 32768 voxels on every axis (an ordinary target: +-2^20) — a target with a point outside
 * is refused; at most 0x7FFFFF00 points in all. A refused ingest leaves the context exactly as it was and names the target's index
 * in locgpu_last_error.
 *
 * A context that holds a set answers only the calls of this block, and locgpu_ndt_set_target* (any form), which replaces the set
 * and makes the context ordinary again. Every other reader of the NDT target — locgpu_ndt_align*, locgpu_ndt_hb*,
 * locgpu_ndt_scan_match, locgpu_ndt_fitness*, locgpu_ndt_init_search, locgpu_ndt_dump, locgpu_pool_create with matcher = 1 and the
 * pool's re-check at submit — returns LOCGPU_ERR_INVALID with a text that says so; an ordinary context refuses
 * locgpu_ndt_align_pairs / locgpu_ndt_fitness_pairs the same way. The ICP target of the context is untouched either way.
 * locgpu_ndt_target_info reports the set's totals. The status of a scan without a target is LOCGPU_STATUS_NO_PAIR_TARGET, above.
 *
 * Not covered: LOAM pairs, incremental-NDT sets, scan pools, hipGraph replay, sharded and shared-source batches, the C++ facade,
 * bench.py, an asynchronous (begin / end) form.
 * ===================================================================================================================== */

/* SetInputTarget -> SetDirectNdtTargetCloud (ndt_registration.cpp:65-85, 87-148) of n_targets clouds at once, host pointers: pts[j] =
 * n[j] points of stride_bytes each, deep-copied before the call returns — the last_cloud of every pair of test_node.cpp:317-374. The
 * points go up in ONE host-to-device copy; keys, one stable sort, per-voxel mean / covariance / SVD run on the device. Blocking.
 * opts NULL = the defaults. LOCGPU_ERR_INVALID, context unchanged: NULL arrays, n_targets < 1 or > 65535, an empty target (its index
 * is named), stride < 12, the incremental method, a point outside the set's key range (target index named). */
LOCGPU_API int locgpu_ndt_set_target_set(locgpu_ctx* ctx, const void* const* pts, const size_t* n, int n_targets, size_t stride_bytes, const locgpu_ndt_opts* opts);
/* The same from a resident plain batch of this context: target j = scan j of `batch` (what locgpu_batch_preprocess left there, for
 * instance — the filtered clouds test_node.cpp:317-374 matches; SetDirectNdtTargetCloud, ndt_registration.cpp:65-85, 87-148). Device
 * only: the scans are read where the batch holds them. The batch is not modified and may be the source batch of the pairs call that
 * follows. Refused (LOCGPU_ERR_INVALID) in addition: a NULL batch, a batch of another context, sharded and shared-source batches, a
 * batch with an alignment begun and not ended, an empty scan (its index is named), more than 65535 scans. */
LOCGPU_API int locgpu_ndt_set_target_set_batch(locgpu_ctx* ctx, const locgpu_batch* batch, const locgpu_ndt_opts* opts);
/* *n_targets = targets of the set; points[j] = points of target j, voxels[j] = the voxels it keeps (count > min_pts_in_voxel,
 * SetDirectNdtTargetCloud, ndt_registration.cpp:87-148) — what locgpu_ndt_target_info reports as num_voxels after locgpu_ndt_set_target
 * of that cloud alone. The arrays have n_targets entries each and may be NULL (call once with NULL arrays for the count).
 * LOCGPU_ERR_INVALID (*n_targets = 0) when the context holds an ordinary NDT target, LOCGPU_ERR_NO_TARGET without any. */
LOCGPU_API int locgpu_ndt_set_info(const locgpu_ctx* ctx, int* n_targets, size_t* points /* [n] or NULL */, size_t* voxels /* [n] or NULL */);
/* locgpu_ndt_dump of ONE target of the set (the grids_ of SetDirectNdtTargetCloud, ndt_registration.cpp:87-148): keys (cap x 3 voxel
 * coordinates, without the target), mu (cap x 3), info (cap x 9), in ascending (x, y, z) key order — the same bytes in the same order
 * after every ingest of the same set. *n_out = voxels of the target. Test read-back. */
LOCGPU_API int locgpu_ndt_set_dump(locgpu_ctx* ctx, int target, int32_t* keys, double* mu, double* info, size_t cap, size_t* n_out);
/* ScanMatch (ndt_registration.cpp:238-261; AlignNdt, :374-464) of every scan of `batch` against target target_of[i] of the context's
 * voxel set — the loop body of test_node.cpp:317-374 for all pairs in one call. init_poses: n_scans x 7, or NULL = the identity for
 * every scan, the reference's `SE3 init_pos` (test_node.cpp:348). target_of[i] == -1: scan i is not aligned — out_poses[i] is its
 * initial pose, stats[i].iterations = 0, stats[i].status = LOCGPU_STATUS_NO_PAIR_TARGET. Scan i's pose and stats equal, bit for bit,
 * row i of locgpu_ndt_align_batch of the SAME batch on an ordinary context that holds target target_of[i] alone (locgpu_ndt_set_target,
 * same options) — status 1 (det(H) == 0, ndt_registration.cpp:435-436: the caller's pose stays) included. Blocking and eager: it runs
 * eagerly whatever locgpu_graph_enable was told. Refused (LOCGPU_ERR_INVALID), with the batch untouched: NULL arguments, a target_of
 * entry < -1 or >= n_targets, sharded and shared-source batches, a batch of another context, a batch with an alignment begun and not
 * ended, an ordinary context. */
LOCGPU_API int locgpu_ndt_align_pairs(locgpu_ctx* ctx, locgpu_batch* batch, const int* target_of, const double* init_poses /* n_scans x 7 or NULL */,
                                      double* out_poses, locgpu_align_stats* stats /* n_scans or NULL */);
/* locgpu_ndt_fitness_batch per pair: the score of scan i under poses[i] against target target_of[i] alone (the residuals of AlignNdt's
 * gate, ndt_registration.cpp:374-464), bit for bit what an ordinary context holding that target reports — the check a caller makes
 * after each ScanMatch of test_node.cpp:317-374. target_of[i] == -1: {+inf, 0, 0}. Refusals as locgpu_ndt_align_pairs. */
LOCGPU_API int locgpu_ndt_fitness_pairs(locgpu_ctx* ctx, locgpu_batch* batch, const int* target_of, const double* poses, locgpu_fitness* out);

/* =====================================================================================================================
 * ---- The ICP target's KD-trees built on the device (csrc/forest_build.hip, csrc/forest_plan.hpp).
 *
 * SetInputTarget (icp_registration.cpp:9-29) builds the mean-split tree of kdtree.cpp:10-31 / :58-94 / :96-123, whose thresholds are
 * float32 sums in index order (math_utils.h:35-47). The calls above build it on the host, so a resident target crosses PCIe twice.
 * The calls of this block build the SAME trees — slot for slot, and for a forest the same array byte for byte, pads and sentinel
 * leaves included — in HBM: one workgroup per tree, level by level, every node's sum a serial chain in the reference's order, nodes,
 * trees and coordinates side by side. Nothing crosses PCIe but a table per tree down and the per-tree depths and flags up.
 *
 * A tree with a degenerate split (every point of a node on one side: duplicate points, NaNs; kdtree.cpp:66-70) cannot be placed
 * top-down. The kernel only finds that out; the WHOLE call then takes the host path of the matching call above (same result by
 * construction), and locgpu_icp_device_build_info says so. A refused call — LOCGPU_ERR_DEPTH included — leaves the context exactly as
 * it was: the trees are built beside the context's target and swapped in on success.
 *
 * Opt-in: no other entry point builds on the device. Not covered: LOAM handles, the C++ facade, asynchronous and broadcast forms,
 * scan pools, sharded and shared-source batches, bench.py.
 * ===================================================================================================================== */

/* locgpu_icp_set_target_forest_batch (SetInputTarget of every scan of a resident plain batch, icp_registration.cpp:9-29; the last_cloud of
 * test_node.cpp:256-315) with the trees built on the device. Accepts and refuses exactly what that call does and leaves the same context
 * state: the forest's bytes, locgpu_icp_forest_info, locgpu_icp_target_info, the search kernels' `bounded` choice. Blocking. */
LOCGPU_API int locgpu_icp_set_target_forest_device(locgpu_ctx* ctx, const locgpu_batch* batch);
/* locgpu_icp_set_target_cloud (SetInputTarget, icp_registration.cpp:9-29; the keyframe local map of lio.cpp:296-305) with the tree built on
 * the device: a forest of one tree installed as an ORDINARY target, its leaf-slot list and sentinel leaf included. Blocking. Refused: a
 * NULL cloud, a cloud of another context, an empty cloud; LOCGPU_ERR_DEPTH for a tree deeper than 64 levels. */
LOCGPU_API int locgpu_icp_set_target_cloud_device(locgpu_ctx* ctx, const locgpu_cloud* target);
/* What the last of the two calls above did on this context (kdtree.cpp:58-94 is what both paths build). out[0]: 0 no such call yet, 1 the
 * device build, 2 the host path after a degenerate split; out[1]: index of the first degenerate tree of the last device build, or -1;
 * out[2]: levels the kernel split (the deepest tree's depth - 1); out[3]: points per tile of the cooperative path; out[4]: the node
 * length up to which one lane splits a node (longer nodes take the cooperative path); out[5]: threads per workgroup (one workgroup a
 * tree); out[6]: 1 a forest, 2 a single cloud; out[7]: 1 when the context's CURRENT target, however it was built, lets the fast
 * search kernel run (every float finite and below 1e18). */
LOCGPU_API int locgpu_icp_device_build_info(const locgpu_ctx* ctx, int64_t out[8]);
/* Test read-back of the packed tree or forest as it stands in HBM after ANY locgpu_icp_set_target* call (kdtree.cpp:10-31's tree in the
 * layout of csrc/kdtree_build.cpp): slots[0 .. min(cap, S + 2)) with S = locgpu_icp_target_info's bytes / 8, i.e. every segment, pad
 * and sentinel leaf up to the last sentinel leaf; for an ORDINARY target also leaf_slots[0 .. min(leaf_cap, leaves)), the slot of every
 * leaf in preorder (a forest keeps none: the array is left alone). Either array may be NULL. */
LOCGPU_API int locgpu_debug_tree_read(locgpu_ctx* ctx, uint64_t* slots, size_t cap, uint32_t* leaf_slots, size_t leaf_cap);

#ifdef __cplusplus
}
#endif
#endif /* LOCGPU_H_ */
