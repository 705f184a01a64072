// loc_lib_amd/csrc/ndt_inc.hip — incremental NDT (NdtMethod::INCREMENTAL_NDT), the mapping flow's default
// (slam_demo/config/slam.yaml:53).
//
// Reference: NdtRegistration::SetIncNdtTargetCloud (ndt_registration.cpp:150-183), UpdateVoxel (:185-236),
// AlignIncNdt (:262-372).
//
// State, all of it in HBM (round 4; rounds 1-3 walked the points on the host through a std::list + std::unordered_map):
//   per slot   key (u64, kNdtEmpty = free), recency stamp (call number << 32 | index of the voxel's last point in that call),
//              μ (3 f64), info (9 f64);    a stack of free slots;    an open-addressing table key → slot for the align kernel.
// The reference's container is an LRU cache of capacity − 1 voxels (inc_ndt_lru.hpp restates its loop), and an LRU cache always
// holds exactly the most recently used keys. So when a cloud touches m ≤ capacity − 1 distinct voxels:
//   * none of the voxels it touches can be evicted again within the call (fewer than capacity − 1 other keys are younger);
//   * the voxel set after the call = the capacity − 1 largest stamps of {old voxels} ∪ {touched voxels}, i.e. the E =
//     max(0, live + new − (capacity − 1)) old voxels with the smallest stamps leave, whatever the order of the points was;
//   * every touched voxel's statistics are recomputed from ALL of its points of this call, in input order (`flag_first_scan_` is
//     forced true at the end of every SetIncNdtTargetCloud, :181, so UpdateVoxel always takes its first branch, :186-198: more
//     than one point ⇒ mean, (n−1)-covariance, info = (Σ + 1e-3·I)⁻¹; a single point ⇒ μ = the point, info = 100·I), untouched
//     voxels keep theirs.
// That is a sort, a scan and a few per-voxel kernels: the ingest front shared with the direct table (ndt_ingest.hpp: the runs of
// equal keys, a voxel's points in input order) → table look-ups → ONE read-back of the counters → stamps, evictions (a sort of the
// live stamps, only when E > 0), slots for the new voxels, table rebuild, per-voxel statistics by one thread per voxel from the
// front's sums — the reference's own summation order, so μ and info carry the oracle's bits, not just its digits, and are the
// same bits run after run (the round-3 kernels summed with FP64 atomics).
// A cloud whose own working set exceeds the capacity (m > capacity − 1: test-sized capacities only — the reference default is
// 100 000 voxels) needs the order of its points: the live {key, stamp, slot} records come back to the host, inc_lru_replay()
// walks the points exactly like the reference, and the device finishes from the replayed state with the lost points masked out.
// Every buffer is owned by the state and only grows: no hipMalloc / hipFree per call. Every array is written before it is
// read: a slot's μ/info are written by the call that hands the slot out (its voxel has at least one point), the table is
// refilled on every call, the scratch arrays are produced by the kernels in front of their readers.
//
// align: AlignIncNdt differs from the direct variant: sums ARE info-weighted (H += Jᵀ·info·J, err += −Jᵀ·info·e, :345-346),
// effective_num counts accepted (point, voxel) pairs (:343), too few ⇒ `return false` with result = current pose (:349-353), and
// there is no det(H) test.
#include "device_buffer.hpp"
#include "device_prims.hpp"
#include "env.hpp"

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "icp_kernels.hpp"
#include "inc_ndt_lru.hpp"
#include "ndt_inc.hpp"
#include "ndt_ingest.hpp"
#include "ndt_kernels.hpp"

namespace locgpu {

static_assert(kIncNoKey == kNdtEmpty, "inc_ndt_lru.hpp and ndt_kernels.hpp disagree on the empty key");

// ---------------------------------------------------------------------------------------------- ingest kernels
// the front's counter block (ndt_ingest.hpp), mirrored in pinned host memory; this file's two: distinct keys of the call that are not
// in the table (new voxels), live slots collected for the eviction sort
enum { kIncNew = kIngUser, kIncCollected = kIngUser + 1 };
static_assert(kIncCollected < kIngCtrs, "the counter block is too small");

// run u → its voxel's slot (−1: not in the table, −2: the run of skipped points); counts the new voxels
__global__ __launch_bounds__(kBlock) void inc_lookup_kernel(const unsigned long long* __restrict__ ukey, const int* __restrict__ ctr_in,
                                                            const unsigned long long* __restrict__ tkeys, const int* __restrict__ tvid, size_t cap_mask,
                                                            int* __restrict__ uslot, int* __restrict__ unew, int* __restrict__ ctr) {
    const int u = blockIdx.x * kBlock + threadIdx.x;
    if (u >= ctr_in[kIngRuns]) return;
    const unsigned long long key = ukey[u];
    int slot = -2, is_new = 0;
    if (key != kNdtEmpty) {
        slot = -1;
        size_t h = ndt_hash(key, cap_mask);
        for (;;) {
            const unsigned long long k2 = tkeys[h];
            if (k2 == key) { slot = tvid[h]; break; }
            if (k2 == kNdtEmpty) break;
            h = (h + 1) & cap_mask;
        }
        is_new = slot < 0 ? 1 : 0;
        if (is_new) atomicAdd(&ctr[kIncNew], 1);
    }
    uslot[u] = slot;
    unew[u] = is_new;
}

// the voxels the call touches that already exist: most recent now (ndt cpp:169-170)
__global__ __launch_bounds__(kBlock) void inc_touch_kernel(const int* __restrict__ uslot, const uint32_t* __restrict__ ustart, const uint32_t* __restrict__ sidx, int m,
                                                           unsigned long long epoch_hi, unsigned long long* __restrict__ slot_stamp) {
    const int u = blockIdx.x * kBlock + threadIdx.x;
    if (u >= m) return;
    const int slot = uslot[u];
    if (slot >= 0) slot_stamp[slot] = epoch_hi | (unsigned long long)sidx[ustart[u + 1] - 1u];  // stable sort: the run's last element is the voxel's last point
}

// {stamp, slot} of every live slot, for the eviction sort
__global__ __launch_bounds__(kBlock) void inc_collect_kernel(const unsigned long long* __restrict__ slot_key, const unsigned long long* __restrict__ slot_stamp, int n_slots,
                                                             unsigned long long* __restrict__ ev_stamp, int* __restrict__ ev_slot, int* __restrict__ ctr) {
    const int sl = blockIdx.x * kBlock + threadIdx.x;
    if (sl >= n_slots || slot_key[sl] == kNdtEmpty) return;
    const int pos = atomicAdd(&ctr[kIncCollected], 1);  // the order is settled by the sort (stamps are unique)
    ev_stamp[pos] = slot_stamp[sl];
    ev_slot[pos] = sl;
}

// the E least recently used voxels leave (ndt cpp:161-165); their slots go on top of the free stack, the oldest lowest
__global__ __launch_bounds__(kBlock) void inc_evict_kernel(const int* __restrict__ ev_slot_sorted, int n_evict, int n_free, unsigned long long* __restrict__ slot_key,
                                                           int* __restrict__ free_stack) {
    const int e = blockIdx.x * kBlock + threadIdx.x;
    if (e >= n_evict) return;
    const int sl = ev_slot_sorted[e];
    slot_key[sl] = kNdtEmpty;
    free_stack[n_free + e] = sl;
}

// a slot for every new voxel: from the top of the free stack, then fresh ones
__global__ __launch_bounds__(kBlock) void inc_assign_kernel(const unsigned long long* __restrict__ ukey, const int* __restrict__ unew, const int* __restrict__ urank,
                                                            const uint32_t* __restrict__ ustart, const uint32_t* __restrict__ sidx, int m, const int* __restrict__ free_stack,
                                                            int n_free, int n_slots, unsigned long long epoch_hi, unsigned long long* __restrict__ slot_key,
                                                            unsigned long long* __restrict__ slot_stamp, int* __restrict__ uslot) {
    const int u = blockIdx.x * kBlock + threadIdx.x;
    if (u >= m || !unew[u]) return;
    const int r = urank[u];
    const int slot = r < n_free ? free_stack[n_free - 1 - r] : n_slots + (r - n_free);
    slot_key[slot] = ukey[u];
    slot_stamp[slot] = epoch_hi | (unsigned long long)sidx[ustart[u + 1] - 1u];
    uslot[u] = slot;
}

// key → slot table of the live slots (refilled on every call)
__global__ __launch_bounds__(kBlock) void inc_table_kernel(const unsigned long long* __restrict__ slot_key, int n_slots, unsigned long long* keys, int* vid,
                                                           size_t cap_mask) {
    const int sl = blockIdx.x * kBlock + threadIdx.x;
    if (sl >= n_slots) return;
    const unsigned long long key = slot_key[sl];
    if (key == kNdtEmpty) return;
    size_t h = ndt_hash(key, cap_mask);
    for (;;) {
        const unsigned long long prev = atomicCAS(&keys[h], kNdtEmpty, key);
        if (prev == kNdtEmpty) break;
        h = (h + 1) & cap_mask;
    }
    vid[h] = sl;
}

// UpdateVoxel, first-scan branch (ndt cpp:186-198): one thread per touched voxel; math::ComputeMeanAndCov's sums are the front's
// (ndt_mean_scatter: no contraction — this kernel must not get an fp contract pragma), the 3×3 inverse is the cofactor form of
// Eigen's fixed-size inverse.
__global__ __launch_bounds__(kBlock) void inc_stats_kernel(const float4* __restrict__ psorted, const uint32_t* __restrict__ ustart, const int* __restrict__ uslot, int m,
                                                           double* __restrict__ mu, double* __restrict__ info) {
    const int u = blockIdx.x * kBlock + threadIdx.x;
    if (u >= m) return;
    const int slot = uslot[u];
    if (slot < 0) return;  // the run of skipped points
    const uint32_t b = ustart[u], e = ustart[u + 1];
    const uint32_t len = e - b;
    double* M = mu + 3 * (size_t)slot;
    double* I = info + 9 * (size_t)slot;
    if (len > 1) {
        double mean[3], sc[6];
        ndt_mean_scatter(psorted, b, e, mean, sc);
        const double l1 = (double)(len - 1);
        const double a = sc[0] / l1 + 1e-3, bq = sc[1] / l1, c = sc[2] / l1, e4 = sc[3] / l1 + 1e-3, f = sc[4] / l1, i8 = sc[5] / l1 + 1e-3;
        const double d = bq, g = c, h = f;  // the matrix is symmetric: (row 1, col 0) = (0, 1) etc. — the same numbers, so the same bits
        const double det = a * (e4 * i8 - f * h) - bq * (d * i8 - f * g) + c * (d * h - e4 * g);
        const double id = 1.0 / det;
        I[0] = (e4 * i8 - f * h) * id; I[1] = (c * h - bq * i8) * id; I[2] = (bq * f - c * e4) * id;
        I[3] = (f * g - d * i8) * id;  I[4] = (a * i8 - c * g) * id;  I[5] = (c * d - a * f) * id;
        I[6] = (d * h - e4 * g) * id;  I[7] = (bq * g - a * h) * id;  I[8] = (a * e4 - bq * d) * id;
        M[0] = mean[0]; M[1] = mean[1]; M[2] = mean[2];
    } else {
        const float4 p = psorted[b];
        M[0] = (double)p.x; M[1] = (double)p.y; M[2] = (double)p.z;
#pragma unroll
        for (int k = 0; k < 9; ++k) I[k] = (k % 4 == 0) ? 1e2 : 0.0;
    }
}

// ---------------------------------------------------------------------------------------------- accumulate kernel
// Grid (ceil(max_n/256), n_scans). acc[27] = number of accepted (point, voxel) residuals.
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void inc_accum_kernel(const unsigned long long* __restrict__ keys, const int* __restrict__ vid,
                                                           const double* __restrict__ mu, const double* __restrict__ info, size_t cap_mask,
                                                           double inv_voxel, double res_th, int n_nearby, const float4* __restrict__ src,
                                                           const int* __restrict__ counts, const PoseState* __restrict__ st, int max_n,
                                                           double* __restrict__ partials, const int* __restrict__ active, const int* __restrict__ src_of) {
#pragma clang fp contract(fast)
    const int scan = active ? active[blockIdx.y] : (int)blockIdx.y;
    if (st[scan].done) return;
    const int i = blockIdx.x * kBlock + threadIdx.x;
    double acc[28];
#pragma unroll
    for (int v = 0; v < 28; ++v) acc[v] = 0.0;
    if (i < counts[scan]) {
        const float4 p = src[src_index(src_of, scan, max_n, i)];
        const D3 q{(double)p.x, (double)p.y, (double)p.z};
        const D3 qs = se3_apply(st[scan].q, st[scan].t, q);
        const int kx = (int)(qs.x * inv_voxel), ky = (int)(qs.y * inv_voxel), kz = (int)(qs.z * inv_voxel);
        const int ox[7] = {0, -1, 1, 0, 0, 0, 0}, oy[7] = {0, 0, 0, 1, -1, 0, 0}, oz[7] = {0, 0, 0, 0, 0, -1, 1};
        double Is[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0}, Ie[3] = {0, 0, 0}, n_acc = 0.0;
        // the seven look-ups level by level instead of one chain of dependent gathers after the other; the sums
        // are formed in the order j = 0..6 from the same numbers
        unsigned long long key[7], kk[7];
        size_t hs[7];
        bool found[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int x = kx + ox[j], y = ky + oy[j], z = kz + oz[j];
            found[j] = j < n_nearby && ndt_key_in_range(x, y, z);
            key[j] = ndt_pack(found[j] ? x : kx, found[j] ? y : ky, found[j] ? z : kz);
            hs[j] = ndt_hash(key[j], cap_mask);
        }
#pragma unroll
        for (int j = 0; j < 7; ++j) kk[j] = keys[hs[j]];
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            if (found[j] && kk[j] != key[j] && kk[j] != kNdtEmpty) {  // collision on the first probe: walk on
                size_t h = (hs[j] + 1) & cap_mask;
                for (;;) {
                    const unsigned long long k2 = keys[h];
                    if (k2 == key[j]) { kk[j] = k2; hs[j] = h; break; }
                    if (k2 == kNdtEmpty) { kk[j] = k2; break; }
                    h = (h + 1) & cap_mask;
                }
            }
            found[j] = found[j] && kk[j] == key[j];
        }
        int vx[7];
#pragma unroll
        for (int j = 0; j < 7; ++j) vx[j] = vid[found[j] ? hs[j] : 0];
#pragma unroll
        for (int j = 0; j < 7; ++j) found[j] = found[j] && vx[j] >= 0;
#pragma unroll
        for (int j = 0; j < 7; ++j) {
            const int v = found[j] ? vx[j] : 0;  // a voxel that is not there reads record 0 and is not accepted
            const double* m = mu + 3 * (size_t)v;
            const double* I = info + 9 * (size_t)v;
            const double e[3] = {qs.x - m[0], qs.y - m[1], qs.z - m[2]};
            double ie[3];
#pragma unroll
            for (int r = 0; r < 3; ++r) ie[r] = (I[3 * r] * e[0] + I[3 * r + 1] * e[1]) + I[3 * r + 2] * e[2];
            const double res = (e[0] * ie[0] + e[1] * ie[1]) + e[2] * ie[2];
            const bool accept = found[j] && !(isnan(res) || res > res_th);
            n_acc = accept ? n_acc + 1.0 : n_acc;
#pragma unroll
            for (int k = 0; k < 9; ++k) Is[k] = accept ? Is[k] + I[k] : Is[k];
#pragma unroll
            for (int k = 0; k < 3; ++k) Ie[k] = accept ? Ie[k] + ie[k] : Ie[k];
        }
        acc[27] = n_acc;
        if (n_acc > 0.0) {
            // J = [A | I3], A = −R·hat(q) (the same for every voxel of this point) ⇒ Σ_v Jᵀ·info_v·J = Jᵀ·(Σ info_v)·J
            const double* R = st[scan].R;
            double A[3][3];
#pragma unroll
            for (int r = 0; r < 3; ++r) {
                A[r][0] = -(R[3 * r + 1] * q.z - R[3 * r + 2] * q.y);
                A[r][1] = -(R[3 * r + 2] * q.x - R[3 * r + 0] * q.z);
                A[r][2] = -(R[3 * r + 0] * q.y - R[3 * r + 1] * q.x);
            }
            double J[3][6], IJ[3][6];
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 3; ++c) { J[r][c] = A[r][c]; J[r][3 + c] = (r == c) ? 1.0 : 0.0; }
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int c = 0; c < 6; ++c) IJ[r][c] = (Is[3 * r] * J[0][c] + Is[3 * r + 1] * J[1][c]) + Is[3 * r + 2] * J[2][c];
            int o = 0;
#pragma unroll
            for (int a = 0; a < 6; ++a)
#pragma unroll
                for (int b = a; b < 6; ++b) acc[o++] = (J[0][a] * IJ[0][b] + J[1][a] * IJ[1][b]) + J[2][a] * IJ[2][b];
#pragma unroll
            for (int a = 0; a < 6; ++a) acc[21 + a] = -((J[0][a] * Ie[0] + J[1][a] * Ie[1]) + J[2][a] * Ie[2]);
        }
    }
    block_reduce_store<28, kAccW>(acc, partials + ((size_t)scan * gridDim.x + blockIdx.x) * kAccW);
}

// ---------------------------------------------------------------------------------------------- state
struct IncNdtState {
    size_t capacity = 100000;
    double inv_voxel = 1.0;
    uint32_t epoch = 0;  // calls so far (the high half of the recency stamps)
    // counts the host keeps (the arrays below are the state itself)
    int n_slots = 0;  // slots ever handed out: [0, n_slots)
    int n_live = 0;   // voxels alive
    int n_free = 0;   // entries on the free stack
    // per slot; d_free, grown last, has the capacity of all five
    DevBuf<unsigned long long> d_slot_key, d_slot_stamp;
    DevBuf<double> d_mu, d_info;
    DevBuf<int> d_free;
    // key → slot table for the align kernel
    DevBuf<unsigned long long> d_keys;
    DevBuf<int> d_vid;
    size_t table_cap = 0;
    NdtIngest ing;  // the front's per-call scratch, by points; grows with the rule of ensure_points
    // per run of the call, as long as the front's arrays (a call has at most n voxels)
    DevBuf<int> d_uslot, d_unew, d_urank;
    // eviction scratch, by slots (ev_cap)
    DevBuf<unsigned long long> d_ev_stamp, d_ev_stamp_sorted;
    DevBuf<int> d_ev_slot, d_ev_slot_sorted;
    size_t ev_cap = 0;
    PinnedBuf<int> h_ctr;  // the front's kIngCtrs counters, read back
};

static size_t grown(size_t have, size_t need, size_t floor_) {
    size_t cap = have ? have : floor_;
    while (cap < need) cap *= 2;
    return cap;
}

// room for `need` slots (μ/info/keys/stamps of the slots in use are kept)
static hipError_t ensure_slots(IncNdtState& st, size_t need, hipStream_t s) {
    if (need <= st.d_free.cap()) return hipSuccess;
    const size_t cap = grown(st.d_free.cap(), need, 4096), old = (size_t)st.n_slots;
    LOCGPU_TRY(st.d_slot_key.grow_keep(cap, old, s));
    LOCGPU_TRY(st.d_slot_stamp.grow_keep(cap, old, s));
    LOCGPU_TRY(st.d_mu.grow_keep(3 * cap, 3 * old, s));
    LOCGPU_TRY(st.d_info.grow_keep(9 * cap, 9 * old, s));
    LOCGPU_TRY(st.d_free.grow_keep(cap, (size_t)st.n_free, s));
    return hipSuccess;
}

static hipError_t ensure_points(IncNdtState& st, size_t n, hipStream_t s) {
    LOCGPU_TRY(st.h_ctr.reserve(kIngCtrs));
    if (!st.table_cap) {  // an empty table, so that the first call's look-ups run like every other call's
        const size_t cap = 1024;
        LOCGPU_TRY(st.d_keys.alloc(cap));
        LOCGPU_TRY(st.d_vid.alloc(cap));
        st.table_cap = cap;
        hipLaunchKernelGGL(ndt_fill_kernel<unsigned long long>, dim3((unsigned)(cap / kBlock)), dim3(kBlock), 0, s, st.d_keys.get(), cap, kNdtEmpty);
        LOCGPU_TRY(hipMemsetAsync(st.d_vid, 0xFF, cap * sizeof(int), s));
    }
    // every call, so that an allocation that failed is tried again; nothing happens when all of it is there
    const size_t cap = n + 1 > st.ing.cap() ? grown(st.ing.cap(), n + 1, 16384) : st.ing.cap();
    LOCGPU_TRY(st.d_uslot.reserve(cap)); LOCGPU_TRY(st.d_unew.reserve(cap)); LOCGPU_TRY(st.d_urank.reserve(cap));
    return st.ing.reserve(cap, true);
}

static hipError_t ensure_evict(IncNdtState& st, size_t n_live, hipStream_t s) {
    if (n_live > st.ev_cap) {
        const size_t cap = grown(st.ev_cap, n_live, 4096);
        LOCGPU_TRY(st.d_ev_stamp.alloc(cap)); LOCGPU_TRY(st.d_ev_stamp_sorted.alloc(cap));
        LOCGPU_TRY(st.d_ev_slot.alloc(cap)); LOCGPU_TRY(st.d_ev_slot_sorted.alloc(cap));
        st.ev_cap = cap;
        size_t b = 0;
        LOCGPU_TRY(prim::sort_pairs(nullptr, b, st.d_ev_stamp.get(), st.d_ev_stamp_sorted.get(), st.d_ev_slot.get(), st.d_ev_slot_sorted.get(), (int)cap, 0, 64, s));
        LOCGPU_TRY(st.ing.ensure_temp(b));
    }
    return hipSuccess;
}

IncNdtState* inc_ndt_create(size_t capacity, double voxel_size) {
    auto* st = new IncNdtState();
    st->capacity = capacity;
    st->inv_voxel = 1.0 / voxel_size;
    return st;
}

void inc_ndt_destroy(IncNdtState* st) { delete st; }

size_t inc_ndt_num_voxels(const IncNdtState* st) { return st ? (size_t)st->n_live : 0; }

static unsigned grid_for(size_t n) { return (unsigned)((std::max<size_t>(n, 1) + kBlock - 1) / kBlock); }

// the front, then the look-ups; returns with h_ctr read back (one synchronisation)
static hipError_t sort_and_look_up(IncNdtState& st, const float4* d_pts, size_t n, bool masked, hipStream_t s) {
    NdtIngest& g = st.ing;
    LOCGPU_TRY(g.run(d_pts, n, st.inv_voxel, masked, s));
    hipLaunchKernelGGL(inc_lookup_kernel, dim3(grid_for(n)), dim3(kBlock), 0, s, g.ukey, g.ctr, st.d_keys, st.d_vid, st.table_cap - 1, st.d_uslot, st.d_unew, g.ctr);
    LOCGPU_TRY(hipGetLastError());
    LOCGPU_TRY(hipMemcpyAsync(st.h_ctr, g.ctr, kIngCtrs * sizeof(int), hipMemcpyDeviceToHost, s));
    LOCGPU_TRY(hipStreamSynchronize(s));
    return hipSuccess;
}

// table of the live slots + per-voxel statistics of the m touched voxels (uslot[u] ≥ 0 for every real run)
static hipError_t rebuild_table_and_stats(IncNdtState& st, int m, hipStream_t s) {
    size_t cap = 1024;
    while (cap < 2 * (size_t)std::max(st.n_live, 1)) cap <<= 1;
    if (cap > st.table_cap) {  // grows only
        st.d_keys.reset(); st.d_vid.reset(); st.table_cap = 0;
        LOCGPU_TRY(st.d_keys.alloc(cap));
        LOCGPU_TRY(st.d_vid.alloc(cap));
        st.table_cap = cap;
    }
    hipLaunchKernelGGL(ndt_fill_kernel<unsigned long long>, dim3(grid_for(st.table_cap)), dim3(kBlock), 0, s, st.d_keys.get(), st.table_cap, kNdtEmpty);
    LOCGPU_TRY(hipMemsetAsync(st.d_vid, 0xFF, st.table_cap * sizeof(int), s));
    hipLaunchKernelGGL(inc_table_kernel, dim3(grid_for((size_t)st.n_slots)), dim3(kBlock), 0, s, st.d_slot_key, st.n_slots, st.d_keys, st.d_vid, st.table_cap - 1);
    if (m > 0) hipLaunchKernelGGL(inc_stats_kernel, dim3(grid_for((size_t)m)), dim3(kBlock), 0, s, st.ing.psorted, st.ing.ustart, st.d_uslot, m, st.d_mu, st.d_info);
    LOCGPU_TRY(hipGetLastError());
    return hipStreamSynchronize(s);
}

// The cloud's own working set exceeds the capacity: replay the points in order on the host (inc_lru_replay), from the device's state.
static hipError_t ingest_replayed(IncNdtState& st, const float4* host_pts, const float4* d_pts, size_t n, hipStream_t s) {
    std::vector<float4> fetched;
    if (!host_pts) {
        fetched.resize(n);
        LOCGPU_TRY(hipMemcpyAsync(fetched.data(), d_pts, n * sizeof(float4), hipMemcpyDeviceToHost, s));
        LOCGPU_TRY(hipStreamSynchronize(s));
        host_pts = fetched.data();
    }
    const size_t ns = (size_t)st.n_slots;
    std::vector<unsigned long long> h_key(ns), h_stamp(ns);
    std::vector<int> free_slots((size_t)st.n_free);
    if (ns) {
        LOCGPU_TRY(hipMemcpyAsync(h_key.data(), st.d_slot_key, ns * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        LOCGPU_TRY(hipMemcpyAsync(h_stamp.data(), st.d_slot_stamp, ns * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
    }
    if (st.n_free) LOCGPU_TRY(hipMemcpyAsync(free_slots.data(), st.d_free, (size_t)st.n_free * sizeof(int), hipMemcpyDeviceToHost, s));
    LOCGPU_TRY(hipStreamSynchronize(s));
    std::vector<IncLive> live;
    live.reserve((size_t)st.n_live);
    for (size_t sl = 0; sl < ns; ++sl)
        if (h_key[sl] != kNdtEmpty) live.push_back(IncLive{h_key[sl], h_stamp[sl], (int)sl});
    std::vector<uint64_t> keys(n);
    for (size_t i = 0; i < n; ++i) {
        // the conversion the device's ndt_key_kernel performs (v_cvt_i32_f64: NaN → 0, saturating) — `(int)` of such a value is
        // undefined on the host, and the two paths must key a point alike
        auto cvt = [](double v) { return v != v ? 0 : (v >= 2147483647.0 ? 2147483647 : (v <= -2147483648.0 ? (-2147483647 - 1) : (int)v)); };
        const int kx = cvt((double)host_pts[i].x * st.inv_voxel), ky = cvt((double)host_pts[i].y * st.inv_voxel), kz = cvt((double)host_pts[i].z * st.inv_voxel);
        keys[i] = ndt_key_in_range(kx, ky, kz) ? ndt_pack(kx, ky, kz) : kIncNoKey;
    }
    std::vector<unsigned char> keep;
    int n_slots = st.n_slots;
    inc_lru_replay(live, free_slots, n_slots, st.capacity, st.epoch, keys.data(), n, keep);
    LOCGPU_TRY(ensure_slots(st, (size_t)std::max(n_slots, 1), s));
    st.n_slots = n_slots;
    st.n_live = (int)live.size();
    st.n_free = (int)free_slots.size();
    h_key.assign((size_t)n_slots, kNdtEmpty);
    h_stamp.assign((size_t)n_slots, 0ull);
    for (const IncLive& v : live) { h_key[(size_t)v.slot] = v.key; h_stamp[(size_t)v.slot] = v.stamp; }
    if (n_slots) {
        LOCGPU_TRY(hipMemcpyAsync(st.d_slot_key, h_key.data(), (size_t)n_slots * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
        LOCGPU_TRY(hipMemcpyAsync(st.d_slot_stamp, h_stamp.data(), (size_t)n_slots * sizeof(unsigned long long), hipMemcpyHostToDevice, s));
    }
    if (st.n_free) LOCGPU_TRY(hipMemcpyAsync(st.d_free, free_slots.data(), (size_t)st.n_free * sizeof(int), hipMemcpyHostToDevice, s));
    LOCGPU_TRY(hipMemcpyAsync(st.ing.keep, keep.data(), n, hipMemcpyHostToDevice, s));
    LOCGPU_TRY(hipStreamSynchronize(s));  // the vectors above are pageable: nothing may still be reading them when they go out of scope
    // the device finishes from the replayed state: table of the new voxel set, then the surviving points by voxel
    LOCGPU_TRY(rebuild_table_and_stats(st, 0, s));
    LOCGPU_TRY(sort_and_look_up(st, d_pts, n, true, s));
    const int m = st.h_ctr[kIngRuns] - st.h_ctr[kIngLastEmpty];
    if (st.h_ctr[kIncNew] != 0) return hipErrorUnknown;  // every surviving point's voxel is in the replayed set
    if (m > 0) hipLaunchKernelGGL(inc_stats_kernel, dim3(grid_for((size_t)m)), dim3(kBlock), 0, s, st.ing.psorted, st.ing.ustart, st.d_uslot, m, st.d_mu, st.d_info);
    LOCGPU_TRY(hipGetLastError());
    return hipStreamSynchronize(s);
}

// SetIncNdtTargetCloud. `d_pts` = the cloud in HBM; `host_pts` = the same on the host when the caller has it (else fetched if needed).
hipError_t inc_ndt_ingest(IncNdtState& st, const float4* host_pts, const float4* d_pts, size_t n, hipStream_t s, bool* bad_key) {
    *bad_key = false;
    if (n == 0) return hipSuccess;
    if (n > 0x7FFFFFF0ull) return hipErrorInvalidValue;
    st.epoch++;
    const unsigned long long epoch_hi = (unsigned long long)st.epoch << 32;
    LOCGPU_TRY(ensure_points(st, n, s));
    LOCGPU_TRY(sort_and_look_up(st, d_pts, n, false, s));
    *bad_key = st.h_ctr[kIngBadKey] != 0;
    const int m = st.h_ctr[kIngRuns] - st.h_ctr[kIngLastEmpty];  // distinct voxels the cloud touches
    const int m_new = st.h_ctr[kIncNew];                       // … of which not alive yet
    const long long M = (long long)st.capacity - 1;            // voxels the reference's list holds after every point (ndt cpp:161-165)
    if (m == 0) return hipSuccess;                             // every point skipped: nothing changes
    const int n_evict = (long long)m > M ? -1 : (int)std::max<long long>(0, (long long)st.n_live + m_new - M);
    static const bool dbg = env_flag("LOCGPU_INC_DEBUG");  // which path a call took (the determinism harness asserts it has seen all three)
    if (dbg) fprintf(stderr, "[locgpu inc-ndt] call %u: %zu points, %d voxels touched (%d new), %d alive, capacity %zu: %s\n", st.epoch, n, m, m_new, st.n_live, st.capacity,
                     n_evict < 0 ? "replayed on the host" : (n_evict > 0 ? "device path with evictions" : "device path, no eviction"));
    if (n_evict < 0) return ingest_replayed(st, host_pts, d_pts, n, s);
    const int n_free_after_evict = st.n_free + n_evict;
    const int n_fresh = std::max(0, m_new - n_free_after_evict);
    LOCGPU_TRY(ensure_slots(st, (size_t)(st.n_slots + n_fresh), s));
    hipLaunchKernelGGL(inc_touch_kernel, dim3(grid_for((size_t)m)), dim3(kBlock), 0, s, st.d_uslot, st.ing.ustart, st.ing.sidx, m, epoch_hi, st.d_slot_stamp);
    if (n_evict > 0) {
        LOCGPU_TRY(ensure_evict(st, (size_t)st.n_live, s));
        hipLaunchKernelGGL(inc_collect_kernel, dim3(grid_for((size_t)st.n_slots)), dim3(kBlock), 0, s, st.d_slot_key, st.d_slot_stamp, st.n_slots, st.d_ev_stamp, st.d_ev_slot, st.ing.ctr);
        size_t tb = st.ing.temp.cap();
        LOCGPU_TRY(prim::sort_pairs(st.ing.temp, tb, st.d_ev_stamp.get(), st.d_ev_stamp_sorted.get(), st.d_ev_slot.get(), st.d_ev_slot_sorted.get(), st.n_live, 0, 64, s));
        hipLaunchKernelGGL(inc_evict_kernel, dim3(grid_for((size_t)n_evict)), dim3(kBlock), 0, s, st.d_ev_slot_sorted, n_evict, st.n_free, st.d_slot_key, st.d_free);
    }
    if (m_new > 0) {
        size_t tb = st.ing.temp.cap();
        LOCGPU_TRY(prim::exclusive_sum(st.ing.temp, tb, st.d_unew.get(), st.d_urank.get(), m, s));
        hipLaunchKernelGGL(inc_assign_kernel, dim3(grid_for((size_t)m)), dim3(kBlock), 0, s, st.ing.ukey, st.d_unew, st.d_urank, st.ing.ustart, st.ing.sidx, m, st.d_free,
                           n_free_after_evict, st.n_slots, epoch_hi, st.d_slot_key, st.d_slot_stamp, st.d_uslot);
    }
    LOCGPU_TRY(hipGetLastError());
    st.n_free = std::max(0, n_free_after_evict - m_new);
    st.n_slots += n_fresh;
    st.n_live += m_new - n_evict;
    return rebuild_table_and_stats(st, m, s);
}

void launch_inc_accum(const IncNdtState* st, double res_th, int n_nearby, const float4* src, const int* counts, const PoseState* ps, int max_n,
                      int n_scans, double* partials, hipStream_t s, const int* active, int n_active, const int* src_of) {
    dim3 grid((max_n + kBlock - 1) / kBlock, active ? n_active : n_scans);
    hipLaunchKernelGGL(inc_accum_kernel, grid, dim3(kBlock), 0, s, st->d_keys, st->d_vid, st->d_mu, st->d_info, st->table_cap - 1, st->inv_voxel, res_th,
                       n_nearby, src, counts, ps, max_n, partials, active, src_of);
}

size_t inc_ndt_dump(const IncNdtState* st, int32_t* keys, double* mu, double* info, size_t cap) {
    const size_t ns = (size_t)st->n_slots;
    std::vector<unsigned long long> h_key(ns);
    std::vector<double> h_mu(ns * 3), h_info(ns * 9);
    if (ns) {
        (void)hipMemcpy(h_key.data(), st->d_slot_key, ns * sizeof(unsigned long long), hipMemcpyDeviceToHost);
        (void)hipMemcpy(h_mu.data(), st->d_mu, h_mu.size() * sizeof(double), hipMemcpyDeviceToHost);
        (void)hipMemcpy(h_info.data(), st->d_info, h_info.size() * sizeof(double), hipMemcpyDeviceToHost);
    }
    size_t n = 0;
    for (size_t sl = 0; sl < ns; ++sl) {
        const unsigned long long k = h_key[sl];
        if (k == kNdtEmpty) continue;
        if (n < cap) {
            if (keys) {
                keys[3 * n + 0] = (int)((k >> 42) & 0x1FFFFF) - kNdtBias;
                keys[3 * n + 1] = (int)((k >> 21) & 0x1FFFFF) - kNdtBias;
                keys[3 * n + 2] = (int)(k & 0x1FFFFF) - kNdtBias;
            }
            if (mu) for (int c = 0; c < 3; ++c) mu[3 * n + c] = h_mu[3 * sl + c];
            if (info) for (int c = 0; c < 9; ++c) info[9 * n + c] = h_info[9 * sl + c];
        }
        ++n;
    }
    return n;
}

size_t inc_ndt_table_size(const IncNdtState* st) { return st ? st->table_cap : 0; }

hipError_t inc_ndt_slots_read(const IncNdtState* st, uint64_t* keys, int32_t* vid, size_t cap, hipStream_t s) {
    const size_t n = std::min(cap, st->table_cap);
    if (n == 0) return hipSuccess;
    static_assert(sizeof(unsigned long long) == sizeof(uint64_t) && sizeof(int) == sizeof(int32_t), "the table's words are the read-back's");
    if (keys) LOCGPU_TRY(hipMemcpyAsync(keys, st->d_keys, n * sizeof(uint64_t), hipMemcpyDeviceToHost, s));
    if (vid) LOCGPU_TRY(hipMemcpyAsync(vid, st->d_vid, n * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    return hipStreamSynchronize(s);
}

const void* inc_ndt_table_ptr(const IncNdtState* st) { return st ? (const void*)st->d_keys : nullptr; }

}  // namespace locgpu
