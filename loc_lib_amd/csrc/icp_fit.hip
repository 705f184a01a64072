// loc_lib_amd/csrc/icp_fit.hip — K2/K3, the fit and solve stage of the ICP hot path: kernels + launchers (see icp_kernels.hpp).
#include "env.hpp"
#include "icp_kernels.hpp"
#include "launch.hpp"

#include <cstdlib>

namespace locgpu {

// acc layout: [0..20] upper triangle of H row by row (00 01 .. 05 11 12 .. 55), [21..26] B, [27] effective_num.
template <int ROWS>
__device__ __forceinline__ void add_rows(double (&acc)[28], const double (&J)[ROWS][6], const double (&e)[ROWS]) {
#pragma clang fp contract(fast)
    int o = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
        for (int j = i; j < 6; ++j) {
            double s = J[0][i] * J[0][j];
#pragma unroll
            for (int r = 1; r < ROWS; ++r) s += J[r][i] * J[r][j];
            acc[o++] += s;
        }
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        double s = -J[0][i] * e[0];
#pragma unroll
        for (int r = 1; r < ROWS; ++r) s += -J[r][i] * e[r];
        acc[21 + i] += s;
    }
}

// Block-cooperative form of add_rows (the plane and line kernels). Keeping the 28 sums per thread costs 56 VGPRs that are live across
// the whole plane/line fit and cap those kernels at three waves per SIMD. Instead every thread leaves its point's row
// {J0..J5, -e, fit} in LDS, and thread (entry, slice) adds the products of ITS entry over its slice of the block's 256 rows: the
// same 28 FMAs per point and thread, one accumulator. Entry → the two row components it multiplies: 0..20 the upper triangle of
// JᵀJ, 21..26 J·(−e), 27 fit·fit (a count), 28..31 idle. Every thread of the block must call add()/store() (barriers inside).
constexpr int kAccPad = kBlock + 2;  // LDS row stride: consecutive rows four banks apart
struct RowAccum {
    int ent, slice, ra, rb;
    double sum;
    bool used;
    __device__ __forceinline__ void init() {
        index(threadIdx.x);
        sum = 0.0;
        used = false;
    }
    // the thread's entry and slice alone, from its thread index (a kernel short of registers may drop them over a phase and ask again)
    __device__ __forceinline__ void index(int tid) {
        ent = tid & 31;
        slice = tid >> 5;
        ra = 7; rb = 7;
        int o = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
            for (int j = i; j < 6; ++j) {
                if (o == ent) { ra = i; rb = j; }
                ++o;
            }
        if (ent >= 21 && ent < 27) { ra = ent - 21; rb = 6; }
    }
    template <int ROWS>
    __device__ __forceinline__ void add(double (&s_row)[8][kAccPad], const double (&J)[ROWS][6], const double (&neg_e)[ROWS], double fitted) {
#pragma clang fp contract(fast)
        const int tid = threadIdx.x;
#pragma unroll
        for (int r = 0; r < ROWS; ++r) {
            if (used) __syncthreads();  // the previous rows have been consumed
            used = true;
#pragma unroll
            for (int c = 0; c < 6; ++c) s_row[c][tid] = J[r][c];
            s_row[6][tid] = neg_e[r];
            s_row[7][tid] = r == 0 ? fitted : 0.0;
            __syncthreads();
            if (ent < 28) {
#pragma unroll 8
                for (int k = 0; k < 32; ++k) {  // rows slice, slice + 8, …: neighbouring slices read neighbouring LDS banks
                    const int col = k * (kBlock / 32) + slice;
                    sum += s_row[ra][col] * s_row[rb][col];
                }
            }
        }
    }
    __device__ __forceinline__ void store(double (&s_slice)[kBlock / 32][32], double* __restrict__ dst) {
        s_slice[slice][ent] = sum;
        __syncthreads();
        if (threadIdx.x < 28) {
            double t = s_slice[0][threadIdx.x];
#pragma unroll
            for (int w = 1; w < kBlock / 32; ++w) t += s_slice[w][threadIdx.x];
            dst[threadIdx.x] = t;
        }
    }
};

// R·hat(q), coefficient order of the oracle's left-to-right 3×3 product (zeros of hat() drop out exactly).
__device__ __forceinline__ void R_hat(const double* R, const D3& q, double (&Rh)[3][3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        Rh[r][0] = R[3 * r + 1] * q.z - R[3 * r + 2] * q.y;
        Rh[r][1] = R[3 * r + 2] * q.x - R[3 * r + 0] * q.z;
        Rh[r][2] = R[3 * r + 0] * q.y - R[3 * r + 1] * q.x;
    }
}

// The point-to-plane Jacobian row of source point q against the plane with unit normal n3 (the plane and map-plane kernels): the
// rotation part (−nᵀR)·hat(q), then n.
__device__ __forceinline__ void plane_row(const D3& n3, const double* R, const D3& q, double (&J)[6]) {
    double nR[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) nR[c] = -n3.x * R[c] + (-n3.y * R[3 + c] + -n3.z * R[6 + c]);  // the reference binary's order (libLocUtils.so 0x58745-0x58801)
    J[0] = nR[1] * q.z - nR[2] * q.y;
    J[1] = nR[2] * q.x - nR[0] * q.z;
    J[2] = nR[0] * q.y - nR[1] * q.x;
    J[3] = n3.x; J[4] = n3.y; J[5] = n3.z;
}

// math::FitPlane (math_utils.h:112-136) over the leaves at the five slots, in the order given, with the five residual checks of
// icp_registration.cpp:176-182. Returns whether the plane n4 = {n, d} fits.
// FIT: 0 = plane_null_vector (4-column one-sided Jacobi), 1 = plane_null_vector_secular with the former as its fall-back.
template <int FIT>
__device__ __forceinline__ bool fit_plane(const uint2* __restrict__ tree, const uint32_t (&slot)[5], double (&n4)[4]) {
    D3 nb[5];
#pragma unroll
    for (int j = 0; j < 5; ++j) nb[j] = leaf_point(tree, slot[j]);
    if constexpr (FIT == 1) {
        if (!plane_null_vector_secular(nb, n4)) plane_null_vector(nb, n4);
    } else {
        plane_null_vector(nb, n4);
    }
    const D3 n3{n4[0], n4[1], n4[2]};
    bool fit = true;
#pragma unroll
    for (int j = 0; j < 5; ++j) {
        const double err = dot3(n3, nb[j]) + n4[3];
        if (err * err > 1e-2) fit = false;
    }
    return fit;
}

// The row of source point p against its fitted plane n4 (icp_registration.cpp:184-200): J and −e stay zero behind the residual gate.
__device__ __forceinline__ void plane_point_row(const double (&n4)[4], const float4& p, const PoseState& ps, double max_plane_distance,
                                                double (&J)[6], double& neg_e) {
    const D3 n3{n4[0], n4[1], n4[2]};
    const D3 q{(double)p.x, (double)p.y, (double)p.z};
    const D3 qs = se3_apply(ps.q, ps.t, q);
    const double dis = dot3(n3, qs) + n4[3];
    if (!(fabs(dis) > max_plane_distance)) {
        plane_row(n3, ps.R, q, J);
        neg_e = -dis;
    }
}

// K2, P2Plane: IcpRegistration::CaculateMatrixHAndBP2Plane (icp_registration.cpp:161-213) + math::FitPlane, a fit per point: the body
// of icp_plane_accum_kernel<FIT, 0> (LOCGPU_PLANE_DEDUP=0; the defaults are the per-run bodies below, which give the same bits).
template <int FIT>
__device__ __forceinline__ void plane_accum_per_point(const uint2* __restrict__ tree, const float4* __restrict__ src,
                                                                 const int* __restrict__ counts, const PoseState* __restrict__ st,
                                                                 const uint32_t* __restrict__ nn, size_t nn_pitch, int max_n,
                                                                 double max_plane_distance, double* __restrict__ partials, int kPlanePts,
                                                                 const int* __restrict__ active, const int* __restrict__ src_of) {
    __shared__ double s_row[8][kAccPad];
    __shared__ double s_slice[kBlock / 32][32];
    const int scan = active ? active[blockIdx.y] : (int)blockIdx.y;
    if (st[scan].done) return;  // uniform per block
    RowAccum ra;  // see there: the 28 sums are not kept per thread
    ra.init();
    const int tid = threadIdx.x;
#pragma unroll 1
    for (int pp = 0; pp < kPlanePts; ++pp) {
        const int i = (blockIdx.x * kPlanePts + pp) * kBlock + tid;
        double J[1][6] = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
        double neg_e[1] = {0.0};
        double fitted = 0.0;
        if (i < counts[scan]) {
            const size_t gi = (size_t)scan * max_n + i;
            // all five indices and the point in one round trip (not: the fifth, then the rest behind its test)
            uint32_t slot[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) slot[j] = __builtin_nontemporal_load(&nn[(size_t)j * nn_pitch + gi]);
            const float4 p = src[src_index(src_of, scan, max_n, i)];
            if (slot[4] != kInvalidSlot) {  // nn.size() > 3: k=5 yields 5 or (k > size_) none
                sort5(slot);
                double n4[4];
                if (fit_plane<FIT>(tree, slot, n4)) {
                    fitted = 1.0;  // effective_num++ before the residual gate (icp cpp:184)
                    plane_point_row(n4, p, st[scan], max_plane_distance, J[0], neg_e[0]);
                }
            }
        }
        ra.add<1>(s_row, J, neg_e, fitted);
    }
    ra.store(s_slice, partials + ((size_t)scan * gridDim.x + blockIdx.x) * kAccW);
}

// K2, P2Plane, one fit per run of equal neighbour sets. Scans are ring-major: consecutive source points land centimetres apart on
// the map and about half of them get the five map points of the point before them, mostly in another distance order. The plane depends
// on the set alone (sort5), so a block fits once per run and deals the fits 64 to a wave; the rows, their LDS order, the block partials
// and with them every bit of the sums are plane_accum_per_point's. Over the block's kPlanePts · 256 points (at most kDedupPts):
//   leaders  a point with a full list whose sorted list differs from the previous lane's (by shuffle); lane 0 of a wave always is one,
//            which costs 1.6 % more fits, needs no read across waves and keeps runs over wave, pp and block boundaries right by
//            construction. A point without a list is neither a leader nor a follower, and the point behind it is a leader again.
//   rank     the inclusive count of leader flags in point order over the block (ballot + popcount, wave totals through LDS): the
//            1-based table row of a leader and of every follower of its run.
//   fit      leader j by thread j % 256 in pass j / 256: its point from s_lead, the five slots once more (an L2 hit), fit_plane,
//            n4 as it comes — NaNs of a non-finite leaf included — into s_plane[j], fit_plane's verdict into the top bit of
//            s_lead[j]. A wave whose 64 indices lie past the block's leader count skips the pass on a scalar branch.
//   rows     every thread takes the planes and verdicts of its points from row rank − 1 into registers; then, per point as before,
//            the row.
// LDS. The table (32 B per leader, 32 KB for 1024) does not fit beside s_row four times in 160 KB — it does not have to: the table
// lives from the fit phase to the moment the planes are in registers, s_row from then on, so s_row is the table's first 16.5 KB.
// Per block: table / s_row 32 768 + s_slice 2 048 + s_lead 2 048 + s_rank 2 048 + s_wcnt 64 = 38 976 B, four blocks in 160 KB.
constexpr int kDedupPP = 4;                   // points per thread the table has room for: icp_accum_split's largest plane rung
constexpr int kDedupPts = kDedupPP * kBlock;
constexpr uint16_t kLeadFits = 0x8000;        // s_lead[j]: the leader's plane fits (set behind its fit)
static_assert(8 * kAccPad <= 4 * kDedupPts && kDedupPts <= kLeadFits, "s_row inside the plane table; a leader's point in 15 bits");
template <int FIT>
__device__ __forceinline__ void plane_accum_per_run(const uint2* __restrict__ tree, const float4* __restrict__ src,
                                                                 const int* __restrict__ counts, const PoseState* __restrict__ st,
                                                                 const uint32_t* __restrict__ nn, size_t nn_pitch, int max_n,
                                                                 double max_plane_distance, double* __restrict__ partials, int kPlanePts,
                                                                 const int* __restrict__ active, const int* __restrict__ src_of) {
    __shared__ double s_plane[kDedupPts][4];
    __shared__ double s_slice[kBlock / 32][32];
    __shared__ uint16_t s_lead[kDedupPts];         // leader j → its point of the block, h · 256 + tid; later | kLeadFits
    __shared__ uint16_t s_rank[kDedupPP][kBlock];  // the ranks of a thread's points over the fit phase
    __shared__ int s_wcnt[kDedupPP][kBlock / 64];
    double (&s_row)[8][kAccPad] = *reinterpret_cast<double (*)[8][kAccPad]>(&s_plane[0][0]);
    const int scan = active ? active[blockIdx.y] : (int)blockIdx.y;
    if (st[scan].done) return;  // uniform per block
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n = counts[scan];
    const size_t region = (size_t)scan * max_n;
    const int first = blockIdx.x * kPlanePts * kBlock;  // point (h, tid) of the block is first + h · 256 + tid
    RowAccum ra;
    ra.init();
    // The fit phase has no register to spare (128 at four waves per SIMD), so nothing a later phase can work out again may stay live
    // across it. The thread index is taken anew per phase, in a way the compiler cannot see through: the addresses made from it, and
    // the accumulator's entry and slice, are then made where they are used; the ranks wait in LDS.
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    int rank[kDedupPP];  // the point's row of s_plane + 1; 0: no list
    bool leader[kDedupPP];
#pragma unroll
    for (int h = 0; h < kDedupPP; ++h) {
        const int i = first + h * kBlock + tid;
        uint32_t slot[5];
        bool has = false;
        if (h < kPlanePts && i < n) {
#pragma unroll
            for (int j = 0; j < 5; ++j) slot[j] = nn[(size_t)j * nn_pitch + region + i];
            has = slot[4] != kInvalidSlot;  // nn.size() > 3: k=5 yields 5 or (k > size_) none
        }
        if (has) {
            sort5(slot);
        } else {
#pragma unroll
            for (int j = 0; j < 5; ++j) slot[j] = kInvalidSlot;  // differs from every full list
        }
        bool differs = lane == 0;
#pragma unroll
        for (int j = 0; j < 5; ++j) differs |= (uint32_t)__shfl_up((int)slot[j], 1, 64) != slot[j];
        leader[h] = has && differs;
        const unsigned long long mask = __ballot(leader[h]);
        const int below = (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));  // leaders in the lanes before this one
        rank[h] = has ? below + (leader[h] ? 1 : 0) : 0;  // within the wave so far
        if (lane == 0) s_wcnt[h][wave] = __popcll(mask);
    }
    __syncthreads();
    int n_lead = 0, before[kDedupPP];
#pragma unroll
    for (int h = 0; h < kDedupPP; ++h) {
        before[h] = n_lead;
#pragma unroll
        for (int w = 0; w < kBlock / 64; ++w) {
            const int c = s_wcnt[h][w];
            before[h] += w < wave ? c : 0;
            n_lead += c;
        }
    }
    n_lead = __builtin_amdgcn_readfirstlane(n_lead);
#pragma unroll
    for (int h = 0; h < kDedupPP; ++h) {
        if (rank[h] > 0) rank[h] += before[h];
        if (leader[h]) s_lead[rank[h] - 1] = (uint16_t)(h * kBlock + tid);
        s_rank[h][tid] = (uint16_t)rank[h];
    }
    __syncthreads();
#pragma unroll 1
    for (int base = 0; base < n_lead; base += kBlock) {
        if (base + wave * 64 < n_lead) {  // scalar: the whole wave has a leader to fit, or none of it
            const int j = base + tid;
            if (j < n_lead) {
                const uint16_t pt = s_lead[j];
                const size_t gi = region + first + pt;
                uint32_t slot[5];
#pragma unroll
                for (int k = 0; k < 5; ++k) slot[k] = __builtin_nontemporal_load(&nn[(size_t)k * nn_pitch + gi]);
                sort5(slot);
                double n4[4];
                if (fit_plane<FIT>(tree, slot, n4)) s_lead[j] = pt | kLeadFits;  // read by this thread alone until the barrier
#pragma unroll
                for (int c = 0; c < 4; ++c) s_plane[j][c] = n4[c];
            }
        }
    }
    __syncthreads();
    tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    ra.index(tid);
    double n4[kDedupPP][4];
    float4 p[kDedupPP];
    bool fits[kDedupPP];
#pragma unroll
    for (int h = 0; h < kDedupPP; ++h) {
        rank[h] = s_rank[h][tid];
        fits[h] = false;
        if (rank[h] > 0) {
            fits[h] = (s_lead[rank[h] - 1] & kLeadFits) != 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) n4[h][c] = s_plane[rank[h] - 1][c];
            p[h] = src[src_index(src_of, scan, max_n, first + h * kBlock + tid)];
        }
    }
    __syncthreads();  // every plane is in registers: from here on the table's LDS is s_row
#pragma unroll
    for (int h = 0; h < kDedupPP; ++h) {
        if (h < kPlanePts) {  // uniform per block
            double J[1][6] = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
            double neg_e[1] = {0.0};
            double fitted = 0.0;
            if (fits[h]) {
                fitted = 1.0;  // effective_num++ before the residual gate (icp cpp:184)
                plane_point_row(n4[h], p[h], st[scan], max_plane_distance, J[0], neg_e[0]);
            }
            ra.add<1>(s_row, J, neg_e, fitted);
        }
    }
    ra.store(s_slice, partials + ((size_t)scan * gridDim.x + blockIdx.x) * kAccW);
}

// What the search stage's run flags (SearchArgs::run_flags) tell the threads of a block about their points: words[k] covers points
// first + 64 k … of the scan (the block's first point is a multiple of 256, so its up to 4 · kDedupPP words are contiguous), `left` =
// count − first. A bit counts only below the scan's count — a wave of the walk kernel that lies wholly past it wrote no word — and
// below the block's kPlanePts · 256 points. leader[h]: the flag of point (h, tid); rank[h]: the inclusive count of leader bits in block
// order up to that point, 0 for a point past the count; n_lead: the block's leaders (uniform). ONE trip to memory: lane k of every
// wave loads word k, the counts before each word are a prefix sum over those 16 lanes, and a wave takes the word of its points and the
// count before it from lane 4 h + wave.
__device__ __forceinline__ void run_flag_ranks(const unsigned long long* __restrict__ words, int left, int kPlanePts, int wave, int lane,
                                               int (&rank)[kDedupPP], bool (&leader)[kDedupPP], int& n_lead) {
    static_assert(4 * kDedupPP <= 16, "a word per lane of a 16-lane row");
    const int k = lane & 15;
    const int valid = k < 4 * kPlanePts ? left - 64 * k : 0;  // points of word k that exist
    unsigned long long word = 0ull;
    if (valid > 0) {
        word = words[k];
        if (valid < 64) word &= (1ull << valid) - 1ull;
    }
    const int count = __popcll(word);
    int upto = count;  // leaders in words 0..k
#pragma unroll
    for (int d = 1; d < 16; d <<= 1) {
        const int t = __shfl_up(upto, d, 16);
        if (k >= d) upto += t;
    }
    n_lead = __builtin_amdgcn_readlane(upto, 15);
#pragma unroll
    for (int h = 0; h < kDedupPP; ++h) {
        const int from = 4 * h + wave;  // uniform: the lane that holds the word of this wave's points h
        const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)word, from), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(word >> 32), from);
        const int before = __builtin_amdgcn_readlane(upto - count, from);
        const int mine = h < kPlanePts ? left - 64 * from : 0;
        const int below = (int)__builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0u));  // leaders in the lanes before this one
        const bool lead = (((lane < 32 ? lo : hi) >> (lane & 31)) & 1u) != 0u;
        leader[h] = lead;
        rank[h] = lane < mine ? before + below + (lead ? 1 : 0) : 0;
    }
}

// K2, P2Plane, one fit per run of equal neighbour sets, the runs marked by the search stage: the 64-lane walk kernel ends with every
// query's five slots in registers, its waves are the aligned groups of 64 points this kernel's waves are, and it answers "is my set
// the set of the point before me?" for a sort and five shuffles behind its main loop (icp_search.hip). Against plane_accum_per_run
// this body reads one 64-bit word per 64 points instead of 20 bytes per point, has no s_wcnt and one barrier less in front of the
// first fit; only the leaders load a list, once. (The ranks wait in LDS over the fit phase as before: working them out again from the
// words would put one more trip to memory in front of the rows.) No fit pass starts with a trip for its lists, and the source points
// are on their way while the block's slowest wave still fits (profiles/plane_trips.md):
//   leaders  as the walk kernel flagged them: lane 0 of a wave, a point without a full list, a point whose list the deep pass, the
//            in-wave exact walk or the redo kernel wrote after the walk (and the point behind it), a point whose set differs from the
//            previous lane's. A follower therefore has a full list, its leader's set. Not every leader has a list: it gets the
//            verdict "no fit" without a look at the tree, and with it the zero row.
//   lists    right behind the ranks thread (h, tid) loads the five words of every one of its points that leads — all of them in ONE
//            trip, up to 20 loads in flight, where registers are still free — and parks them, unsorted, in the leader's own table
//            row s_plane[rank − 1]: 32 B that nothing uses before that leader's fit. One 16-byte and one 4-byte store per list;
//            rows 32 B apart put eight rows on the 64 banks, so the 16-byte store of 64 consecutive rows uses half the banks of each
//            pass and the 4-byte one an eighth — a few dozen cycles per wave, nine waves' worth of stores per block.
//   fit      leader j by thread j % 256 in pass j / 256: the five words from row j, the test for a full list, sort5, fit_plane, n4
//            as it comes — NaNs of a non-finite leaf included — over the same row, the verdict into s_fits[j]. A row belongs to one
//            thread from the barrier in front of the fit phase to the one behind it.
//   points   a wave that has no pass left asks for the source points of its threads, all four in one trip, BEFORE it waits at the
//            barrier behind the fit phase. A thread without a point asks for the scan's last one: one block of loads under a uniform
//            branch (a branch per point makes four trips of them: the conversion to double sinks behind each load).
//   rows, LDS order, partials: plane_accum_per_run's, so every bit of the sums is.
// LDS per block: table / s_row 32 768 + s_slice 2 048 + s_fits 2 048 + s_rank 2 048 = 38 912 B, four blocks in 160 KB.
typedef uint4 __attribute__((may_alias)) table_u4;  // a parked list in a row of the plane table
typedef uint32_t __attribute__((may_alias)) table_u32;
template <int FIT>
__device__ __forceinline__ void plane_accum_flagged(const uint2* __restrict__ tree, const float4* __restrict__ src,
                                                                 const int* __restrict__ counts, const PoseState* __restrict__ st,
                                                                 const uint32_t* __restrict__ nn, size_t nn_pitch, int max_n,
                                                                 double max_plane_distance, double* __restrict__ partials, int kPlanePts,
                                                                 const int* __restrict__ active, const int* __restrict__ src_of,
                                                                 const unsigned long long* __restrict__ run_flags) {
    __shared__ double s_plane[kDedupPts][4];       // row j: leader j's five slots until its fit, its plane from then on
    __shared__ double s_slice[kBlock / 32][32];
    __shared__ uint16_t s_fits[kDedupPts];         // leader j → kLeadFits if its plane fits, else 0 (written by its fit)
    __shared__ uint16_t s_rank[kDedupPP][kBlock];  // the ranks of a thread's points over the fit phase
    double (&s_row)[8][kAccPad] = *reinterpret_cast<double (*)[8][kAccPad]>(&s_plane[0][0]);
    const int scan = active ? active[blockIdx.y] : (int)blockIdx.y;
    if (st[scan].done) return;  // uniform per block
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const size_t region = (size_t)scan * max_n;
    const int first = blockIdx.x * kPlanePts * kBlock;  // point (h, tid) of the block is first + h · 256 + tid
    const int left = counts[scan] - first;
    const unsigned long long* words = run_flags + (size_t)scan * ((max_n + 63) >> 6) + (first >> 6);
    RowAccum ra;
    ra.init();
    // As in plane_accum_per_run nothing a later phase can work out again may stay live across the fit phase: the thread index is
    // taken anew per phase, the ranks wait in LDS.
    int tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    int rank[kDedupPP], n_lead;
    bool leader[kDedupPP];
    run_flag_ranks(words, left, kPlanePts, wave, lane, rank, leader, n_lead);
    n_lead = __builtin_amdgcn_readfirstlane(n_lead);
    {
        uint32_t list[kDedupPP][5];  // the lists' only read: a leader bit is set only for a point below the count
#pragma unroll
        for (int h = 0; h < kDedupPP; ++h)
            if (leader[h]) {
#pragma unroll
                for (int k = 0; k < 5; ++k) list[h][k] = __builtin_nontemporal_load(&nn[(size_t)k * nn_pitch + region + first + h * kBlock + tid]);
            }
#pragma unroll
        for (int h = 0; h < kDedupPP; ++h) {
            if (leader[h]) {
                table_u4* row = reinterpret_cast<table_u4*>(&s_plane[rank[h] - 1][0]);
                row[0] = make_uint4(list[h][0], list[h][1], list[h][2], list[h][3]);
                reinterpret_cast<table_u32*>(row + 1)[0] = list[h][4];
            }
            s_rank[h][tid] = (uint16_t)rank[h];
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int base = 0; base < n_lead; base += kBlock) {
        if (base + wave * 64 < n_lead) {  // scalar: the whole wave has a leader to fit, or none of it
            const int j = base + tid;
            if (j < n_lead) {
                const table_u4* row = reinterpret_cast<const table_u4*>(&s_plane[j][0]);
                const uint4 head = row[0];
                uint32_t slot[5] = {head.x, head.y, head.z, head.w, reinterpret_cast<const table_u32*>(row + 1)[0]};
                uint16_t verdict = 0;
                if (slot[4] != kInvalidSlot) {  // nn.size() > 3: k=5 yields 5 or (k > size_) none — no list, no fit
                    sort5(slot);
                    double n4[4];
                    if (fit_plane<FIT>(tree, slot, n4)) verdict = kLeadFits;
#pragma unroll
                    for (int c = 0; c < 4; ++c) s_plane[j][c] = n4[c];
                }
                s_fits[j] = verdict;
            }
        }
    }
    tid = threadIdx.x;
    asm volatile("" : "+v"(tid));
    double n4[kDedupPP][4];
    float4 p[kDedupPP];
    bool fits[kDedupPP];
    if (left > 0) {  // uniform. A thread without a point asks for the scan's last one: ONE block of four loads, no branch per point
        typedef float quad __attribute__((ext_vector_type(4)));
        const quad* mine = reinterpret_cast<const quad*>(src + src_index(src_of, scan, max_n, first));
        quad q[kDedupPP];
#pragma unroll
        for (int h = 0; h < kDedupPP; ++h) q[h] = mine[min(h * kBlock + tid, left - 1)];
#pragma unroll
        for (int h = 0; h < kDedupPP; ++h) {
            asm volatile("" : "+v"(q[h]));  // all four asked for before the first conversion to double waits
            p[h] = make_float4(q[h].x, q[h].y, q[h].z, q[h].w);
        }
    }
#pragma unroll
    for (int h = 0; h < kDedupPP; ++h) rank[h] = s_rank[h][tid];  // the thread's own stores
    __syncthreads();
    ra.index(tid);
#pragma unroll
    for (int h = 0; h < kDedupPP; ++h) {
        fits[h] = false;
        if (rank[h] > 0) {
            fits[h] = s_fits[rank[h] - 1] != 0;
#pragma unroll
            for (int c = 0; c < 4; ++c) n4[h][c] = s_plane[rank[h] - 1][c];
        }
    }
    __syncthreads();  // every plane is in registers: from here on the table's LDS is s_row
#pragma unroll
    for (int h = 0; h < kDedupPP; ++h) {
        if (h < kPlanePts) {  // uniform per block
            double J[1][6] = {{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}};
            double neg_e[1] = {0.0};
            double fitted = 0.0;
            if (fits[h]) {
                fitted = 1.0;  // effective_num++ before the residual gate (icp cpp:184)
                plane_point_row(n4[h], p[h], st[scan], max_plane_distance, J[0], neg_e[0]);
            }
            ra.add<1>(s_row, J, neg_e, fitted);
        }
    }
    ra.store(s_slice, partials + ((size_t)scan * gridDim.x + blockIdx.x) * kAccW);
}

// The three bodies above under ONE kernel name — what the profiles, the benchmark's counters and the tools look for. RUNS: a fit per
// point (0), per run of equal neighbour sets found from the lists (1), per run as the search stage flagged them (2; run_flags set).
template <int FIT, int RUNS>
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(4, 4))) void icp_plane_accum_kernel(const uint2* __restrict__ tree, const float4* __restrict__ src,
                                                                 const int* __restrict__ counts, const PoseState* __restrict__ st,
                                                                 const uint32_t* __restrict__ nn, size_t nn_pitch, int max_n,
                                                                 double max_plane_distance, double* __restrict__ partials, int kPlanePts,
                                                                 const int* __restrict__ active, const int* __restrict__ src_of,
                                                                 const unsigned long long* __restrict__ run_flags) {
    if constexpr (RUNS == 2)
        plane_accum_flagged<FIT>(tree, src, counts, st, nn, nn_pitch, max_n, max_plane_distance, partials, kPlanePts, active, src_of, run_flags);
    else if constexpr (RUNS == 1)
        plane_accum_per_run<FIT>(tree, src, counts, st, nn, nn_pitch, max_n, max_plane_distance, partials, kPlanePts, active, src_of);
    else
        plane_accum_per_point<FIT>(tree, src, counts, st, nn, nn_pitch, max_n, max_plane_distance, partials, kPlanePts, active, src_of);
}

// K2', P2P: CaculateMatrixHAndBP2P (icp_registration.cpp:57-103), including the /16 on the rotation block.
__global__ __launch_bounds__(kBlock) void icp_point_accum_kernel(const uint2* __restrict__ tree, const float4* __restrict__ src,
                                                                 const int* __restrict__ counts, const PoseState* __restrict__ st,
                                                                 const uint32_t* __restrict__ nn, size_t nn_pitch, int max_n,
                                                                 double max_nn_distance, double* __restrict__ partials, int pts,
                                                                 const int* __restrict__ active, const int* __restrict__ src_of) {
    const int scan = active ? active[blockIdx.y] : (int)blockIdx.y;
    if (st[scan].done) return;
    double acc[28];
#pragma unroll
    for (int v = 0; v < 28; ++v) acc[v] = 0.0;
#pragma unroll 1
    for (int pp = 0; pp < pts; ++pp) {  // several points per thread before the 28-value wave reduction (see the plane kernel)
    const int i = (blockIdx.x * pts + pp) * kBlock + threadIdx.x;
    if (i < counts[scan]) {
        const size_t gi = (size_t)scan * max_n + i;
        const uint32_t s0 = nn[gi];
        if (s0 != kInvalidSlot) {
            const float4 p = src[src_index(src_of, scan, max_n, i)];
            const D3 q{(double)p.x, (double)p.y, (double)p.z};
            const D3 qs = se3_apply(st[scan].q, st[scan].t, q);
            const D3 e3 = leaf_point(tree, s0) - qs;
            const double dis2 = dot3(e3, e3);
            if (!(dis2 > max_nn_distance)) {
                acc[27] += 1.0;
                double Rh[3][3];
                R_hat(st[scan].R, q, Rh);
                double J[3][6];
#pragma unroll
                for (int r = 0; r < 3; ++r)
#pragma unroll
                    for (int c = 0; c < 3; ++c) { J[r][c] = Rh[r][c] / 16; J[r][3 + c] = (r == c) ? -1.0 : 0.0; }
                const double e[3] = {e3.x, e3.y, e3.z};
                add_rows<3>(acc, J, e);
            }
        }
    }
    }
    block_reduce_store<28, kAccW>(acc, partials + ((size_t)scan * gridDim.x + blockIdx.x) * kAccW);
}

// K2'', LOCGPU_P2PLANE_MAP: CaculateMatrixHAndBP2Plane (icp_registration.cpp:161-213) with the per-query math::FitPlane
// (math_utils.h:112-136) replaced by a look-up of the plane fitted at ingest for the NEAREST leaf (map_planes.hip). Per point: the
// source point, one slot word, one 32-byte row planes[slot >> 1] (four NaNs = no valid plane) — no leaf load, no SVD. J and dis in the
// plane kernel's coefficient order; sums per thread and one wave reduction per block like the point kernel.
__global__ __launch_bounds__(kBlock) void icp_mapplane_accum_kernel(const double4* __restrict__ planes, const float4* __restrict__ src,
                                                                    const int* __restrict__ counts, const PoseState* __restrict__ st,
                                                                    const uint32_t* __restrict__ nn, int max_n, double max_plane_distance,
                                                                    double* __restrict__ partials, int pts, const int* __restrict__ active,
                                                                    const int* __restrict__ src_of) {
    const int scan = active ? active[blockIdx.y] : (int)blockIdx.y;
    if (st[scan].done) return;
    double acc[28];
#pragma unroll
    for (int v = 0; v < 28; ++v) acc[v] = 0.0;
    const int n = counts[scan];
    const size_t region = src_index(src_of, scan, max_n, 0);
#pragma unroll 1
    for (int pp = 0; pp < pts; ++pp) {
        const int i = (blockIdx.x * pts + pp) * kBlock + threadIdx.x;
        if (i < n) {
            const uint32_t s0 = __builtin_nontemporal_load(&nn[(size_t)scan * max_n + i]);
            const float4 p = src[region + i];
            if (s0 != kInvalidSlot) {  // a non-finite source point is no query (the search left it the empty list)
                const double4 n4 = planes[s0 >> 1];
                if (n4.x == n4.x) {
                    acc[27] += 1.0;  // effective_num++ before the residual gate (icp cpp:184)
                    const D3 n3{n4.x, n4.y, n4.z};
                    const D3 q{(double)p.x, (double)p.y, (double)p.z};
                    const D3 qs = se3_apply(st[scan].q, st[scan].t, q);
                    const double dis = dot3(n3, qs) + n4.w;
                    if (!(fabs(dis) > max_plane_distance)) {
                        double J[1][6];
                        plane_row(n3, st[scan].R, q, J[0]);
                        const double e[1] = {dis};
                        add_rows<1>(acc, J, e);
                    }
                }
            }
        }
    }
    block_reduce_store<28, kAccW>(acc, partials + ((size_t)scan * gridDim.x + blockIdx.x) * kAccW);
}

// K2', P2Line: CaculateMatrixHAndBP2Line (icp_registration.cpp:105-159) + math::FitLine (math_utils.h:138-163).
__global__ __launch_bounds__(kBlock) __attribute__((amdgpu_waves_per_eu(5, 5))) void icp_line_accum_kernel(const uint2* __restrict__ tree, const float4* __restrict__ src,
                                                                const int* __restrict__ counts, const PoseState* __restrict__ st,
                                                                const uint32_t* __restrict__ nn, size_t nn_pitch, int max_n,
                                                                double max_line_distance, double* __restrict__ partials, int pts,
                                                                const int* __restrict__ active, const int* __restrict__ src_of) {
    __shared__ double s_row[8][kAccPad];
    __shared__ double s_slice[kBlock / 32][32];
    const int scan = active ? active[blockIdx.y] : (int)blockIdx.y;
    if (st[scan].done) return;
    RowAccum ra;
    ra.init();
#pragma unroll 1
    for (int pp = 0; pp < pts; ++pp) {
    const int i = (blockIdx.x * pts + pp) * kBlock + threadIdx.x;
    double J[3][6], neg_e[3] = {0.0, 0.0, 0.0};
    double fitted = 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 6; ++c) J[r][c] = 0.0;
    if (i < counts[scan]) {
        const size_t gi = (size_t)scan * max_n + i;
        uint32_t slot[5];  // one round trip for the five indices and the point (see the plane kernel)
#pragma unroll
        for (int j = 0; j < 5; ++j) slot[j] = nn[(size_t)j * nn_pitch + gi];
        const float4 p = src[src_index(src_of, scan, max_n, i)];
        if (slot[4] != kInvalidSlot) {  // nn.size() == 5
            const D3 q{(double)p.x, (double)p.y, (double)p.z};
            const D3 qs = se3_apply(st[scan].q, st[scan].t, q);
            D3 nb[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) nb[j] = leaf_point(tree, slot[j]);
            D3 sum{0.0, 0.0, 0.0};
#pragma unroll
            for (int j = 0; j < 5; ++j) sum = sum + nb[j];
            const D3 p0{sum.x / 5.0, sum.y / 5.0, sum.z / 5.0};
            D3 dl[5];
#pragma unroll
            for (int j = 0; j < 5; ++j) dl[j] = nb[j] - p0;
            const D3 d = line_direction(dl);
            bool fit = true;
#pragma unroll
            for (int j = 0; j < 5; ++j) {
                const D3 c = cross3(d, nb[j] - p0);
                if (dot3(c, c) > max_line_distance) fit = false;
            }
            if (fit) {
                fitted = 1.0;
                const D3 e3 = cross3(d, qs - p0);  // SO3::hat(d) * (qs - p0)
                if (!(sqrt(dot3(e3, e3)) > max_line_distance)) {
                    const double hd[3][3] = {{0.0, -d.z, d.y}, {d.z, 0.0, -d.x}, {-d.y, d.x, 0.0}};
                    const double hq[3][3] = {{0.0, -q.z, q.y}, {q.z, 0.0, -q.x}, {-q.y, q.x, 0.0}};
                    const double* R = st[scan].R;
                    double hR[3][3], A[3][3];
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            double s = hd[r][0] * R[c];
                            s += hd[r][1] * R[3 + c];
                            s += hd[r][2] * R[6 + c];
                            hR[r][c] = s;
                        }
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) {
                            double s = hR[r][0] * hq[0][c];
                            s += hR[r][1] * hq[1][c];
                            s += hR[r][2] * hq[2][c];
                            A[r][c] = s;
                        }
#pragma unroll
                    for (int r = 0; r < 3; ++r)
#pragma unroll
                        for (int c = 0; c < 3; ++c) { J[r][c] = -A[r][c]; J[r][3 + c] = hd[r][c]; }
                    neg_e[0] = -e3.x; neg_e[1] = -e3.y; neg_e[2] = -e3.z;
                }
            }
        }
    }
    ra.add<3>(s_row, J, neg_e, fitted);
    }
    ra.store(s_slice, partials + ((size_t)scan * gridDim.x + blockIdx.x) * kAccW);
}

// Sum of the block partials of one scan, per column, in a fixed order (chunk c takes rows c, c + 8, …; the chunks are then added in
// order). Many loads are in flight per thread: a single-scan alignment has 450 rows, and a row-by-row load → add chain made this the
// longest part of the solve kernel. Returns the column total in threads 0..kAccW-1 (0 elsewhere). Ends with the block synchronised.
__device__ __forceinline__ double reduce_partials(const double* __restrict__ rows, int blocks_per_scan, bool mine, double (*s_sum)[kAccW]) {
    const int col = threadIdx.x & (kAccW - 1), chunk = threadIdx.x / kAccW;
    constexpr int kChunks = kBlock / kAccW;
    double s = 0.0;
    if (mine && col < 28) {
        constexpr int kFlight = 32;  // loads in flight per thread (round 5: 8 → 32: a one-scan alignment's 450 rows are two rounds instead of seven; the order of the sums — row after row within a chunk — is unchanged, so are the bits)
        for (int b = chunk; b < blocks_per_scan; b += kChunks * kFlight) {
            double v[kFlight];
#pragma unroll
            for (int u = 0; u < kFlight; ++u) {
                const int idx = b + u * kChunks;
                v[u] = idx < blocks_per_scan ? rows[(size_t)idx * kAccW + col] : 0.0;
            }
#pragma unroll
            for (int u = 0; u < kFlight; ++u) s += v[u];
        }
    }
    s_sum[chunk][col] = s;
    __syncthreads();
    double t = 0.0;
    if (threadIdx.x < kAccW) {
        t = s_sum[0][threadIdx.x];
#pragma unroll
        for (int c = 1; c < kChunks; ++c) t += s_sum[c][threadIdx.x];
    }
    __syncthreads();
    return t;
}

// ---------------------------------------------------------------------------------------------
// K3: one 256-thread block per scan. Sums the block partials in a fixed order, then thread 0 runs the
// reference's checks and update (icp_registration.cpp:204-211 + 362-375; ndt_registration.cpp:435-459).
// hb_out (optional): per scan 44 doubles = H (36, row-major), B (6), effective_num, ok.
// scans (optional): the scans to solve — block i takes scan scans[i] (a scan pool solves its open slots only, scan_pool.hip).
__device__ __forceinline__ void gn_update(const double* tot, PoseState& ps, const GnParams& prm, int do_update, double* __restrict__ hb) {
    double H[36], B[6], dx[6] = {0, 0, 0, 0, 0, 0};
    int o = 0;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { H[6 * i + j] = tot[o]; H[6 * j + i] = tot[o]; ++o; }
    for (int i = 0; i < 6; ++i) B[i] = tot[21 + i];
    const long long eff = (long long)tot[27];
    bool ok;
    const double det = lu6_det_solve_reg(H, B, dx);  // in registers: unrolled, pivot rows swapped in with selects (device_math.hpp)
    auto write_hb = [&](double okv) {
        if (!hb) return;
        for (int i = 0; i < 36; ++i) hb[i] = H[i];
        for (int i = 0; i < 6; ++i) hb[36 + i] = B[i];
        hb[42] = (double)eff;
        hb[43] = okv;
    };
    if (prm.method == kMethodNdtDirect) {
        // direct NDT: det(H)==0 is tested FIRST and aborts the whole alignment (ndt cpp:435-436)
        if (det == 0.0) {
            ps.status = 1; ps.done = 1; ps.iterations += 1; ps.last_eff = eff;
            write_hb(0.0);
            return;
        }
        ok = eff >= prm.min_effective_pts;
    } else if (prm.method == kMethodNdtInc) {
        // incremental NDT: too few accepted residuals ⇒ `result_pose = pose; return false` (ndt cpp:349-353); no det(H) test
        ok = eff >= prm.min_effective_pts;
        if (!ok) {
            ps.status = 2; ps.done = 1; ps.iterations += 1; ps.last_eff = eff;
            write_hb(0.0);
            return;
        }
    } else {
        ok = (eff >= prm.min_effective_pts) && !(det == 0.0);
    }
    write_hb(ok ? 1.0 : 0.0);
    ps.last_eff = eff;
    if (!do_update) return;
    ps.iterations += 1;
    if (ok) {
        if (prm.method == LOCGPU_P2P)
            for (int i = 0; i < 6; ++i) dx[i] = dx[i] / 16;  // dx = H.inverse()/16 * err (icp cpp:287)
        se3_apply_update(ps.q, ps.t, dx);
        quat_to_R(ps.q, ps.R);
        // dx.norm() as the reference's binary sums it: three packets p0 + (p1 + p2), then low + high (libLocUtils.so 0x5b113-0x5b185)
        const double nrm = sqrt((dx[0] * dx[0] + (dx[2] * dx[2] + dx[4] * dx[4])) + (dx[1] * dx[1] + (dx[3] * dx[3] + dx[5] * dx[5])));
        ps.last_dx_norm = nrm;
        if (nrm < prm.eps) { ps.converged = 1; ps.done = 1; }
    }
    if (ps.iterations >= prm.max_iteration) ps.done = 1;
}

__global__ __launch_bounds__(kBlock) void gn_solve_kernel(const double* __restrict__ partials, int blocks_per_scan, PoseState* __restrict__ st,
                                                          GnParams prm, int do_update, double* __restrict__ hb_out, unsigned int* __restrict__ list_counts,
                                                          const int* __restrict__ scans, GnPost post) {
    __shared__ double s_sum[kBlock / kAccW][kAccW];
    const int scan = scans ? scans[blockIdx.x] : (int)blockIdx.x;
    // The search stage's work-list counters (walk kernel → deep pass → redo kernel) are consumed by now: zero them for the next iteration's
    // search instead of paying two fill launches per iteration (a single-scan alignment is launch-latency bound).
    if (list_counts && blockIdx.x == 0 && threadIdx.x < 4) list_counts[threadIdx.x] = 0u;
    if (st[scan].done) return;
    const double col_total = reduce_partials(partials + (size_t)scan * blocks_per_scan * kAccW, blocks_per_scan, true, s_sum);
    if (threadIdx.x < kAccW) s_sum[0][threadIdx.x] = col_total;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double tot[28];
    for (int v = 0; v < 28; ++v) tot[v] = s_sum[0][v];
    PoseState& ps = st[scan];
    gn_update(tot, ps, prm, do_update, hb_out ? hb_out + 44 * (size_t)scan : nullptr);
    if (post.word) {
        // A one-scan alignment paced from the host (locgpu_api.hip, align_finish): a word in pinned host memory says which iteration
        // this was — the host launches the next iteration but one when it sees it — and a finished scan's result goes there too: no
        // chunk of idle launches, no copy, no stream synchronisation on the latency path. Plain stores to fine-grained host memory
        // (they write through); a system-scope RELEASE here writes the whole L2 back — ≈12 µs per iteration, measured — so the
        // record is sealed by a checksum instead of a fence: the host takes it when the sum over what it reads matches.
        const unsigned long long tag = ((unsigned long long)post.call << 32) | ((unsigned long long)(unsigned int)ps.iterations << 1) | (ps.done ? 1ull : 0ull);
        if (ps.done) {
            GnPostRecord r;
            for (int i = 0; i < 4; ++i) r.w[i] = __double_as_longlong(ps.q[i]);
            for (int i = 0; i < 3; ++i) r.w[4 + i] = __double_as_longlong(ps.t[i]);
            r.w[7] = __double_as_longlong(ps.last_dx_norm);
            r.w[8] = (unsigned long long)ps.last_eff;
            r.w[9] = ((unsigned long long)(unsigned int)ps.converged << 32) | (unsigned int)ps.status;
            typedef unsigned long long u64x2 __attribute__((ext_vector_type(2)));
            volatile u64x2* to = reinterpret_cast<volatile u64x2*>(post.record);
            for (int i = 0; i < GnPostRecord::kWords / 2; ++i) to[i] = u64x2{r.w[2 * i], r.w[2 * i + 1]};
            *reinterpret_cast<volatile u64x2*>(post.word) = u64x2{tag, gn_post_sum(tag, r)};
        } else {
            __hip_atomic_store(post.word, tag, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        }
    }
}

// The LOAM matcher's solve (loam_registration.cpp:47-90): one 256-thread block per scan over TWO sets of block partials — the surface
// class's, then the edge class's, each summed in reduce_partials' fixed order with its own blocks_per_scan. Thread 0 then applies the
// reference's rules: a class is false iff its effective_num < min_effective_pts or its own det(H) == 0 (icp_registration.cpp:204-211),
// surface tested first (:53-70: status 3 / 4, the alignment ends, the pose is not handed out); otherwise dx = (H_surf + H_edge)⁻¹
// (B_surf + B_edge) with NO test on the sum (:76-79), the decoupled update (:82-83) and the stop at |dx| < eps (:85). det(H_sum) == 0 —
// where the reference divides by zero — is an iteration without an update, as locgpu_gn_update has it. The three factorisations run
// one after the other through the same H, B registers. Both classes' local stages read the ONE PoseState written here.
__global__ __launch_bounds__(kBlock) void loam_solve_kernel(LoamSolveArgs a) {
    __shared__ double s_sum[kBlock / kAccW][kAccW];
    __shared__ double s_tot[2][kAccW];
    const int scan = a.scans ? a.scans[blockIdx.x] : (int)blockIdx.x;
    // both batches' search work lists are consumed by now (see gn_solve_kernel)
    if (blockIdx.x == 0 && threadIdx.x < 4) {
        if (a.list_counts[0]) a.list_counts[0][threadIdx.x] = 0u;
        if (a.list_counts[1]) a.list_counts[1][threadIdx.x] = 0u;
    }
    if (a.st[scan].done) return;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        double t = 0.0;
        if (a.partials[c]) t = reduce_partials(a.partials[c] + (size_t)scan * a.blocks_per_scan[c] * kAccW, a.blocks_per_scan[c], true, s_sum);
        if (threadIdx.x < kAccW) s_tot[c][threadIdx.x] = t;
    }
    __syncthreads();
    if (threadIdx.x != 0) return;
    PoseState& ps = a.st[scan];
    double H[36], B[6], dx[6];
    long long eff[2] = {0, 0};
    bool ok[2] = {true, true};  // a class that is switched off is never evaluated: it cannot report false
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        if (!a.partials[c]) continue;
        int o = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j) { H[6 * i + j] = s_tot[c][o]; H[6 * j + i] = s_tot[c][o]; ++o; }
        for (int i = 0; i < 6; ++i) B[i] = s_tot[c][21 + i];
        eff[c] = (long long)s_tot[c][27];
        const double det_c = lu6_det_solve_reg(H, B, dx);
        ok[c] = (eff[c] >= a.min_effective_pts[c]) && !(det_c == 0.0);
    }
    {
        int o = 0;
        for (int i = 0; i < 6; ++i)
            for (int j = i; j < 6; ++j) { const double v = s_tot[0][o] + s_tot[1][o]; H[6 * i + j] = v; H[6 * j + i] = v; ++o; }
        for (int i = 0; i < 6; ++i) { B[i] = s_tot[0][21 + i] + s_tot[1][21 + i]; dx[i] = 0.0; }
    }
    if (a.hb_out) {
        double* hb = a.hb_out + (size_t)kLoamHbW * scan;
        for (int i = 0; i < 36; ++i) hb[i] = H[i];
        for (int i = 0; i < 6; ++i) hb[36 + i] = B[i];
        hb[42] = (double)eff[0]; hb[43] = (double)eff[1];
        hb[44] = ok[0] ? 1.0 : 0.0; hb[45] = ok[1] ? 1.0 : 0.0;
    }
    ps.last_eff = eff[0] + eff[1];
    if (!a.do_update) return;
    ps.iterations += 1;
    if (!ok[0] || !ok[1]) {
        ps.status = !ok[0] ? 3 : 4;
        ps.done = 1;
        return;
    }
    const double det = lu6_det_solve_reg(H, B, dx);
    if (!(det == 0.0)) {
        se3_apply_update(ps.q, ps.t, dx);
        quat_to_R(ps.q, ps.R);
        const double nrm = sqrt((dx[0] * dx[0] + (dx[2] * dx[2] + dx[4] * dx[4])) + (dx[1] * dx[1] + (dx[3] * dx[3] + dx[5] * dx[5])));  // as gn_update sums it
        ps.last_dx_norm = nrm;
        if (nrm < a.eps) { ps.converged = 1; ps.done = 1; }
    }
    if (ps.iterations >= a.max_iteration) ps.done = 1;
}

// First half of gn_solve_kernel for sharded batches (see launch.hpp): one block per GLOBAL scan.
// owned (optional, scan pools): owned[g] != 0 where this rank holds the points of slot g; then first = 0 and n_local = all slots.
__global__ __launch_bounds__(kBlock) void sum_partials_kernel(const double* __restrict__ partials, int blocks_per_scan, const PoseState* __restrict__ st_all,
                                                              int first, int n_local, double* __restrict__ acc, const unsigned char* __restrict__ owned) {
    __shared__ double s_sum[kBlock / kAccW][kAccW];
    const int g = blockIdx.x;
    const int scan = g - first;
    const bool mine = scan >= 0 && scan < n_local && !st_all[g].done && (!owned || owned[g]);  // a finished scan's partials are stale: contribute zeros (nobody reads them)
    const double t = reduce_partials(partials + (size_t)(mine ? scan : 0) * blocks_per_scan * kAccW, blocks_per_scan, mine, s_sum);
    if (threadIdx.x < kAccW) acc[(size_t)g * kAccW + threadIdx.x] = threadIdx.x < 28 ? t : 0.0;
}

// pcl::transformPointCloud with the float32 4×4 (icp_registration.cpp:241): ((m0·x + m1·y) + m2·z) + m3 per row.
// The 3×4 matrix travels as a kernel argument (no upload in front of the launch); the output is packed x, y, z — what goes back to the
// caller's cloud, whose other fields are the source's (locgpu_api.hip, write_output_cloud).
__global__ __launch_bounds__(kBlock) void transform_cloud_kernel(const float4* __restrict__ src, size_t n, M12f m, float* __restrict__ dst_xyz) {
    const size_t i = (size_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float4 p = src[i];
    const float* m12 = m.v;
    dst_xyz[3 * i + 0] = ((m12[0] * p.x + m12[1] * p.y) + m12[2] * p.z) + m12[3];
    dst_xyz[3 * i + 1] = ((m12[4] * p.x + m12[5] * p.y) + m12[6] * p.z) + m12[7];
    dst_xyz[3 * i + 2] = ((m12[8] * p.x + m12[9] * p.y) + m12[10] * p.z) + m12[11];
}

// Launchers (declared in launch.hpp).
// LOCGPU_PLANE_FIT (read once): 1 = secular-equation fit (plane_null_vector_secular), 0 = the 4-column Jacobi fit.
int plane_fit_mode() {
    static const int mode = [] { const char* e = getenv("LOCGPU_PLANE_FIT"); return e && *e ? atoi(e) : 1; }();  // not env_int: an empty value is the default too
    return mode;
}
// LOCGPU_PLANE_DEDUP (read once): 1 (default) = one plane fit per run of equal neighbour sets (plane_accum_per_run), 0 = a fit per
// point (plane_accum_per_point). The two give the same bits. With 1, a launch whose search stage wrote run flags
// (LOCGPU_PLANE_RUNFLAGS, gn_driver.hip) takes the runs from them (plane_accum_flagged) — the same bits again.
static bool plane_dedup() {
    static const bool on = env_int("LOCGPU_PLANE_DEDUP", 1) != 0;
    return on;
}

// Points per thread of the accumulate kernels for a batch of n_scans scans of at most max_n points: amortise the block reduction
// when the batch already fills the chip; 1 for small launches (latency). The plane kernel's reduction is cheap (LDS rows, see
// there): 4 is as good as 8 and leaves a finer tail; the line and point kernels still pay a 28-value wave reduction per block.
int icp_accum_split(int method, int max_n, int n_scans) {
    static_assert(kDedupPP >= 4, "the plane table of plane_accum_per_run has room for the largest plane rung below");
    const long total_blocks = (long)((max_n + kBlock - 1) / kBlock) * n_scans;
    return total_blocks >= 8192 ? (method == LOCGPU_P2PLANE ? 4 : 8) : (total_blocks >= 4096 ? 4 : (total_blocks >= 2048 ? 2 : 1));
}

int launch_icp_accum(int method, const AccumArgs& a, hipStream_t s) {
    const int blocks = (a.max_n + kBlock - 1) / kBlock;
    int pts = icp_accum_split(method, a.max_n, a.n_scans);  // ALL scans of the batch, open or not: the split — hence the order of the sums — must not depend on a.active
    if (a.split_scans > 0) pts = icp_accum_split(method, a.max_n, a.split_scans);
    const dim3 grid((blocks + pts - 1) / pts, a.active ? a.n_active : a.n_scans);
    if (method == LOCGPU_P2PLANE) {
        const bool secular = plane_fit_mode() == 1;
        // pts <= kDedupPP always (the static_assert in icp_accum_split); were a larger rung added without the table growing, the launch
        // would still be right, a fit per point
        const bool runs = plane_dedup() && pts <= kDedupPP;
        auto kernel = !runs ? (secular ? icp_plane_accum_kernel<1, 0> : icp_plane_accum_kernel<0, 0>)
                      : !a.run_flags ? (secular ? icp_plane_accum_kernel<1, 1> : icp_plane_accum_kernel<0, 1>)
                                     : (secular ? icp_plane_accum_kernel<1, 2> : icp_plane_accum_kernel<0, 2>);
        hipLaunchKernelGGL(kernel, grid, dim3(kBlock), 0, s, a.tree, a.src, a.counts, a.st, a.nn, a.nn_pitch, a.max_n, a.gate, a.partials, pts, a.active, a.src_of, a.run_flags);
    } else if (method == LOCGPU_P2PLANE_MAP)
        hipLaunchKernelGGL(icp_mapplane_accum_kernel, grid, dim3(kBlock), 0, s, reinterpret_cast<const double4*>(a.planes), a.src, a.counts, a.st, a.nn, a.max_n, a.gate, a.partials, pts, a.active, a.src_of);
    else if (method == LOCGPU_P2LINE)
        hipLaunchKernelGGL(icp_line_accum_kernel, grid, dim3(kBlock), 0, s, a.tree, a.src, a.counts, a.st, a.nn, a.nn_pitch, a.max_n, a.gate, a.partials, pts, a.active, a.src_of);
    else
        hipLaunchKernelGGL(icp_point_accum_kernel, grid, dim3(kBlock), 0, s, a.tree, a.src, a.counts, a.st, a.nn, a.nn_pitch, a.max_n, a.gate, a.partials, pts, a.active, a.src_of);
    return (int)grid.x;
}

void launch_gn_solve(const double* partials, int blocks_per_scan, PoseState* st, int n_scans, const GnParams& prm, int do_update, double* hb_out,
                     unsigned int* list_counts, hipStream_t s, const int* scans, const GnPost* post) {
    hipLaunchKernelGGL(gn_solve_kernel, dim3(n_scans), dim3(kBlock), 0, s, partials, blocks_per_scan, st, prm, do_update, hb_out, list_counts, scans, post ? *post : GnPost{});
}

void launch_loam_solve(const LoamSolveArgs& a, int n_scans, hipStream_t s) {
    hipLaunchKernelGGL(loam_solve_kernel, dim3(n_scans), dim3(kBlock), 0, s, a);
}

void launch_sum_partials(const double* partials, int blocks_per_scan, const PoseState* st_all, int first, int n_local, int n_total, double* acc,
                         hipStream_t s, const unsigned char* owned) {
    hipLaunchKernelGGL(sum_partials_kernel, dim3(n_total), dim3(kBlock), 0, s, partials, blocks_per_scan, st_all, first, n_local, acc, owned);
}

void launch_transform_cloud(const float4* src, size_t n, const M12f& m12, float* dst_xyz, hipStream_t s) {
    hipLaunchKernelGGL(transform_cloud_kernel, dim3((unsigned)((n + kBlock - 1) / kBlock)), dim3(kBlock), 0, s, src, n, m12, dst_xyz);
}

}  // namespace locgpu
