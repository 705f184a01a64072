// loc_lib_amd/csrc/forest_build.hip — the ICP target's packed KD-trees built ON THE DEVICE from points resident in HBM:
// locgpu_icp_set_target_forest_device (the forest of the pairs calls, from a resident batch), locgpu_icp_set_target_cloud_device (one
// tree, an ordinary target, from a resident cloud), and the read-back both builds are compared through.
//
// The tree is kdtree_build.cpp's, slot for slot: split thresholds are float32 sums taken SEQUENTIALLY in index order, so one node's sum
// is a serial chain — but nodes of a level, trees and the three coordinates are independent, the terms (p − m)², the partition flags,
// their prefix positions and the scatter are order-free, and without a degenerate split every slot position is known top-down
// (forest_plan.hpp). One workgroup builds one tree, level by level; the records {x, y, z, id} ping-pong between two global arrays.
// A degenerate split (every point of a node on one side: duplicates, NaNs) makes positions unknowable top-down: the kernel only
// flags it, and the entry point takes the host path for the whole call.
//
// Float semantics the bytes depend on (checked in the compiler's output): -ffp-contract=off (no FMA across the
// variance's multiply and add), correctly rounded float32 division and float32 subnormals kept — hipcc's defaults for gfx950.
// No atomics: flags are plain stores of one value.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "cloud_filters.hpp"
#include "context.hpp"
#include "env.hpp"
#include "forest_build.hpp"
#include "kdtree_build.hpp"
#include "search_dispatch.hpp"

using namespace locgpu;
using fplan::Node;
using fplan::Rec;
using fplan::Slot;

static_assert(sizeof(Rec) == sizeof(float4) && sizeof(Slot) == sizeof(uint2) && sizeof(Node) == 16, "layouts");
static_assert(kFbTile % 64 == 0 && kFbLaneLen >= 2, "tile");
static_assert(fplan::kMaxDepth == kMaxSearchDepth, "depth limit");

namespace {

// Lanes of one wave hand data to each other through LDS: a wave's LDS operations execute in program order, so all that is needed is
// that the compiler keeps them in that order.
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// One pass of a wave over a node's points: every lane computes the three terms of its points (term(p, out[3])) into the wave's LDS
// tile, then lane c < 3 adds coordinate c's terms to `acc` one by one in index order. Returns acc of lanes 0..2 in (a0, a1, a2).
template <class Term>
__device__ __forceinline__ void chain_pass(const Rec* src, uint32_t len, float* tile, int lane, Term term, float& a0, float& a1, float& a2) {
    float acc = 0.f;
    for (uint32_t first = 0; first < len; first += kFbTile) {
        const uint32_t m = min((uint32_t)kFbTile, len - first);
        for (uint32_t k = lane; k < m; k += 64) {
            float t[3];
            term(src[first + k], t);
            tile[k] = t[0];
            tile[kFbTile + k] = t[1];
            tile[2 * kFbTile + k] = t[2];
        }
        wave_sync();
        if (lane < 3) {
            const float* tp = tile + lane * kFbTile;
            uint32_t k = 0;
            for (; k + 16 <= m; k += 16) {  // four LDS reads in flight under the sixteen dependent adds; the order of the adds is the index order
                const float4 q0 = *reinterpret_cast<const float4*>(tp + k), q1 = *reinterpret_cast<const float4*>(tp + k + 4);
                const float4 q2 = *reinterpret_cast<const float4*>(tp + k + 8), q3 = *reinterpret_cast<const float4*>(tp + k + 12);
                acc = acc + q0.x; acc = acc + q0.y; acc = acc + q0.z; acc = acc + q0.w;
                acc = acc + q1.x; acc = acc + q1.y; acc = acc + q1.z; acc = acc + q1.w;
                acc = acc + q2.x; acc = acc + q2.y; acc = acc + q2.z; acc = acc + q2.w;
                acc = acc + q3.x; acc = acc + q3.y; acc = acc + q3.z; acc = acc + q3.w;
            }
            for (; k + 4 <= m; k += 4) {
                const float4 q = *reinterpret_cast<const float4*>(tp + k);
                acc = acc + q.x; acc = acc + q.y; acc = acc + q.z; acc = acc + q.w;
            }
            for (; k < m; ++k) acc = acc + tp[k];
        }
        wave_sync();
    }
    a0 = __shfl(acc, 0);
    a1 = __shfl(acc, 1);
    a2 = __shfl(acc, 2);
}

// The split of one node by one wave: Builder::split's arithmetic with the sums' operands in the same order.
__device__ __forceinline__ fplan::Split wave_split(const Rec* src, Rec* dst, uint32_t len, float* tile, int lane) {
    float sx, sy, sz;
    chain_pass(src, len, tile, lane, [](const Rec& p, float* t) { t[0] = p.x; t[1] = p.y; t[2] = p.z; }, sx, sy, sz);
    const float fl = (float)len;
    const float mx = sx / fl, my = sy / fl, mz = sz / fl;
    float vx, vy, vz;
    chain_pass(src, len, tile, lane, [=](const Rec& p, float* t) {
        const float dx = p.x - mx, dy = p.y - my, dz = p.z - mz;
        t[0] = dx * dx; t[1] = dy * dy; t[2] = dz * dz;
    }, vx, vy, vz);
    const float fl1 = (float)(len - 1);
    vx = vx / fl1; vy = vy / fl1; vz = vz / fl1;
    fplan::Split s;
    s.axis = fplan::pick_axis(vx, vy, vz);
    s.th = s.axis == 0 ? mx : (s.axis == 1 ? my : mz);
    // four 64-point chunks a round: their loads are in flight together (a long node is one wave's work, and latency is all it waits for)
    uint32_t nl = 0;
    for (uint32_t first = 0; first < len; first += 256) {
        bool left[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t k = first + 64 * u + lane;
            left[u] = k < len && fplan::coord(src[k], s.axis) < s.th;
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) nl += (uint32_t)__popcll(__ballot(left[u]));
    }
    uint32_t l = 0, r = nl;
    const unsigned long long below = (1ull << lane) - 1ull;
    for (uint32_t first = 0; first < len; first += 256) {
        Rec p[4];
        bool in[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const uint32_t k = first + 64 * u + lane;
            in[u] = k < len;
            p[u] = Rec{0.f, 0.f, 0.f, 0};
            if (in[u]) p[u] = src[k];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {  // the chunks in index order: the partition is stable
            const bool left = in[u] && fplan::coord(p[u], s.axis) < s.th;
            const bool right = in[u] && !left;
            const unsigned long long ml = __ballot(left), mr = __ballot(right);
            if (left) dst[l + (uint32_t)__popcll(ml & below)] = p[u];
            if (right) dst[r + (uint32_t)__popcll(mr & below)] = p[u];
            l += (uint32_t)__popcll(ml);
            r += (uint32_t)__popcll(mr);
        }
    }
    s.nl = nl;
    return s;
}

__global__ __launch_bounds__(kFbThreads) void forest_build_kernel(const float4* src, const ForestBuildTab* tab, float4* recs_all, size_t points, Node* nodes_all,
                                                                    size_t node_entries, uint2* tree, uint32_t* leaf_all, ForestBuildRes* res) {
    __shared__ __attribute__((aligned(16))) float s_tile[kFbWaves][3 * kFbTile];
    __shared__ uint32_t s_wave_total[kFbWaves];
    __shared__ uint32_t s_count, s_stop, s_unbounded, s_degenerate;
    const ForestBuildTab t = tab[blockIdx.x];
    const uint32_t n = t.n;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    Rec* rec[2] = {reinterpret_cast<Rec*>(recs_all) + t.pt_off, reinterpret_cast<Rec*>(recs_all) + points + t.pt_off};
    Node* list[2] = {nodes_all + t.node_off, nodes_all + node_entries + t.node_off};
    Slot* slots = reinterpret_cast<Slot*>(tree) + t.base;
    uint32_t* leaf_slots = leaf_all + t.pt_off;

    if (tid == 0) {
        s_count = n > 1 ? 1u : 0u;
        s_stop = 0;
        s_unbounded = 0;
        s_degenerate = 0;
        fplan::write_sentinel(slots + fplan::tree_slots(n));
        if (t.pad) slots[fplan::tree_slots(n) + 2] = Slot{0u, 0u};
        if (n > 1) list[0][0] = Node{0u, n, 0u, 0u};
    }
    __syncthreads();
    for (uint32_t i = tid; i < n; i += kFbThreads) {
        const float4 p = src[t.src_off + i];
        const Rec r{p.x, p.y, p.z, (int32_t)i};
        rec[0][i] = r;
        if (!(fplan::float_bounded(p.x) && fplan::float_bounded(p.y) && fplan::float_bounded(p.z))) s_unbounded = 1u;
        if (n == 1) { fplan::write_leaf(slots, r); leaf_slots[0] = 0u; }
    }
    __syncthreads();

    // Level `level` holds the nodes of list[cur], all of at least two points; their children stand on level + 1.
    int level = 1, cur = 0;
    bool too_deep = false;
    for (;;) {
        const uint32_t count = s_count;  // written behind the previous level's second barrier, together with s_stop
        if (count == 0 || s_stop) break;
        if (level >= fplan::kMaxDepth) { too_deep = true; break; }
        const Rec* from = rec[cur];
        Rec* to = rec[cur ^ 1];
        Node* now = list[cur];
        Node* next = list[cur ^ 1];
        // the long nodes, a wave each
        for (uint32_t i = wave; i < count; i += kFbWaves) {
            const Node nd = now[i];
            if (nd.len <= (uint32_t)kFbLaneLen) continue;
            const fplan::Split sp = wave_split(from + nd.off, to + nd.off, nd.len, s_tile[wave], lane);
            if (lane == 0) {
                slots[nd.slot] = fplan::node_slot(sp.th, sp.axis, fplan::right_slot(nd.slot, sp.nl));
                now[i].nl = sp.nl;
                if (!fplan::float_bounded(sp.th)) s_unbounded = 1u;
                if (fplan::degenerate(nd.len, sp.nl)) s_degenerate = 1u;
            }
        }
        // the short ones, a lane each
        for (uint32_t i = tid; i < count; i += kFbThreads) {
            const Node nd = now[i];
            if (nd.len > (uint32_t)kFbLaneLen) continue;
            const fplan::Split sp = fplan::split_seq(from + nd.off, to + nd.off, nd.len);
            slots[nd.slot] = fplan::node_slot(sp.th, sp.axis, fplan::right_slot(nd.slot, sp.nl));
            now[i].nl = sp.nl;
            if (!fplan::float_bounded(sp.th)) s_unbounded = 1u;
            if (fplan::degenerate(nd.len, sp.nl)) s_degenerate = 1u;
        }
        __syncthreads();
        // the children: leaves are written, longer ones are listed for the next level in the order of their parents
        const uint32_t chunk = (count + kFbThreads - 1) / kFbThreads;
        const uint32_t lo = min((uint32_t)tid * chunk, count), hi = min(lo + chunk, count);
        uint32_t mine = 0;
        for (uint32_t i = lo; i < hi; ++i) mine += fplan::child_nodes(now[i]);
        uint32_t incl = mine;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if (lane >= d) incl += up;
        }
        if (lane == 63) s_wave_total[wave] = incl;
        __syncthreads();
        uint32_t before = 0, total = 0;
        for (int w = 0; w < kFbWaves; ++w) {
            const uint32_t v = s_wave_total[w];
            if (w < wave) before += v;
            total += v;
        }
        uint32_t at = before + incl - mine;
        for (uint32_t i = lo; i < hi; ++i) {
            const Node nd = now[i];
            fplan::emit_children(nd, to, slots, leaf_slots, next + at);
            at += fplan::child_nodes(nd);
        }
        if (tid == 0) { s_count = total; s_stop = s_degenerate; }
        __syncthreads();
        cur ^= 1;
        ++level;
    }
    if (tid == 0) {
        ForestBuildRes out;
        out.depth = level;  // the last level that was split, + 1: where its children stand (a tree of one point: 1)
        out.flags = (s_unbounded ? kFbUnbounded : 0u) | (s_degenerate ? kFbDegenerate : 0u) | (too_deep ? kFbTooDeep : 0u);
        res[blockIdx.x] = out;
    }
}

}  // namespace

void locgpu::launch_forest_build(const float4* src, const ForestBuildTab* tab, int n_trees, float4* recs, size_t points, Node* nodes, size_t node_entries, uint2* tree,
                                 uint32_t* leaf_slots, ForestBuildRes* res, hipStream_t s) {
    hipLaunchKernelGGL(forest_build_kernel, dim3((unsigned)n_trees), dim3(kFbThreads), 0, s, src, tab, recs, points, nodes, node_entries, tree, leaf_slots, res);
}

void locgpu::forest_build_free(locgpu_ctx* ctx) {
    delete ctx->fbuild;
    ctx->fbuild = nullptr;
}

// --------------------------------------------------------------------------------------------- entry points
namespace {

struct BuildOutcome {
    std::vector<uint32_t> base;
    std::vector<size_t> leaves;
    std::vector<int> depth;
    size_t total_slots = 0, points = 0;
    int max_depth = 0, levels = 0, first_degenerate = -1, first_deep = -1;
    bool bounded = true;
};

// Runs the kernel over n_trees ranges of `src` (tree j: n[j] points from src_off[j]) into the scratch's own tree and leaf arrays.
// Nothing of the context's target is touched. Returns a locgpu_status; size refusals carry build_packed_forest's texts.
int build_on_device(locgpu_ctx* ctx, const float4* src, const std::vector<size_t>& src_off, const std::vector<size_t>& n, const char* who, BuildOutcome& out) {
    const size_t n_trees = n.size();
    size_t points = 0;
    for (size_t j = 0; j < n_trees; ++j) {
        // 3n-1 slots of 8 bytes must stay below 4 GiB: the search kernel addresses the tree through a 32-bit buffer offset
        if (n[j] >= (1ull << 29) / 3) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": target " + std::to_string(j) + ": target cloud too large (the packed tree must stay below 4 GiB)");
        points += n[j];
    }
    const std::string too_large = std::string(who) + ": target clouds too large (the packed forest must stay below 4 GiB)";
    if (points >= kForestMaxSlots) return fail(ctx, LOCGPU_ERR_INVALID, too_large);
    out.base.resize(n_trees);
    if (!fplan::plan_bases(n.data(), n_trees, kForestMaxSlots, out.base.data(), &out.total_slots)) return fail(ctx, LOCGPU_ERR_INVALID, too_large);
    std::vector<ForestBuildTab> tab(n_trees);
    size_t pt = 0, nodes = 0;
    for (size_t j = 0; j < n_trees; ++j) {
        ForestBuildTab& t = tab[j];
        t.src_off = src_off[j];
        t.pt_off = (uint32_t)pt;
        t.node_off = (uint32_t)nodes;
        t.n = (uint32_t)n[j];
        t.base = out.base[j];
        t.pad = j + 1 < n_trees && out.base[j + 1] != fplan::segment_end(out.base[j], n[j]) ? 1u : 0u;
        t.reserved = 0;
        pt += n[j];
        nodes += n[j] / 2 + 1;
    }
    if (!ctx->fbuild) ctx->fbuild = new ForestBuildScratch();
    ForestBuildScratch& sc = *ctx->fbuild;
    if (2 * points > sc.recs.cap()) LOCGPU_HIP(ctx, sc.recs.alloc(with_headroom(2 * points)));
    if (2 * nodes > sc.nodes.cap()) LOCGPU_HIP(ctx, sc.nodes.alloc(with_headroom(2 * nodes)));
    if (n_trees > sc.tab.cap()) LOCGPU_HIP(ctx, sc.tab.alloc(with_headroom(n_trees)));
    if (n_trees > sc.res.cap()) LOCGPU_HIP(ctx, sc.res.alloc(with_headroom(n_trees)));
    if (out.total_slots > sc.tree.cap()) LOCGPU_HIP(ctx, sc.tree.alloc(with_headroom(out.total_slots)));
    if (points > sc.leaf_slots.cap()) LOCGPU_HIP(ctx, sc.leaf_slots.alloc(with_headroom(points)));
    hipStream_t s = ctx->stream;
    std::vector<ForestBuildRes> res(n_trees);
    static const bool times = env_flag("LOCGPU_FOREST_TIMES");  // diagnostic: the kernel's time on stderr (the host path prints its phases under the same flag)
    if (times) { LOCGPU_HIP(ctx, sc.ev[0].ensure(hipEventDefault)); LOCGPU_HIP(ctx, sc.ev[1].ensure(hipEventDefault)); }
    LOCGPU_HIP(ctx, hipMemcpyAsync(sc.tab, tab.data(), n_trees * sizeof(ForestBuildTab), hipMemcpyHostToDevice, s));
    if (times) LOCGPU_HIP(ctx, hipEventRecord(sc.ev[0], s));
    launch_forest_build(src, sc.tab, (int)n_trees, sc.recs, points, sc.nodes, nodes, sc.tree, sc.leaf_slots, sc.res, s);
    LOCGPU_HIP(ctx, hipGetLastError());
    if (times) LOCGPU_HIP(ctx, hipEventRecord(sc.ev[1], s));
    LOCGPU_HIP(ctx, hipMemcpyAsync(res.data(), sc.res, n_trees * sizeof(ForestBuildRes), hipMemcpyDeviceToHost, s));
    LOCGPU_HIP(ctx, hipStreamSynchronize(s));
    if (times) {
        float ms = 0.f;
        LOCGPU_HIP(ctx, hipEventElapsedTime(&ms, sc.ev[0], sc.ev[1]));
        fprintf(stderr, "[locgpu forest device] forest_build_kernel %.3f ms (%zu trees, %zu points)\n", ms, n_trees, points);
    }
    out.points = points;
    out.leaves.resize(n_trees);
    out.depth.resize(n_trees);
    for (size_t j = 0; j < n_trees; ++j) {
        out.leaves[j] = n[j];
        out.depth[j] = res[j].depth;
        out.max_depth = std::max(out.max_depth, res[j].depth);
        out.levels = std::max(out.levels, res[j].depth - 1);
        if (res[j].flags & kFbUnbounded) out.bounded = false;
        if ((res[j].flags & kFbDegenerate) && out.first_degenerate < 0) out.first_degenerate = (int)j;
        if ((res[j].flags & kFbTooDeep) && out.first_deep < 0) out.first_deep = (int)j;
    }
    return LOCGPU_OK;
}

// The built arrays become the context's target: the old target's arrays become the next build's.
int install_device_build(locgpu_ctx* ctx, const BuildOutcome& o) {
    ForestBuildScratch& sc = *ctx->fbuild;
    (void)target_join(ctx, false);  // a pending asynchronous ingest is superseded
    for (hipStream_t st : ctx->slot_stream) LOCGPU_HIP(ctx, hipStreamSynchronize(st));  // nobody reads the old tree any more (install_tree_meta's own wait, before the swap)
    ctx->d_tree.swap(sc.tree);
    ctx->d_leaf_slots.swap(sc.leaf_slots);
    // tree_slots: up to the LAST tree's sentinel leaf, which then stands where an ordinary tree's does. A tree of n distinct points has
    // n leaves and n − 1 internal nodes.
    const long long meta[6] = {(long long)o.total_slots - 2, (long long)o.points, (long long)(2 * o.points - o.base.size()), (long long)o.points, o.max_depth, o.bounded ? 1 : 0};
    return install_tree_meta(ctx, meta);  // both arrays are large enough: nothing is allocated
}

// what locgpu_icp_device_build_info reports: written only by a call that replaced the target
void note_build(locgpu_ctx* ctx, const BuildOutcome& o, int path, int kind) {
    ForestBuildScratch& sc = *ctx->fbuild;
    sc.last_path = path;
    sc.last_kind = kind;
    sc.first_degenerate = o.first_degenerate;
    sc.levels = o.levels;
}

int refuse_deep(locgpu_ctx* ctx, const char* who, const BuildOutcome& o, bool forest) {
    return fail(ctx, LOCGPU_ERR_DEPTH, std::string(who) + (forest ? ": target " + std::to_string(o.first_deep) : std::string()) + ": KD-tree depth exceeds the " +
                                           std::to_string(kMaxSearchDepth) + "-entry traversal stack");
}

}  // namespace

extern "C" {

int locgpu_icp_set_target_forest_device(locgpu_ctx* ctx, const locgpu_batch* b) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    const char* who = "icp_set_target_forest_device";
    if (!b || b->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": NULL batch or a batch of another context");
    if (b->sharded || b->shared_src) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": sharded and shared-source batches hold no scans of their own");
    if (b->pending.active) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": an alignment of this batch has been begun and not finished");
    if (b->n_scans < 1) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": the batch holds no scan");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    { const int orc = order_behind_batch(ctx, const_cast<locgpu_batch*>(b), "icp_set_target_forest_device: ordering behind the batch"); if (orc != LOCGPU_OK) return orc; }
    const size_t n_trees = (size_t)b->n_scans;
    std::vector<size_t> n(n_trees), off(n_trees);
    for (size_t j = 0; j < n_trees; ++j) {
        if (b->counts[j] <= 0) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": target " + std::to_string(j) + ": empty cloud or stride < 12");
        n[j] = (size_t)b->counts[j];
        off[j] = j * (size_t)b->max_n;
    }
    BuildOutcome o;
    const int brc = build_on_device(ctx, b->d_src, off, n, who, o);
    if (brc != LOCGPU_OK) return brc;
    if (o.first_degenerate >= 0) {  // positions are not known top-down: the host builder measures sizes first — for the whole call
        const int rc = locgpu_icp_set_target_forest_batch(ctx, b);
        if (rc == LOCGPU_OK) note_build(ctx, o, 2, 1);
        return rc;
    }
    if (o.first_deep >= 0) return refuse_deep(ctx, who, o, true);
    if (n_trees > ctx->d_forest_base.cap()) LOCGPU_HIP(ctx, ctx->d_forest_base.alloc(with_headroom(n_trees)));
    const int rc = install_device_build(ctx, o);
    if (rc != LOCGPU_OK) return rc;
    LOCGPU_HIP(ctx, hipMemcpyAsync(ctx->d_forest_base, o.base.data(), n_trees * sizeof(uint32_t), hipMemcpyHostToDevice, ctx->stream));
    LOCGPU_HIP(ctx, hipStreamSynchronize(ctx->stream));
    ctx->forest_n = (int)n_trees;
    ctx->forest_base = std::move(o.base);
    ctx->forest_leaves = std::move(o.leaves);
    ctx->forest_depth = std::move(o.depth);
    note_build(ctx, o, 1, 1);
    return LOCGPU_OK;
}

int locgpu_icp_set_target_cloud_device(locgpu_ctx* ctx, const locgpu_cloud* target) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    const char* who = "icp_set_target_cloud_device";
    if (!target || target->ctx != ctx) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": bad cloud");
    if (target->n == 0) return fail(ctx, LOCGPU_ERR_INVALID, std::string(who) + ": empty cloud or stride < 12");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    BuildOutcome o;
    const int brc = build_on_device(ctx, target->d, std::vector<size_t>{0}, std::vector<size_t>{target->n}, who, o);
    if (brc != LOCGPU_OK) return brc;
    if (o.first_degenerate >= 0) {
        const int rc = locgpu_icp_set_target_cloud(ctx, target);
        if (rc == LOCGPU_OK) note_build(ctx, o, 2, 2);
        return rc;
    }
    if (o.first_deep >= 0) return refuse_deep(ctx, who, o, false);
    const int rc = install_device_build(ctx, o);  // forest_n = 0: an ordinary target
    if (rc != LOCGPU_OK) return rc;
    note_build(ctx, o, 1, 2);
    return LOCGPU_OK;
}

int locgpu_icp_device_build_info(const locgpu_ctx* ctx, int64_t out[8]) {
    if (!ctx || !out) return LOCGPU_ERR_INVALID;
    const ForestBuildScratch* sc = ctx->fbuild;
    out[0] = sc ? sc->last_path : 0;
    out[1] = sc ? sc->first_degenerate : -1;
    out[2] = sc ? sc->levels : 0;
    out[3] = kFbTile;
    out[4] = kFbLaneLen;
    out[5] = kFbThreads;
    out[6] = sc ? sc->last_kind : 0;
    out[7] = ctx->tree_bounded ? 1 : 0;
    return LOCGPU_OK;
}

int locgpu_debug_tree_read(locgpu_ctx* ctx, uint64_t* slots, size_t cap, uint32_t* leaf_slots, size_t leaf_cap) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    { const int jrc = target_join(ctx); if (jrc != LOCGPU_OK) return jrc; }
    if (!ctx->d_tree) return fail(ctx, LOCGPU_ERR_NO_TARGET, "debug_tree_read: no ICP target");
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    for (hipStream_t st : ctx->slot_stream) LOCGPU_HIP(ctx, hipStreamSynchronize(st));
    const size_t ns = std::min(cap, ctx->tree_slots + 2);
    if (slots && ns) LOCGPU_HIP(ctx, hipMemcpy(slots, ctx->d_tree, ns * sizeof(uint64_t), hipMemcpyDeviceToHost));
    const size_t nl = ctx->forest_n == 0 ? std::min(leaf_cap, ctx->num_leaves) : 0;
    if (leaf_slots && nl) LOCGPU_HIP(ctx, hipMemcpy(leaf_slots, ctx->d_leaf_slots, nl * sizeof(uint32_t), hipMemcpyDeviceToHost));
    return LOCGPU_OK;
}

}  // extern "C"
