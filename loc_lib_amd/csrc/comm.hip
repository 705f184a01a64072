// loc_lib_amd/csrc/comm.hip — the context's communicator: RCCL bound at run time, the collectives the library uses, locgpu_comm_*.
#include <cstring>
#include <string>

#include "context.hpp"

#include <dlfcn.h>
#include <sched.h>
#include <rccl/rccl.h>

using namespace locgpu;

// RCCL is bound at the first locgpu_comm_* call (dlopen), not at load time: a single-GPU process — the slam_demo front-end, the
// tests — never maps librccl and its dependencies (rocm_smi, roctx, rocprofiler-register). The entry points used:
namespace {
struct Rccl {
    ncclResult_t (*GetUniqueId)(ncclUniqueId*) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t*, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*AllReduce)(const void*, void*, size_t, ncclDataType_t, ncclRedOp_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*Broadcast)(const void*, void*, size_t, ncclDataType_t, int, ncclComm_t, hipStream_t) = nullptr;
    const char* (*GetErrorString)(ncclResult_t) = nullptr;
    bool ok = false;
    std::string err;
};
Rccl& rccl() {
    static Rccl r = [] {
        Rccl x;
        // LOCGPU_RCCL_LIB names another library with the same six entry points: a site's own RCCL build, or the loopback double the
        // tests use to run two ranks as two threads on one GPU (tests/cpp/loopback_rccl.hip).
        const char* named = getenv("LOCGPU_RCCL_LIB");
        void* h = (named && *named) ? dlopen(named, RTLD_NOW | RTLD_LOCAL)
                                    : dlopen("librccl.so.1", RTLD_NOW | RTLD_GLOBAL);  // a copy already mapped by the host process (e.g. PyTorch's) is reused
        if (!h && !(named && *named)) h = dlopen("librccl.so", RTLD_NOW | RTLD_GLOBAL);
        if (!h) { x.err = std::string("cannot load librccl: ") + dlerror(); return x; }
        x.GetUniqueId = (decltype(x.GetUniqueId))dlsym(h, "ncclGetUniqueId");
        x.CommInitRank = (decltype(x.CommInitRank))dlsym(h, "ncclCommInitRank");
        x.CommDestroy = (decltype(x.CommDestroy))dlsym(h, "ncclCommDestroy");
        x.AllReduce = (decltype(x.AllReduce))dlsym(h, "ncclAllReduce");
        x.Broadcast = (decltype(x.Broadcast))dlsym(h, "ncclBroadcast");
        x.GetErrorString = (decltype(x.GetErrorString))dlsym(h, "ncclGetErrorString");
        x.ok = x.GetUniqueId && x.CommInitRank && x.CommDestroy && x.AllReduce && x.Broadcast && x.GetErrorString;
        if (!x.ok) x.err = "librccl lacks an expected entry point";
        return x;
    }();
    return r;
}
}  // namespace

// Sum of `count` doubles over the context's communicator, in place, on stream `s`: the exchange step of sharded batches and pools.
bool locgpu::comm_all_reduce_f64(locgpu_ctx* ctx, double* buf, size_t count, hipStream_t s) {
    const ncclResult_t nr = rccl().AllReduce(buf, buf, count, ncclDouble, ncclSum, (ncclComm_t)ctx->comm, s);
    if (nr == ncclSuccess) return true;
    fail(ctx, LOCGPU_ERR_NO_DEVICE, std::string("ncclAllReduce: ") + rccl().GetErrorString(nr));
    return false;
}

bool locgpu::comm_broadcast(locgpu_ctx* ctx, void* buf, size_t bytes, int root, hipStream_t s) {
    return rccl().Broadcast(buf, buf, bytes, ncclChar, root, (ncclComm_t)ctx->comm, s) == ncclSuccess;
}
bool locgpu::comm_all_reduce_min_int(locgpu_ctx* ctx, int* buf, hipStream_t s) {
    return rccl().AllReduce(buf, buf, 1, ncclInt, ncclMin, (ncclComm_t)ctx->comm, s) == ncclSuccess;
}
void locgpu::comm_destroy(locgpu_ctx* ctx) {
    if (ctx->comm) { (void)rccl().CommDestroy((ncclComm_t)ctx->comm); ctx->comm = nullptr; }
}

extern "C" {

int locgpu_comm_unique_id(void* id_out) {
    if (!id_out) return LOCGPU_ERR_INVALID;
    static_assert(LOCGPU_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "locgpu.h and rccl.h disagree on the id size");
    ncclUniqueId id;
    if (!rccl().ok || rccl().GetUniqueId(&id) != ncclSuccess) return LOCGPU_ERR_NO_DEVICE;
    std::memcpy(id_out, &id, sizeof(id));
    return LOCGPU_OK;
}

int locgpu_comm_init(locgpu_ctx* ctx, int rank, int world, const void* id) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (!id || world < 1 || rank < 0 || rank >= world) return fail(ctx, LOCGPU_ERR_INVALID, "comm_init: bad arguments");
    if (ctx->comm) return fail(ctx, LOCGPU_ERR_INVALID, "comm_init: this context already has a communicator");
    if (!rccl().ok) return fail(ctx, LOCGPU_ERR_NO_DEVICE, "comm_init: " + rccl().err);
    LOCGPU_HIP(ctx, hipSetDevice(ctx->device));
    ncclUniqueId uid;
    std::memcpy(&uid, id, sizeof(uid));
    ncclComm_t comm = nullptr;
    // RCCL may narrow the calling thread's CPU affinity while it initialises, and threads created afterwards (the uploader's
    // packers, the tree-build pool) inherit what it leaves behind: put the caller's mask back.
    cpu_set_t saved_affinity;
    const bool have_affinity = sched_getaffinity(0, sizeof(saved_affinity), &saved_affinity) == 0;
    const ncclResult_t nr = rccl().CommInitRank(&comm, world, uid, rank);
    if (have_affinity) (void)sched_setaffinity(0, sizeof(saved_affinity), &saved_affinity);
    if (nr != ncclSuccess) return fail(ctx, LOCGPU_ERR_NO_DEVICE, std::string("ncclCommInitRank: ") + rccl().GetErrorString(nr));
    ctx->comm = comm;
    ctx->comm_rank = rank;
    ctx->comm_world = world;
    return LOCGPU_OK;
}

int locgpu_comm_info(const locgpu_ctx* ctx, int* rank, int* world) {
    if (!ctx) return LOCGPU_ERR_INVALID;
    if (rank) *rank = ctx->comm_rank;
    if (world) *world = ctx->comm ? ctx->comm_world : 1;
    return LOCGPU_OK;
}

}  // extern "C"
