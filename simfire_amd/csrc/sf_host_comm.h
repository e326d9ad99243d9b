// Host code of the result-block all-gather over RCCL (sf_comm_*, sf_allgather_status); the library is loaded on first use.
// Part of the single translation unit simfire_hip.hip (included there, behind sf_handle.h).
#pragma once

// ---- the one collective: RCCL through dlopen, so that a one-GPU host needs no librccl
namespace {
struct RcclApi {
    void *lib = nullptr;
    ncclResult_t (*GetUniqueId)(ncclUniqueId *) = nullptr;
    ncclResult_t (*CommInitRank)(ncclComm_t *, int, ncclUniqueId, int) = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
};
RcclApi g_rccl;
int rccl_load()
{
    if (g_rccl.lib) return SF_OK;
    // (SIMFIRE_RCCL_LIB: another library with the same five entry points - the tests' single-process stand-in, tests/fake_rccl.cpp,
    // which lets 8 handles on ONE GPU play the 8 ranks of a node; never set in production)
    const char *names[] = {getenv("SIMFIRE_RCCL_LIB"), "librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void *lib = nullptr;
    for (const char *n : names) if (n && *n && (lib = dlopen(n, RTLD_NOW | RTLD_LOCAL))) break;
    if (!lib) return fail(SF_ERCCL, "librccl.so could not be loaded: %s", dlerror());
    RcclApi a;
    a.lib = lib;
    a.GetUniqueId = reinterpret_cast<decltype(a.GetUniqueId)>(dlsym(lib, "ncclGetUniqueId"));
    a.CommInitRank = reinterpret_cast<decltype(a.CommInitRank)>(dlsym(lib, "ncclCommInitRank"));
    a.AllGather = reinterpret_cast<decltype(a.AllGather)>(dlsym(lib, "ncclAllGather"));
    a.CommDestroy = reinterpret_cast<decltype(a.CommDestroy)>(dlsym(lib, "ncclCommDestroy"));
    a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(dlsym(lib, "ncclGetErrorString"));
    if (!a.GetUniqueId || !a.CommInitRank || !a.AllGather || !a.CommDestroy || !a.GetErrorString) {
        dlclose(lib);
        return fail(SF_ERCCL, "librccl.so lacks one of ncclGetUniqueId / ncclCommInitRank / ncclAllGather / ncclCommDestroy / ncclGetErrorString");
    }
    g_rccl = a;
    return SF_OK;
}
#define RCCLCHK(x) do { ncclResult_t _r = (x); if (_r != ncclSuccess) return fail(SF_ERCCL, "%s failed: %s", #x, g_rccl.GetErrorString(_r)); } while (0)
}  // namespace

extern "C" int sf_comm_unique_id(void *id_out)
{
    if (!id_out) return fail(SF_EINVAL, "sf_comm_unique_id: null argument");
    static_assert(sizeof(ncclUniqueId) == 128, "the header promises 128 bytes");
    SF_TRY(rccl_load());
    ncclUniqueId id;
    RCCLCHK(g_rccl.GetUniqueId(&id));
    std::memcpy(id_out, &id, sizeof id);
    return SF_OK;
}

extern "C" int sf_comm_destroy(sf_sim *s) { return s ? comm_close(s) : fail(SF_EINVAL, "sf_comm_destroy: null handle"); }
static int comm_close(sf_sim *s)
{
    if (!s->comm) return SF_OK;
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    HIPCHK(hipStreamSynchronize(s->stream));
    ncclComm_t c = s->comm;
    s->comm = nullptr; s->comm_world = 0;
    RCCLCHK(g_rccl.CommDestroy(c));
    return SF_OK;
}

extern "C" int sf_comm_init(sf_sim *s, int32_t rank, int32_t world_size, const void *unique_id)
{
    if (!s || !unique_id) return fail(SF_EINVAL, "sf_comm_init: null argument");
    if (world_size < 1 || rank < 0 || rank >= world_size) return fail(SF_EINVAL, "sf_comm_init: rank %d of %d", rank, world_size);
    SF_TRY(rccl_load());
    SF_TRY(comm_close(s));
    HIPCHK(hipSetDevice(s->p.device)); LOOP_QUIESCE(s);
    ncclUniqueId id;
    std::memcpy(&id, unique_id, sizeof id);
    RCCLCHK(g_rccl.CommInitRank(&s->comm, world_size, id, rank));
    s->comm_world = world_size;
    return SF_OK;
}

extern "C" int sf_allgather_status(sf_sim *s, void *device_out)
{
    if (!s || !device_out) return fail(SF_EINVAL, "sf_allgather_status: null argument");
    if (!s->comm) return fail(SF_ESTATE, "sf_allgather_status: call sf_comm_init first");
    SF_TRY(status_query(s, "sf_allgather_status", nullptr));      // the block of this rank's shard (fresh already after a resident launch)
    // on the handle's stream: behind the steps in flight and the refresh, no host wait in between
    RCCLCHK(g_rccl.AllGather(s->status_block, device_out, (size_t)8 * s->g.E, ncclInt32, s->comm, s->stream));
    return finish_call(s, "sf_allgather_status", true, nullptr);
}
