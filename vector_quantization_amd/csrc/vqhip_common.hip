// libvqhip — what every unit shares on the host (vqhip_host.h): the last error, the LDS attribute cache; and the host-only RCCL block.
#include "vqhip.h"

#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <mutex>

#include "vqhip_host.h"

static thread_local char g_err[256] = "";

int fail(int code, const char *what, const char *detail) {
    snprintf(g_err, sizeof(g_err), "%s%s%s", what, detail[0] ? ": " : "", detail);
    return code;
}

int ensure_dyn_lds(const void *kern, size_t bytes, LdsCache &set) {
    int dev = 0;
    VQ_HIP(hipGetDevice(&dev));
    const bool cached = dev >= 0 && dev < VQ_MAX_DEVICES;
    if (!cached || bytes > set[dev].load(std::memory_order_acquire)) {
        VQ_HIP(hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes));
        if (cached) {                                   // keep the maximum (another thread may have raised it meanwhile)
            size_t cur = set[dev].load(std::memory_order_relaxed);
            while (cur < bytes && !set[dev].compare_exchange_weak(cur, bytes, std::memory_order_release)) {}
        }
    }
    return VQHIP_OK;
}

extern "C" {

int vqhip_version(void) { return VQHIP_VERSION; }
const char *vqhip_last_error(void) { return g_err; }

// ---- the packed all-reduce on the caller's stream (RCCL resolved at run time; include/vqhip.h) -----------------------
// libvqhip never links librccl: a process that already holds one (PyTorch-ROCm's) must not get a second copy, and a
// caller without RCCL must still be able to load the library.  The handful of symbols are looked up once.
#include <dlfcn.h>
struct VqRcclId { char bytes[VQHIP_RCCL_ID_BYTES]; };      // ncclUniqueId (rccl.h: 128 opaque bytes), passed by value
namespace {
struct RcclApi {
    void *handle = nullptr;
    int (*get_unique_id)(void *) = nullptr;
    int (*comm_init_rank)(void **, int, VqRcclId, int) = nullptr;
    int (*comm_destroy)(void *) = nullptr;
    int (*all_reduce)(const void *, void *, size_t, int, int, void *, hipStream_t) = nullptr;
    const char *(*error_string)(int) = nullptr;
};
}  // namespace
static RcclApi g_rccl;
static std::mutex g_rccl_mu;
static const int kNcclFloat32 = 7, kNcclInt64 = 4, kNcclSum = 0, kNcclMin = 3;        // rccl.h: ncclFloat32 = 7, ncclInt64 = 4, ncclSum = 0, ncclMin = 3

static int rccl_fail(const char *what, int rc) {
    return fail(VQHIP_ERCCL, what, g_rccl.error_string ? g_rccl.error_string(rc) : "RCCL error");
}

int vqhip_rccl_load(const char *path) {
    std::lock_guard<std::mutex> lock(g_rccl_mu);
    if (g_rccl.handle) return VQHIP_OK;
    void *h = nullptr;
    if (path && path[0]) {
        h = dlopen(path, RTLD_NOW | RTLD_GLOBAL);
        if (!h) return fail(VQHIP_ERCCL, "vqhip_rccl_load: librccl.so not loadable", dlerror());
    } else {
        // without a path: ONLY the copy the process already has (RTLD_NOLOAD).  Falling back to the loader's search path could map
        // a second RCCL (say /opt/rocm's next to PyTorch's) into the process — two copies must never coexist; a caller whose
        // copy was loaded under another name passes its path
        const char *names[] = {"librccl.so", "librccl.so.1"};
        for (const char *n : names)
            if (!h) h = dlopen(n, RTLD_NOW | RTLD_NOLOAD);
        if (!h) return fail(VQHIP_ERCCL, "vqhip_rccl_load: no librccl.so is mapped into this process under that name; pass the path of the copy the application uses");
    }
    RcclApi api;
    api.handle = h;
    api.get_unique_id = (decltype(api.get_unique_id))dlsym(h, "ncclGetUniqueId");
    api.comm_init_rank = (decltype(api.comm_init_rank))dlsym(h, "ncclCommInitRank");
    api.comm_destroy = (decltype(api.comm_destroy))dlsym(h, "ncclCommDestroy");
    api.all_reduce = (decltype(api.all_reduce))dlsym(h, "ncclAllReduce");
    api.error_string = (decltype(api.error_string))dlsym(h, "ncclGetErrorString");
    if (!api.get_unique_id || !api.comm_init_rank || !api.comm_destroy || !api.all_reduce || !api.error_string)
        return fail(VQHIP_ERCCL, "vqhip_rccl_load: librccl.so lacks an nccl* symbol");
    g_rccl = api;
    return VQHIP_OK;
}

int vqhip_rccl_unique_id(void *id_host) {
    if (!id_host) return fail(VQHIP_EINVAL, "vqhip_rccl_unique_id: null buffer");
    if (!g_rccl.handle) return fail(VQHIP_ERCCL, "vqhip_rccl_unique_id: call vqhip_rccl_load first");
    static_assert(sizeof(VqRcclId) == 128, "ncclUniqueId is 128 bytes (rccl.h: NCCL_UNIQUE_ID_BYTES)");
    const int rc = g_rccl.get_unique_id(id_host);
    return rc == 0 ? VQHIP_OK : rccl_fail("ncclGetUniqueId", rc);
}

int vqhip_rccl_comm_init(void **comm, int nranks, const void *id_host, int rank) {
    if (!comm || !id_host || nranks < 1 || rank < 0 || rank >= nranks) return fail(VQHIP_EINVAL, "vqhip_rccl_comm_init: bad argument");
    if (!g_rccl.handle) return fail(VQHIP_ERCCL, "vqhip_rccl_comm_init: call vqhip_rccl_load first");
    VqRcclId id;
    memcpy(id.bytes, id_host, sizeof(id.bytes));
    *comm = nullptr;
    const int rc = g_rccl.comm_init_rank(comm, nranks, id, rank);
    return rc == 0 ? VQHIP_OK : rccl_fail("ncclCommInitRank", rc);
}

int vqhip_rccl_comm_destroy(void *comm) {
    if (!comm) return VQHIP_OK;
    if (!g_rccl.handle) return fail(VQHIP_ERCCL, "vqhip_rccl_comm_destroy: RCCL not loaded");
    const int rc = g_rccl.comm_destroy(comm);
    return rc == 0 ? VQHIP_OK : rccl_fail("ncclCommDestroy", rc);
}

int vqhip_allreduce_packed(float *buf, int64_t floats, void *comm, void *stream) {
    if (!buf || !comm || floats < 0) return fail(VQHIP_EINVAL, "vqhip_allreduce_packed: bad argument");
    if (!g_rccl.handle) return fail(VQHIP_ERCCL, "vqhip_allreduce_packed: RCCL not loaded");
    if (floats == 0) return VQHIP_OK;
    const int rc = g_rccl.all_reduce(buf, buf, (size_t)floats, kNcclFloat32, kNcclSum, comm, (hipStream_t)stream);
    return rc == 0 ? VQHIP_OK : rccl_fail("ncclAllReduce", rc);
}

int vqhip_allreduce_min_i64(int64_t *buf, int64_t n, void *comm, void *stream) {
    if (!buf || !comm || n < 0) return fail(VQHIP_EINVAL, "vqhip_allreduce_min_i64: bad argument");
    if (!g_rccl.handle) return fail(VQHIP_ERCCL, "vqhip_allreduce_min_i64: RCCL not loaded");
    if (n == 0) return VQHIP_OK;
    const int rc = g_rccl.all_reduce(buf, buf, (size_t)n, kNcclInt64, kNcclMin, comm, (hipStream_t)stream);
    return rc == 0 ? VQHIP_OK : rccl_fail("ncclAllReduce", rc);
}

}  // extern "C"
