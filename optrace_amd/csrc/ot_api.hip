// C-ABI of the MI355X tracing core (include/optrace_amd.h), core unit: version, errors, device check, the scratch pool and
// the arithmetic self-test.  The stages live in ot_*_api.hip, one translation unit each; what they share is ot_host.hpp.
// Build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -munsafe-fp-atomics -fPIC -shared (see Makefile).
#include <cstdlib>
#include <cstring>
#include <string>

#include "ot_host.hpp"
#include "ot_selftest.hpp"

// ---------------------------------------------------------------------------------------------------------
// errors: the one thread-local message of the library, whichever unit reports (ot_host.hpp::fail)
// ---------------------------------------------------------------------------------------------------------
static thread_local std::string g_err;

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

extern "C" int ot_abi_version(void) { return OT_ABI_VERSION; }
extern "C" const char* ot_last_error(void) { return g_err.c_str(); }
extern "C" int ot_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) return OT_ERR_NO_DEVICE;
    return n;
}

int require_device() {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0)
        return fail(OT_ERR_NO_DEVICE, "no HIP device available; this library has no CPU fallback");
    return OT_OK;
}

// Scratch of the binning paths (hit records, slabs: up to ~25 B per ray and image): ot_scratch.hpp.  One pool per process,
// blocks keyed by (device, stream, purpose), LEASED for the launches of a call (an automatic image keeps its lease from begin
// to finish / cancel), kept between calls, capped (OT_SCRATCH_CAP_GB in the environment or ot_scratch_set_cap; 64 GB of the
// 288), idle blocks freed least recently used first.  torch's allocator, which owns the ray storage, cannot see this memory:
// ot_scratch_trim() hands the idle part back on request.
static void* ws_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipMalloc(&p, bytes) != hipSuccess || !p) {
        (void)hipGetLastError();
        return nullptr;
    }
    return p;
}
static void ws_release(void* p) { (void)hipFree(p); }  // (waits for the work that may still use p)
static void ws_sync() { (void)hipDeviceSynchronize(); }
static ot_scratch::Pool& scratch_pool() {
    static ot_scratch::Pool pool({ws_alloc, ws_release, ws_sync}, [] {
        const char* v = std::getenv("OT_SCRATCH_CAP_GB");
        const double gb = v ? std::atof(v) : 64.0;
        return (size_t)((gb > 0.0 ? gb : 64.0) * 1e9);
    }());
    return pool;
}

ot_scratch::Lease workspace(int purpose, size_t bytes, hipStream_t st) {
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess) return {};
    return ot_scratch::Lease(scratch_pool(), dev, purpose, (void*)st, bytes);
}

extern "C" int ot_scratch_trim(void) {
    if (int rc = require_device()) return rc;
    scratch_pool().trim();
    return OT_OK;
}

extern "C" int ot_scratch_set_cap(int64_t bytes) {
    if (bytes < 0) return fail(OT_ERR_INVALID, "ot_scratch_set_cap: negative cap");
    scratch_pool().set_cap((size_t)bytes);
    return OT_OK;
}

extern "C" int ot_scratch_stats(int64_t* kept_bytes, int32_t* blocks, int32_t* leased) {
    size_t kept = 0;
    int nb = 0, busy = 0;
    scratch_pool().stats(&kept, &nb, &busy);
    if (kept_bytes) *kept_bytes = (int64_t)kept;
    if (blocks) *blocks = nb;
    if (leased) *leased = busy;
    return OT_OK;
}

int cu_count() {
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) == hipSuccess && hipGetDeviceProperties(&prop, dev) == hipSuccess && prop.multiProcessorCount > 0)
        return prop.multiProcessorCount;
    return 256;
}

// ---------------------------------------------------------------------------------------------------------
// diagnostics: exactness of the division / square-root cores (ot_selftest.hpp)
// ---------------------------------------------------------------------------------------------------------
extern "C" int ot_selftest_arith(int32_t op, int32_t operand_class, int64_t n, uint64_t seed, int64_t* mismatches,
                                 double* first_bad4, void* stream) {
    if (!mismatches || !first_bad4 || n < 0) return fail(OT_ERR_INVALID, "ot_selftest_arith: bad argument");
    // (the accuracy case and its operand class belong to each other)
    if (op < OT_ST_DIV || op > OT_ST_FAST_RCP || operand_class < OT_CLS_WIDE || operand_class > OT_CLS_RECIPROCAL ||
        (op == OT_ST_FAST_RCP) != (operand_class == OT_CLS_RECIPROCAL))
        return fail(OT_ERR_INVALID, "ot_selftest_arith: unknown operation or operand class");
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    char* scratch = nullptr;
    HIP_TRY(hipMalloc((void**)&scratch, 64));
    hipError_t e = hipMemsetAsync(scratch, 0, 64, st);
    unsigned long long host[2] = {0, 0};
    double bad[4] = {0, 0, 0, 0};
    if (e == hipSuccess && n > 0 && op == OT_ST_FAST_RCP) {
        hipLaunchKernelGGL(selftest_rcp_kernel, dim3((unsigned)(cu_count() * 8)), dim3(256), 0, st, n, seed,
                           (unsigned long long*)scratch, (double*)(scratch + 16));
        e = hipGetLastError();
    } else if (e == hipSuccess && n > 0) {
        hipLaunchKernelGGL(selftest_arith_kernel, dim3((unsigned)(cu_count() * 8)), dim3(256), 0, st, (int)op,
                           (int)operand_class, n, seed, (unsigned long long*)scratch, (double*)(scratch + 16));
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(host, scratch, 16, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipMemcpyAsync(bad, scratch + 16, 32, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(scratch);
    HIP_TRY(e);
    *mismatches = (int64_t)host[0];
    std::memcpy(first_bad4, bad, sizeof(bad));
    return OT_OK;
}

extern "C" int ot_selftest_eval(int32_t op, int64_t n, const double* a, const double* b, const double* c, double* core_out,
                                double* ieee_out, void* stream) {
    if (n < 0 || (n && (!a || !core_out || !ieee_out))) return fail(OT_ERR_INVALID, "ot_selftest_eval: bad argument");
    if (op < OT_ST_DIV || op > OT_ST_DIV_SHARED) return fail(OT_ERR_INVALID, "ot_selftest_eval: unknown operation");
    if (int rc = require_device()) return rc;
    if (n == 0) return OT_OK;
    hipLaunchKernelGGL(selftest_eval_kernel, grid_for(n), dim3(256), 0, (hipStream_t)stream, (int)op, n, a, b, c, core_out,
                       ieee_out);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
