// C-ABI, leaf stage: the surface and medium functions of ot_device.hpp one by one (hit search, normals, mask, sag, HURB
// properties, refractive index), for tests and for the Python classes that evaluate a single surface.
#include "ot_device.hpp"
#include "ot_host.hpp"

// ---- leaf kernels (one lane per element) -------------------------------------------------------------------
__global__ __launch_bounds__(256) void find_hit_kernel(SurfDev sf, int64_t n, const double* __restrict__ p,
                                                       const double* __restrict__ s, double* __restrict__ ph_out,
                                                       uint8_t* __restrict__ hit_out, uint8_t* __restrict__ ill_out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    V3 pp = {p[i], p[i + n], p[i + 2 * n]}, ss = {s[i], s[i + n], s[i + 2 * n]}, ph;
    bool hit, ill;
    bool ok = find_hit(sf, pp, ss, ph, hit, ill);
    ph_out[i] = ph.x;
    ph_out[i + n] = ph.y;
    ph_out[i + 2 * n] = ph.z;
    hit_out[i] = hit;
    ill_out[i] = (uint8_t)((ill ? 1 : 0) | (ok ? 0 : 2));
}

__global__ __launch_bounds__(256) void normals_kernel(SurfDev sf, int64_t n, const double* __restrict__ x,
                                                      const double* __restrict__ y, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    V3 nn = surf_normal(sf, x[i], y[i]);
    out[i] = nn.x;
    out[i + n] = nn.y;
    out[i + 2 * n] = nn.z;
}

__global__ __launch_bounds__(256) void mask_kernel(SurfDev sf, int64_t n, const double* __restrict__ x,
                                                   const double* __restrict__ y, uint8_t* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = surf_mask(sf, x[i], y[i]);
}

__global__ __launch_bounds__(256) void values_kernel(SurfDev sf, int64_t n, const double* __restrict__ x,
                                                     const double* __restrict__ y, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = surf_values(sf, x[i], y[i]);
}

__global__ __launch_bounds__(256) void hurb_props_kernel(SurfDev sf, int64_t n, const double* __restrict__ x,
                                                         const double* __restrict__ y, double* __restrict__ a_,
                                                         double* __restrict__ b_, double* __restrict__ b,
                                                         uint8_t* __restrict__ inside) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double a, bb;
    V3 bv;
    bool in;
    hurb_props(sf, x[i], y[i], a, bb, bv, in);
    a_[i] = a;
    b_[i] = bb;
    b[i] = bv.x;
    b[i + n] = bv.y;
    b[i + 2 * n] = bv.z;
    inside[i] = in;
}

__global__ __launch_bounds__(256) void refraction_index_kernel(ot_medium md, const double* __restrict__ pool, int64_t n,
                                                               const float* __restrict__ wl, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    out[i] = medium_n(md, pool, wl[i]);
}

// ---- leaf entry points -------------------------------------------------------------------------------------
extern "C" int ot_surface_find_hit(const ot_surface* surf, int64_t n, const double* p, const double* s, double* p_hit,
                                   uint8_t* is_hit, uint8_t* ill, void* stream) {
    if (!surf || n < 0 || (n && (!p || !s || !p_hit || !is_hit || !ill))) return fail(OT_ERR_INVALID, "ot_surface_find_hit: bad argument");
    if (int rc = require_device()) return rc;
    LeafSurface ls;
    if (int rc = ls.init(surf, (hipStream_t)stream)) return rc;
    const SurfDev& d = ls.d;
    if (n == 0) return OT_OK;
    hipLaunchKernelGGL(find_hit_kernel, grid_for(n), dim3(256), 0, (hipStream_t)stream, d, n, p, s, p_hit, is_hit, ill);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_surface_normals(const ot_surface* surf, int64_t n, const double* x, const double* y, double* normals,
                                  void* stream) {
    if (!surf || n < 0 || (n && (!x || !y || !normals))) return fail(OT_ERR_INVALID, "ot_surface_normals: bad argument");
    if (int rc = require_device()) return rc;
    LeafSurface ls;
    if (int rc = ls.init(surf, (hipStream_t)stream)) return rc;
    const SurfDev& d = ls.d;
    if (n == 0) return OT_OK;
    hipLaunchKernelGGL(normals_kernel, grid_for(n), dim3(256), 0, (hipStream_t)stream, d, n, x, y, normals);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_surface_mask(const ot_surface* surf, int64_t n, const double* x, const double* y, uint8_t* mask,
                               void* stream) {
    if (!surf || n < 0 || (n && (!x || !y || !mask))) return fail(OT_ERR_INVALID, "ot_surface_mask: bad argument");
    if (int rc = require_device()) return rc;
    LeafSurface ls;
    if (int rc = ls.init(surf, (hipStream_t)stream)) return rc;
    const SurfDev& d = ls.d;
    if (n == 0) return OT_OK;
    hipLaunchKernelGGL(mask_kernel, grid_for(n), dim3(256), 0, (hipStream_t)stream, d, n, x, y, mask);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_surface_values(const ot_surface* surf, int64_t n, const double* x, const double* y, double* z,
                                 void* stream) {
    if (!surf || n < 0 || (n && (!x || !y || !z))) return fail(OT_ERR_INVALID, "ot_surface_values: bad argument");
    if (int rc = require_device()) return rc;
    LeafSurface ls;
    if (int rc = ls.init(surf, (hipStream_t)stream)) return rc;
    const SurfDev& d = ls.d;
    if (n == 0) return OT_OK;
    hipLaunchKernelGGL(values_kernel, grid_for(n), dim3(256), 0, (hipStream_t)stream, d, n, x, y, z);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_surface_hurb_props(const ot_surface* surf, int64_t n, const double* x, const double* y, double* a_,
                                     double* b_, double* b, uint8_t* inside, void* stream) {
    if (!surf || n < 0 || (n && (!x || !y || !a_ || !b_ || !b || !inside)))
        return fail(OT_ERR_INVALID, "ot_surface_hurb_props: bad argument");
    if (surf->kind != OT_SURF_RING && surf->kind != OT_SURF_SLIT)
        return fail(OT_ERR_UNSUPPORTED, "hurb_props is defined for ring and slit surfaces only");
    if (int rc = require_device()) return rc;
    LeafSurface ls;
    if (int rc = ls.init(surf, (hipStream_t)stream)) return rc;
    const SurfDev& d = ls.d;
    if (n == 0) return OT_OK;
    hipLaunchKernelGGL(hurb_props_kernel, grid_for(n), dim3(256), 0, (hipStream_t)stream, d, n, x, y, a_, b_, b, inside);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_refraction_index(const ot_medium* medium, const double* table_pool, int64_t table_pool_len, int64_t n,
                                   const float* wl, double* out, void* stream) {
    if (!medium || n < 0 || (n && (!wl || !out))) return fail(OT_ERR_INVALID, "ot_refraction_index: bad argument");
    if ((medium->model == OT_N_DATA || medium->model == OT_N_LINES) &&
        (!table_pool || medium->tab_off < 0 || medium->tab_off + 2 * (int64_t)medium->tab_len > table_pool_len))
        return fail(OT_ERR_INVALID, "ot_refraction_index: table outside the pool");
    if (int rc = require_device()) return rc;
    if (n == 0) return OT_OK;
    hipLaunchKernelGGL(refraction_index_kernel, grid_for(n), dim3(256), 0, (hipStream_t)stream, *medium, table_pool, n, wl, out);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
