// C-ABI, image stage: conversion of a rendered XYZ histogram into the image modes, the resolution filter, and the cost
// functions of the focus search.
#include <cmath>
#include <string>

#include "ot_focus.hpp"
#include "ot_host.hpp"
#include "ot_image.hpp"

// ---- image conversion ----------------------------------------------------------------------------------------
extern "C" int ot_image_convert(const double* hist, int32_t Nx, int32_t Ny, int32_t fact, int32_t mode, double apx,
                                double K, double L_th, double chroma_scale, double* out, double* workspace, void* stream) {
    if (!hist || !out || !workspace || Nx < 1 || Ny < 1 || fact < 1 || Nx % fact || Ny % fact)
        return fail(OT_ERR_INVALID, "ot_image_convert: bad argument");
    const int flags = mode & (OT_IMG_FLAG_NO_NORMALIZE | OT_IMG_FLAG_NO_CLIP);
    mode &= ~(OT_IMG_FLAG_NO_NORMALIZE | OT_IMG_FLAG_NO_CLIP);
    if (mode < OT_IMG_IRRADIANCE || mode > OT_IMG_SATURATION) return fail(OT_ERR_INVALID, "ot_image_convert: unknown mode");
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t npx = (int64_t)(Nx / fact) * (Ny / fact);
    double* img = workspace;            // (ny, nx, 4) down-binned working copy
    double* red = workspace + npx * 4;  // OT_RED_N reduction slots
    dim3 grid = grid_for(npx), block(256);
    hipLaunchKernelGGL(img_downbin_kernel, grid, block, 0, st, hist, Nx, Ny, fact, img);
    const double inf = INFINITY;
    double init[OT_RED_N] = {-inf, -inf, 0.0, -inf, 0.0, inf, -inf, 0.0};
    HIP_TRY(hipMemcpyAsync(red, init, sizeof(init), hipMemcpyHostToDevice, st));
    if (mode != OT_IMG_IRRADIANCE && mode != OT_IMG_ILLUMINANCE)
        hipLaunchKernelGGL(img_reduce1_kernel, grid, block, 0, st, img, npx, red);
    if (mode == OT_IMG_SRGB_ABSOLUTE || mode == OT_IMG_SRGB_PERCEPTUAL) {
        double h[OT_RED_N];
        HIP_TRY(hipMemcpyAsync(h, red, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const bool any_inv = h[OT_RED_ANY_INV] != 0.0;
        const bool cs_given = !std::isnan(chroma_scale);
        int intent = 0;  // srgb.py:318-319: nothing out of gamut and no fixed chroma scale -> plain conversion
        int use_ones = 0;
        double cs = 1.0;
        if (any_inv || cs_given) {
            if (mode == OT_IMG_SRGB_ABSOLUTE) {
                intent = 1;
            } else {
                intent = 2;
                hipLaunchKernelGGL(img_reduce2_kernel, grid, block, 0, st, img, npx, L_th, red);
                HIP_TRY(hipMemcpyAsync(h, red, sizeof(h), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                use_ones = h[OT_RED_ANY_GAMUT] == 0.0;
                double crmin = (use_ones || !std::isfinite(h[OT_RED_CRMIN])) ? 1.0 : h[OT_RED_CRMIN];
                double f = std::sqrt(crmin);
                f = f < 0.32 ? 0.32 : (f > 1.0 ? 1.0 : f);  // srgb.py:252
                cs = cs_given ? chroma_scale : f;
            }
        }
        hipLaunchKernelGGL(img_correct_kernel, grid, block, 0, st, img, npx, intent, cs, use_ones, red);
    }
    hipLaunchKernelGGL(img_final_kernel, grid, block, 0, st, img, npx, mode | flags, apx, K, red, out);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_image_convolve(const double* in, int32_t Nx, int32_t Ny, const double* psf, int32_t ps, double* out,
                                 void* stream) {
    if (!in || !psf || !out || Nx < 1 || Ny < 1 || ps < 0 || in == out) return fail(OT_ERR_INVALID, "ot_image_convolve: bad argument");
    const size_t lds = sizeof(double) * (size_t)(2 * ps + 1) * (2 * ps + 1);
    if (lds > 150 * 1024) return fail(OT_ERR_UNSUPPORTED, "ot_image_convolve: kernel larger than 137 x 137 taps");
    if (int rc = require_device()) return rc;
    if (lds > 64 * 1024)
        HIP_TRY(hipFuncSetAttribute((const void*)img_convolve_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    hipLaunchKernelGGL(img_convolve_kernel, grid_for((int64_t)Nx * Ny), dim3(256), lds, (hipStream_t)stream, in, Nx, Ny, psf, ps, out);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

// ---- focus search -------------------------------------------------------------------------------------------
static unsigned stream_blocks(int64_t n, int threads, int per_cu) {
    int64_t blocks = (n + threads - 1) / threads;
    const int64_t cap = (int64_t)cu_count() * per_cu;
    if (blocks > cap) blocks = cap;
    return (unsigned)(blocks < 1 ? 1 : blocks);
}

extern "C" int ot_focus_prepare(const ot_rays* rays, int64_t first, int64_t count, double z, double* pasb, float* w,
                                int64_t* n_use, void* stream) {
    if (!rays || !rays->p || !rays->w || first < 0 || count < 0 || first + count > rays->N || rays->nt < 2 || !n_use ||
        (count && (!pasb || !w)))
        return fail(OT_ERR_INVALID, "ot_focus_prepare: bad argument");
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(n_use, 0, sizeof(int64_t), st));
    if (count == 0) return OT_OK;
    hipLaunchKernelGGL(focus_prepare_kernel, grid_for(count), dim3(256), 0, st, *rays, first, count, z, pasb, w,
                       (unsigned long long*)n_use);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_focus_cost(int64_t count, const double* pasb, const float* w, int32_t mode, const double* z, int32_t nz,
                             int32_t n_px, double* workspace, double* cost, void* stream) {
    if (count < 1 || !pasb || !w || !z || nz < 1 || !workspace || !cost || mode < OT_FOCUS_RMS ||
        mode > OT_FOCUS_CENTER_SHARPNESS || (mode != OT_FOCUS_RMS && n_px < 2))
        return fail(OT_ERR_INVALID, "ot_focus_cost: bad argument");
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    double* img = workspace + OT_FOCUS_WS;
    const int64_t np2 = (int64_t)n_px * n_px;
    const unsigned gs = stream_blocks(count, 256, 8), gb = stream_blocks(count, 1024, 1);
    for (int i = 0; i < nz; i++) {
        hipLaunchKernelGGL(focus_init_kernel, dim3(1), dim3(64), 0, st, workspace);
        hipLaunchKernelGGL(focus_stats_kernel, dim3(gs), dim3(256), 0, st, count, pasb, w, z[i], workspace);
        if (mode == OT_FOCUS_RMS) {
            hipLaunchKernelGGL(focus_var_kernel, dim3(gs), dim3(256), 0, st, count, pasb, w, z[i], workspace);
        } else {
            HIP_TRY(hipMemsetAsync(img, 0, sizeof(double) * np2, st));
            hipLaunchKernelGGL(focus_bin_kernel, dim3(gb), dim3(1024), 0, st, count, pasb, w, z[i], workspace, n_px, img);
            hipLaunchKernelGGL(focus_image1_kernel, grid_for(np2), dim3(256), 0, st, img, n_px, mode, workspace);
            if (mode == OT_FOCUS_IRR_VAR)
                hipLaunchKernelGGL(focus_image2_kernel, grid_for(np2), dim3(256), 0, st, img, n_px, workspace);
        }
        hipLaunchKernelGGL(focus_finalize_kernel, dim3(1), dim3(64), 0, st, mode, n_px, workspace, cost + i);
    }
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_focus_moments(int64_t count, const double* pasb, const float* w, double b0, double b1, double* sums,
                                void* stream) {
    if (count < 1 || !pasb || !w || !sums || !(b1 > b0)) return fail(OT_ERR_INVALID, "ot_focus_moments: bad argument");
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(sums, 0, sizeof(double) * 16, st));
    const unsigned gs = stream_blocks(count, 256, 8);
    hipLaunchKernelGGL(focus_moments1_kernel, dim3(gs), dim3(256), 0, st, count, pasb, w, sums);
    hipLaunchKernelGGL(focus_moments2_kernel, dim3(gs), dim3(256), 0, st, count, pasb, w, b0, b1, sums);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
