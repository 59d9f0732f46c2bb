// C-ABI, image stage: conversion of a rendered XYZ histogram into the image modes, the colour conversions on arrays of the
// caller, the resolution filter, and the cost functions of the focus search.
#include <cmath>
#include <string>

#include "ot_focus.hpp"
#include "ot_host.hpp"
#include "ot_image.hpp"
#include "ot_color.hpp"

// ---- image conversion ----------------------------------------------------------------------------------------
// start values of the reduction slots (OT_RED_*, and OT_CRED_* behind them for n = OT_CRED_N)
static int red_init(double* red, int n, hipStream_t st) {
    const double inf = INFINITY;
    const double init[OT_CRED_N] = {-inf, -inf, 0.0, -inf, 0.0, inf, -inf, 0.0, 0.0, inf, -inf, 0.0, 0.0, 0.0, 0.0, 0.0};
    HIP_TRY(hipMemcpyAsync(red, init, sizeof(double) * n, hipMemcpyHostToDevice, st));
    return OT_OK;
}

// The decisions of xyz_to_srgb_linear srgb.py:305-349 on the quantities of pass 1 (already queued), and pass 3 src -> dst (which may be
// the same array) for pixels of stride S.  requested: 0 Ignore, 1 Absolute, 2 Perceptual.  Synchronises the stream unless the
// intent is Ignore: what pass 1 (and, for the Perceptual intent, pass 2) found picks the next launch.
template <int S>
static int intent_pass(const double* src, double* dst, int64_t npx, int requested, double L_th, double chroma_scale, double* red,
                       hipStream_t st) {
    dim3 grid = grid_for(npx), block(256);
    int intent = 0;  // srgb.py:318-319: nothing out of gamut and no fixed chroma scale -> plain conversion
    int use_ones = 0;
    double cs = 1.0;
    if (requested) {
        double h[OT_RED_N];
        HIP_TRY(hipMemcpyAsync(h, red, sizeof(h), hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        const bool any_inv = h[OT_RED_ANY_INV] != 0.0;
        const bool cs_given = !std::isnan(chroma_scale);
        if (any_inv || cs_given) {
            if (requested == 1) {
                intent = 1;
            } else {
                intent = 2;
                hipLaunchKernelGGL(img_reduce2_kernel<S>, grid, block, 0, st, src, npx, L_th, red);
                HIP_TRY(hipMemcpyAsync(h, red, sizeof(h), hipMemcpyDeviceToHost, st));
                HIP_TRY(hipStreamSynchronize(st));
                use_ones = h[OT_RED_ANY_GAMUT] == 0.0;
                double crmin = (use_ones || !std::isfinite(h[OT_RED_CRMIN])) ? 1.0 : h[OT_RED_CRMIN];
                double f = std::sqrt(crmin);
                f = f < 0.32 ? 0.32 : (f > 1.0 ? 1.0 : f);  // srgb.py:252
                cs = cs_given ? chroma_scale : f;
            }
        }
    }
    hipLaunchKernelGGL(img_correct_kernel<S>, grid, block, 0, st, src, dst, npx, intent, cs, use_ones, red);
    return OT_OK;
}

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
    if (int rc = red_init(red, OT_RED_N, st)) return rc;
    if (mode != OT_IMG_IRRADIANCE && mode != OT_IMG_ILLUMINANCE)
        hipLaunchKernelGGL(img_reduce1_kernel<4>, grid, block, 0, st, img, npx, red);
    if (mode == OT_IMG_SRGB_ABSOLUTE || mode == OT_IMG_SRGB_PERCEPTUAL)
        if (int rc = intent_pass<4>(img, img, npx, mode == OT_IMG_SRGB_ABSOLUTE ? 1 : 2, L_th, chroma_scale, red, st)) return rc;
    hipLaunchKernelGGL(img_final_kernel, grid, block, 0, st, img, npx, mode | flags, apx, K, red, out);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

// ---- colour conversions on arrays of the caller ------------------------------------------------------------------------
// xyz_to_srgb_linear / xyz_to_srgb (gamma) of `in` into `out` (which may be `in`): passes 1 to 3 and the last one
static int srgb_chain(const double* in, double* out, int64_t npx, int requested, bool normalize, bool clip, bool gamma, double L_th,
                      double chroma_scale, double* red, hipStream_t st) {
    dim3 grid = grid_for(npx), block(256);
    if (int rc = red_init(red, OT_CRED_N, st)) return rc;
    hipLaunchKernelGGL(img_reduce1_kernel<3>, grid, block, 0, st, in, npx, red);
    if (int rc = intent_pass<3>(in, out, npx, requested, L_th, chroma_scale, red, st)) return rc;
    hipLaunchKernelGGL(col_final_kernel, grid, block, 0, st, out, npx, (int)normalize, (int)clip, (int)gamma, 0, red, out);
    return OT_OK;
}

extern "C" int ot_color_convert(const double* in, int64_t npx, int32_t op, double L_th, double chroma_scale, double* out,
                                double* result, void* stream) {
    const int flags = op & ~0xff;
    op &= 0xff;
    const int requested = (flags & OT_COL_INTENT_PERCEPTUAL) ? 2 : ((flags & OT_COL_INTENT_ABSOLUTE) ? 1 : 0);
    const bool normalize = !(flags & OT_IMG_FLAG_NO_NORMALIZE), clip = !(flags & OT_IMG_FLAG_NO_CLIP);
    if (!in || npx < 1 || op < OT_COL_XYZ_TO_XYY || op > OT_COL_SPECTRAL_COLORMAP || (!out && op != OT_COL_CHROMA_SCALE) ||
        (flags & ~(OT_IMG_FLAG_NO_NORMALIZE | OT_IMG_FLAG_NO_CLIP | OT_COL_INTENT_ABSOLUTE | OT_COL_INTENT_PERCEPTUAL)) ||
        ((op == OT_COL_CHROMA_SCALE || op == OT_COL_LOG_SRGB) && !result) || (in == out && op != OT_COL_XYZ_TO_SRGB_LINEAR && op != OT_COL_XYZ_TO_SRGB))
        return fail(OT_ERR_INVALID, "ot_color_convert: bad argument");
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    dim3 grid = grid_for(npx), block(256);
    // scratch: the reduction slots; for the colour map the observer table, the colours of the wavelengths and their two sRGB rows
    Carver carve{0};
    const size_t o_red = carve(sizeof(double) * OT_CRED_N);
    size_t o_obs = 0, o_xyz = 0;
    if (op == OT_COL_SPECTRAL_COLORMAP) {
        o_obs = carve(sizeof(ot_observer_xyz));
        o_xyz = carve(sizeof(double) * 9 * (size_t)npx);
    }
    const ot_scratch::Lease lease = workspace(OT_WS_COLOR, carve.off, st);
    if (!lease) return fail(OT_ERR_HIP, "ot_color_convert: out of device memory");
    double* red = (double*)(lease.p() + o_red);
    double h[OT_CRED_N];
    switch (op) {
        case OT_COL_XYZ_TO_LUV:
            if (normalize) {
                if (int rc = red_init(red, OT_CRED_N, st)) return rc;
                hipLaunchKernelGGL(col_ymax_kernel, grid, block, 0, st, in, npx, 0, red);
            }
            hipLaunchKernelGGL(col_map_kernel, grid, block, 0, st, in, npx, op, (int)normalize, red, out);
            break;
        case OT_COL_XYZ_TO_SRGB_LINEAR:
        case OT_COL_XYZ_TO_SRGB:
            if (int rc = srgb_chain(in, out, npx, requested, normalize, clip && op == OT_COL_XYZ_TO_SRGB, op == OT_COL_XYZ_TO_SRGB, L_th,
                                    chroma_scale, red, st))
                return rc;
            break;
        case OT_COL_OUTSIDE_GAMUT:
            if (int rc = red_init(red, OT_CRED_N, st)) return rc;
            hipLaunchKernelGGL(img_reduce1_kernel<3>, grid, block, 0, st, in, npx, red);
            hipLaunchKernelGGL(col_final_kernel, grid, block, 0, st, in, npx, 1, 0, 0, 1, red, out);
            break;
        case OT_COL_CHROMA_SCALE: {
            if (int rc = red_init(red, OT_CRED_N, st)) return rc;
            hipLaunchKernelGGL(col_chroma_kernel, grid, block, 0, st, in, npx, 0, L_th, 0, red, out);
            hipLaunchKernelGGL(col_chroma_kernel, grid, block, 0, st, in, npx, 1, L_th, 0, red, out);
            HIP_TRY(hipMemcpyAsync(h, red, sizeof(h), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));  // the factor is the result, and whether any colour is valid picks pass 2's values
            const int use_ones = h[OT_RED_ANY_GAMUT] == 0.0;
            const double crmin = (use_ones || !std::isfinite(h[OT_RED_CRMIN])) ? 1.0 : h[OT_RED_CRMIN];
            const double f = std::sqrt(crmin);
            result[0] = f < 0.32 ? 0.32 : (f > 1.0 ? 1.0 : f);
            if (out) hipLaunchKernelGGL(col_chroma_kernel, grid, block, 0, st, in, npx, 2, L_th, use_ones, red, out);
            break;
        }
        case OT_COL_LOG_SRGB: {
            if (int rc = red_init(red, OT_CRED_N, st)) return rc;
            hipLaunchKernelGGL(col_ymax_kernel, grid, block, 0, st, in, npx, 1, red);
            hipLaunchKernelGGL(col_log_kernel, grid, block, 0, st, in, npx, 0, 0.0, 0.0, red, out);
            HIP_TRY(hipMemcpyAsync(h, red, sizeof(h), hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));  // srgb.py:418, 431: nothing positive or one lightness only -> a copy
            const double lmin = h[OT_CRED_LMIN], lmax = h[OT_CRED_LPMAX];
            result[0] = (h[OT_CRED_ANY_POS] == 0.0 || !std::isfinite(lmin) || lmin == lmax) ? 1.0 : 0.0;
            if (result[0] != 0.0) {
                HIP_TRY(hipMemcpyAsync(out, in, sizeof(double) * 3 * (size_t)npx, hipMemcpyDeviceToDevice, st));
                break;
            }
            hipLaunchKernelGGL(col_log_kernel, grid, block, 0, st, in, npx, 1, 99.5 / std::log(lmin / lmax), lmax, red, out);
            if (int rc = srgb_chain(out, out, npx, 1, true, true, true, 0.0, NAN, red, st)) return rc;
            break;
        }
        case OT_COL_SPECTRAL_COLORMAP: {
            double* obs = (double*)(lease.p() + o_obs);
            double* xyz = (double*)(lease.p() + o_xyz);
            double *rgba = xyz + 3 * npx, *rgbp = xyz + 6 * npx;
            HIP_TRY(hipMemcpyAsync(obs, ot_observer_xyz, sizeof(ot_observer_xyz), hipMemcpyHostToDevice, st));
            hipLaunchKernelGGL(col_spectral_kernel, grid, block, 0, st, in, npx, 0, obs, rgba, rgbp, xyz);
            if (int rc = srgb_chain(xyz, rgba, npx, 1, true, false, false, 0.0, NAN, red, st)) return rc;
            if (int rc = srgb_chain(xyz, rgbp, npx, 2, true, false, false, 0.0, NAN, red, st)) return rc;
            hipLaunchKernelGGL(col_spectral_kernel, grid, block, 0, st, in, npx, 1, obs, rgba, rgbp, out);
            break;
        }
        default: hipLaunchKernelGGL(col_map_kernel, grid, block, 0, st, in, npx, op, 0, red, out);
    }
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
