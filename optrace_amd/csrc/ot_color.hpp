// Colour stage: the conversions of optrace's color module on (npx, 3) float64 arrays of the caller (ot.color): xyz.py xyz_to_xyY /
// xyY_to_xyz, luv.py xyz_to_luv / luv_to_xyz / luv_to_u_v_l / luv_hue / luv_chroma / luv_saturation, srgb.py srgb_to_xyz /
// srgb_linear_to_xyz / xyz_to_srgb_linear / xyz_to_srgb / outside_srgb_gamut / get_chroma_scale / log_srgb / spectral_colormap.
// Plain streaming code, one lane per pixel (24 bytes in, 8 to 32 bytes out).  The per-pixel arithmetic is that of
// ot_color_px.hpp; the three passes of the rendering intents are the image stage's kernels (ot_image.hpp) at stride 3.
// Image-wide quantities are maxima, minima and flags only (wave shuffle + one atomic per wave), so every result is independent
// of where a pixel sits in its wave or workgroup.
// Defines kernels that are no templates: included by ot_image_api.hip alone, after ot_image.hpp.
#pragma once
#include "ot_image.hpp"

// reduction slots of the colour stage behind the image stage's OT_RED_*
#define OT_CRED_ANY_POS 8   // any(img > 0)                          srgb.py:418
#define OT_CRED_LMIN 9      // min L | L > 0                          srgb.py:429
#define OT_CRED_LPMAX 10    // max L | L > 0                          srgb.py:428
#define OT_CRED_N 16

OT_DEV void rgbl_to_xyz1(double r, double g, double b, double& X, double& Y, double& Z) {  // srgb_linear_to_xyz srgb.py:50-68
    X = 0.4124564 * r + 0.3575761 * g + 0.1804375 * b;
    Y = 0.2126729 * r + 0.7151522 * g + 0.0721750 * b;
    Z = 0.0193339 * r + 0.1191920 * g + 0.9503041 * b;
}

OT_DEV void luv_to_uv1(double L, double u, double v, double& u_, double& v_) {  // luv_to_u_v_l luv.py:112-127
    u_ = 0.19783982;
    v_ = 0.4683363;
    if (L > 0) {
        u_ += 1.0 / 13 * u / L;
        v_ += 1.0 / 13 * v / L;
    }
}

// nanmax(Y | Y > 0) alone: Yn of xyz_to_luv(normalize=True).  srgb != 0: the input is sRGB (log_srgb), and any(img > 0) is reduced too
__global__ __launch_bounds__(256) void col_ymax_kernel(const double* __restrict__ in, int64_t npx, int srgb, double* __restrict__ red) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = i < npx;
    double a = 0, Y = 0, c = 0;
    if (act) {
        a = in[i * 3];
        Y = in[i * 3 + 1];
        c = in[i * 3 + 2];
    }
    if (srgb) {
        if (__ballot(a > 0 || Y > 0 || c > 0) && __lane_id() == 0) red[OT_CRED_ANY_POS] = 1.0;
        double X, Z;
        rgbl_to_xyz1(srgb_inverse_gamma(a), srgb_inverse_gamma(Y), srgb_inverse_gamma(c), X, Y, Z);
    }
    Y = fmax(Y, 0.0);
    wave_atomic_max(&red[OT_RED_YMAX], (act && Y > 0) ? Y : -__builtin_inf());
}

// the conversions that need no image-wide quantity but Yn (read from red[OT_RED_YMAX] where `normalize`): 3 -> nch channels
__global__ __launch_bounds__(256) void col_map_kernel(const double* __restrict__ in, int64_t npx, int op, int normalize,
                                                      const double* __restrict__ red, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    const double a = in[i * 3], b = in[i * 3 + 1], c = in[i * 3 + 2];
    double o0 = 0, o1 = 0, o2 = 0;
    switch (op) {
        case OT_COL_XYZ_TO_XYY: {  // xyz.py:17-35: black -> whitepoint, Y = 0
            const double s = a + b + c;
            o0 = 0.31272;
            o1 = 0.32903;
            if (s > 0) {
                o0 = a / s;
                o1 = b / s;
            }
            o2 = b;
            break;
        }
        case OT_COL_XYY_TO_XYZ: {  // xyz.py:38-54
            o0 = a;
            o1 = b;
            o2 = 1 - a - b;
            if (b != 0) {
                const double k = c / b;
                o0 *= k;
                o1 *= k;
                o2 *= k;
            }
            break;
        }
        case OT_COL_XYZ_TO_LUV: {
            const double Yn = normalize ? red[OT_RED_YMAX] : 1.0;
            if (isfinite(Yn)) xyz_to_luv1(a, b, c, Yn, o0, o1, o2);  // no pixel with Y > 0: all zero (luv.py:36-37)
            break;
        }
        case OT_COL_LUV_TO_XYZ: luv_to_xyz1(a, b, c, o0, o1, o2); break;
        case OT_COL_LUV_TO_UVL:
            luv_to_uv1(a, b, c, o0, o1);
            o2 = a;
            break;
        case OT_COL_LUV_HUE: out[i] = luv_hue1(b, c); return;
        case OT_COL_LUV_CHROMA: out[i] = luv_chroma1(b, c); return;
        case OT_COL_LUV_SATURATION: out[i] = luv_saturation1(a, b, c); return;
        case OT_COL_SRGB_LINEAR_TO_XYZ: rgbl_to_xyz1(a, b, c, o0, o1, o2); break;
        default:  // OT_COL_SRGB_TO_XYZ
            rgbl_to_xyz1(srgb_inverse_gamma(a), srgb_inverse_gamma(b), srgb_inverse_gamma(c), o0, o1, o2);
    }
    out[i * 3] = o0;
    out[i * 3 + 1] = o1;
    out[i * 3 + 2] = o2;
}

// last pass of xyz_to_srgb_linear / xyz_to_srgb / outside_srgb_gamut: XYZ' (pass 3 left it in `io`) -> linear sRGB, normalised,
// clipped and gamma-corrected on request, in place; gamut != 0: the flag of srgb.py:92 into io[i] of a (npx) array instead
__global__ __launch_bounds__(256) void col_final_kernel(const double* xyz, int64_t npx, int normalize, int clip, int gamma,
                                                        int gamut, const double* __restrict__ red, double* io) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    double r, g, b;
    to_rgbl(xyz[i * 3], xyz[i * 3 + 1], xyz[i * 3 + 2], r, g, b);
    if (gamut) {
        rgbl_finish1(r, g, b, red[OT_RED_RGBMAX], true, false);
        io[i] = (r < -1e-6 || g < -1e-6 || b < -1e-6) ? 1.0 : 0.0;
        return;
    }
    rgbl_finish1(r, g, b, red[OT_RED_RGBMAX2], normalize, clip);
    io[i * 3] = gamma ? srgb_gamma(r) : r;
    io[i * 3 + 1] = gamma ? srgb_gamma(g) : g;
    io[i * 3 + 2] = gamma ? srgb_gamma(b) : b;
}

// get_chroma_scale srgb.py:242-264 on a Luv input.  pass 0: max L;  pass 1: any(in_gamut), min cr_fact2 over valid pixels above
// L_th * max L;  pass 2 (return_full): sqrt(cr_fact2) per pixel, ones where no pixel is valid (srgb.py:222-223)
__global__ __launch_bounds__(256) void col_chroma_kernel(const double* __restrict__ luv, int64_t npx, int pass, double L_th,
                                                         int use_ones, double* __restrict__ red, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = i < npx;
    double L = 0, u = 0, v = 0;
    if (act) {
        L = luv[i * 3];
        u = luv[i * 3 + 1];
        v = luv[i * 3 + 2];
    }
    if (pass == 0) {
        wave_atomic_max(&red[OT_RED_LMAX], act ? L : -__builtin_inf());
        return;
    }
    bool in_gamut;
    double cr2;
    chroma_scale1(L, u, v, in_gamut, cr2);
    if (pass == 1) {
        in_gamut = in_gamut && act;
        if (__ballot(in_gamut) && __lane_id() == 0) red[OT_RED_ANY_GAMUT] = 1.0;
        const bool use = in_gamut && (L > L_th * red[OT_RED_LMAX]);
        wave_atomic_min(&red[OT_RED_CRMIN], use ? cr2 : __builtin_inf());
    } else if (act) {
        out[i] = use_ones ? 1.0 : sqrt(cr2);
    }
}

// log_srgb srgb.py:410-444.  pass 0: min and max of the positive lightness (Yn in red[OT_RED_YMAX]);  pass 1: lightness rescaled
// logarithmically at unchanged chromaticity, back to XYZ (`k` = 99.5 / log(lmin / lmax)); xyz_to_srgb follows on `out`
__global__ __launch_bounds__(256) void col_log_kernel(const double* __restrict__ in, int64_t npx, int pass, double k, double lmax,
                                                      double* __restrict__ red, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = i < npx;
    double L = 0, u = 0, v = 0;
    const double Yn = red[OT_RED_YMAX];
    if (act && isfinite(Yn)) {
        double X, Y, Z;
        rgbl_to_xyz1(srgb_inverse_gamma(in[i * 3]), srgb_inverse_gamma(in[i * 3 + 1]), srgb_inverse_gamma(in[i * 3 + 2]), X, Y, Z);
        xyz_to_luv1(X, Y, Z, Yn, L, u, v);
    }
    if (pass == 0) {
        wave_atomic_min(&red[OT_CRED_LMIN], (L > 0) ? L : __builtin_inf());
        wave_atomic_max(&red[OT_CRED_LPMAX], (L > 0) ? L : -__builtin_inf());
        return;
    }
    if (!act) return;
    if (L > 0) {
        const double L2 = 100 - k * log(L / lmax);
        const double cs = L2 / L;
        L = L2;
        u *= cs;
        v *= cs;
    }
    double X, Y, Z;
    luv_to_xyz1(L, u, v, X, Y, Z);
    out[i * 3] = X;
    out[i * 3 + 1] = Y;
    out[i * 3 + 2] = Z;
}

OT_DEV void brightest_to_one(double& r, double& g, double& b) {  // srgb.py:587-588: rows that are not black, by their maximum
    if (r != 0 || g != 0 || b != 0) {
        const double m = fmax(fmax(r, g), b);
        r = r / m;
        g = g / m;
        b = b / m;
    }
}

// spectral_colormap srgb.py:569-606.  pass 0: wl -> XYZ of the observers (obs: device copy of the 471 x 3 table);
// pass 1: the two linear sRGB rows (Absolute and Perceptual intent), each normalised per wavelength, mixed, the fall-off, gamma
__global__ __launch_bounds__(256) void col_spectral_kernel(const double* __restrict__ wl, int64_t n, int pass,
                                                           const double* __restrict__ obs, const double* __restrict__ rgba,
                                                           const double* __restrict__ rgbp, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double l = wl[i];
    if (pass == 0) {
        double X, Y, Z;
        observer_xyz_at(obs, l, X, Y, Z);
        out[i * 3] = X;
        out[i * 3 + 1] = Y;
        out[i * 3 + 2] = Z;
        return;
    }
    double ra = rgba[i * 3], ga = rgba[i * 3 + 1], ba = rgba[i * 3 + 2];
    double rp = rgbp[i * 3], gp = rgbp[i * 3 + 1], bp = rgbp[i * 3 + 2];
    brightest_to_one(ra, ga, ba);
    brightest_to_one(rp, gp, bp);
    const double f = 1.0 / 4 * (1 - tanh((l - 650) / 50)) * (1 + tanh((l - 440) / 30));
    out[i * 4] = srgb_gamma((0.5 * ra + 0.5 * rp) * f);
    out[i * 4 + 1] = srgb_gamma((0.5 * ga + 0.5 * gp) * f);
    out[i * 4 + 2] = srgb_gamma((0.5 * ba + 0.5 * bp) * f);
    out[i * 4 + 3] = 1.0;
}
