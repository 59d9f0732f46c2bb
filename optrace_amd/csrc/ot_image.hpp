// Image conversion of the rendered XYZW histogram: RenderImage.get render_image.py:131-222 with
// color.xyz_to_srgb / xyz_to_srgb_linear srgb.py:267-407, color.xyz_to_luv / luv_to_xyz / luv_* luv.py,
// color.xyz_to_xyY xyz.py, the chroma clipping helper _triangle_intersect srgb.py:133-183 and _get_chroma_scale
// srgb.py:186-222.  One lane per (down-binned) pixel; the few image-wide quantities (maxima, any-flags, the
// minimum chroma factor) are reduced on the device between the passes (wave shuffle + one atomic per wave).
// The per-pixel arithmetic lives in ot_color_px.hpp, shared with the colour stage (ot_color.hpp).
// Defines kernels that are no templates: included by ot_image_api.hip alone.
#pragma once
#include "ot_color_px.hpp"

#define OT_IMG_IRRADIANCE 0
#define OT_IMG_ILLUMINANCE 1
#define OT_IMG_SRGB_ABSOLUTE 2
#define OT_IMG_SRGB_PERCEPTUAL 3
#define OT_IMG_OUTSIDE_GAMUT 4
#define OT_IMG_LIGHTNESS 5
#define OT_IMG_HUE 6
#define OT_IMG_CHROMA 7
#define OT_IMG_SATURATION 8

// slots of the reduction scratch (doubles)
#define OT_RED_YMAX 0        // nanmax(Y | Y > 0)                                  luv.py: Yn (normalize=True)
#define OT_RED_RGBMAX 1      // nanmax(M XYZ) of the unmodified image               srgb.py:_to_srgb
#define OT_RED_ANY_INV 2     // any(RGBL < 0)                                       srgb.py:317
#define OT_RED_LMAX 3        // max L (Luv, normalize=False) of the clipped image   srgb.py:249
#define OT_RED_ANY_GAMUT 4   // any(in_gamut)                                       srgb.py:209
#define OT_RED_CRMIN 5       // min cr_fact2 over valid & L > L_th * Lmax           srgb.py:250-251
#define OT_RED_RGBMAX2 6     // nanmax(M XYZ') of the corrected image
#define OT_RED_N 8

// INTER_AREA down-binning by an integer factor = mean of fact x fact bins (render_image.py:174), 4 channels
__global__ __launch_bounds__(256) void img_downbin_kernel(const double* __restrict__ hist, int Nx, int Ny, int fact,
                                                          double* __restrict__ out) {
    const int nx = Nx / fact, ny = Ny / fact;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)nx * ny) return;
    const int y = (int)(i / nx), x = (int)(i - (int64_t)y * nx);
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int dy = 0; dy < fact; dy++)
        for (int dx = 0; dx < fact; dx++) {
            const double* h = hist + (((int64_t)(y * fact + dy)) * Nx + (x * fact + dx)) * 4;
            a0 += h[0];
            a1 += h[1];
            a2 += h[2];
            a3 += h[3];
        }
    const double inv = 1.0 / ((double)fact * fact);
    out[i * 4 + 0] = a0 * inv;
    out[i * 4 + 1] = a1 * inv;
    out[i * 4 + 2] = a2 * inv;
    out[i * 4 + 3] = a3 * inv;
}

// Passes 1 to 3 are templates on the pixel stride S in doubles: 4 for the XYZW working copy here, 3 for the (npx, 3) arrays of
// the colour stage (ot_color.hpp), which launches the same kernels.
// pass 1: image-wide quantities of the unmodified image
template <int S>
__global__ __launch_bounds__(256) void img_reduce1_kernel(const double* __restrict__ img, int64_t npx, double* __restrict__ red) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = i < npx;
    double X = 0, Y = 0, Z = 0;
    if (act) {
        X = img[i * S];
        Y = img[i * S + 1];
        Z = img[i * S + 2];
    }
    double r, g, b;
    to_rgbl(X, Y, Z, r, g, b);
    const double ninf = -__builtin_inf();
    wave_atomic_max(&red[OT_RED_YMAX], (act && fmax(Y, 0.0) > 0) ? fmax(Y, 0.0) : ninf);
    wave_atomic_max(&red[OT_RED_RGBMAX], act ? fmax(fmax(r, g), b) : ninf);
    bool inv = act && (r < 0 || g < 0 || b < 0);
    if (__ballot(inv) && __lane_id() == 0) red[OT_RED_ANY_INV] = 1.0;
    // Luv of the clipped image with Yn = 1 (normalize=False) for the perceptual intent
    double L, u, v;
    xyz_to_luv1(X, Y, Z, 1.0, L, u, v);
    wave_atomic_max(&red[OT_RED_LMAX], act ? L : ninf);
}

// pass 2 (perceptual intent): any(in_gamut) and the minimum squared chroma factor over valid, bright pixels
template <int S>
__global__ __launch_bounds__(256) void img_reduce2_kernel(const double* __restrict__ img, int64_t npx, double L_th,
                                                          double* __restrict__ red) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = i < npx;
    double L = 0, u = 0, v = 0;
    if (act) xyz_to_luv1(img[i * S], img[i * S + 1], img[i * S + 2], 1.0, L, u, v);
    bool in_gamut;
    double cr2;
    chroma_scale1(L, u, v, in_gamut, cr2);
    in_gamut = in_gamut && act;
    if (__ballot(in_gamut) && __lane_id() == 0) red[OT_RED_ANY_GAMUT] = 1.0;
    bool use = in_gamut && (L > L_th * red[OT_RED_LMAX]);
    wave_atomic_min(&red[OT_RED_CRMIN], use ? cr2 : __builtin_inf());
}

// pass 3: corrected XYZ' per pixel (src -> dst, which may be the same array) and nanmax(M XYZ')
//   intent 0 = Ignore, 1 = Absolute, 2 = Perceptual with the final per-image chroma_scale (srgb.py:313-352)
template <int S>
__global__ __launch_bounds__(256) void img_correct_kernel(const double* src, double* dst, int64_t npx, int intent,
                                                          double chroma_scale, int use_ones, double* __restrict__ red) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool act = i < npx;
    double X = 0, Y = 0, Z = 0;
    if (act) {
        X = src[i * S];
        Y = src[i * S + 1];
        Z = src[i * S + 2];
    }
    intent_correct1(X, Y, Z, intent, chroma_scale, use_ones);
    if (act) {
        dst[i * S] = X;
        dst[i * S + 1] = Y;
        dst[i * S + 2] = Z;
    }
    double r, g, b;
    to_rgbl(X, Y, Z, r, g, b);
    wave_atomic_max(&red[OT_RED_RGBMAX2], act ? fmax(fmax(r, g), b) : -__builtin_inf());
}

// final pass: write the requested quantity
__global__ __launch_bounds__(256) void img_final_kernel(const double* __restrict__ img, int64_t npx, int mode, double apx,
                                                        double K, const double* __restrict__ red, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npx) return;
    const double X = img[i * 4], Y = img[i * 4 + 1], Z = img[i * 4 + 2], W = img[i * 4 + 3];
    const bool normalize = !(mode & OT_IMG_FLAG_NO_NORMALIZE), clip = !(mode & OT_IMG_FLAG_NO_CLIP);
    mode &= ~(OT_IMG_FLAG_NO_NORMALIZE | OT_IMG_FLAG_NO_CLIP);
    switch (mode) {
        case OT_IMG_IRRADIANCE: out[i] = 1 / apx * W; return;
        case OT_IMG_ILLUMINANCE: out[i] = K / apx * Y; return;
        case OT_IMG_SRGB_ABSOLUTE:
        case OT_IMG_SRGB_PERCEPTUAL: {
            double r, g, b;
            to_rgbl(X, Y, Z, r, g, b);
            rgbl_finish1(r, g, b, red[OT_RED_RGBMAX2], normalize, clip);
            out[i * 3 + 0] = srgb_gamma(r);
            out[i * 3 + 1] = srgb_gamma(g);
            out[i * 3 + 2] = srgb_gamma(b);
            return;
        }
        case OT_IMG_OUTSIDE_GAMUT: {
            double r, g, b;
            to_rgbl(X, Y, Z, r, g, b);
            double nmax = red[OT_RED_RGBMAX];
            if (nmax != 0 && isfinite(nmax)) {
                double s = 1 / nmax;
                r *= s;
                g *= s;
                b *= s;
            }
            out[i] = (r < -1e-6 || g < -1e-6 || b < -1e-6) ? 1.0 : 0.0;
            return;
        }
        default: {
            double Yn = red[OT_RED_YMAX];
            double L = 0, u = 0, v = 0;
            if (isfinite(Yn)) xyz_to_luv1(X, Y, Z, Yn, L, u, v);  // no pixel with Y > 0: all zero (luv.py:34-35)
            if (mode == OT_IMG_LIGHTNESS) out[i] = L;
            else if (mode == OT_IMG_CHROMA) out[i] = luv_chroma1(u, v);
            else if (mode == OT_IMG_SATURATION) out[i] = luv_saturation1(L, u, v);
            else out[i] = luv_hue1(u, v);
        }
    }
}

// RenderImage._apply_rayleigh_filter render_image.py:257-296: "same"-size convolution of every channel with the
// (2ps+1)^2 Airy kernel.  The reference uses scipy.signal.fftconvolve; the kernel is small against the image, so
// a direct sum per output pixel (zero-padded borders, zero taps skipped, kernel staged in LDS) gives the same
// result without FFT round-off (the reference clamps its negative FFT noise to 0 afterwards).
__global__ __launch_bounds__(256) void img_convolve_kernel(const double* __restrict__ in, int Nx, int Ny,
                                                           const double* __restrict__ psf, int ps, double* __restrict__ out) {
    extern __shared__ double kern[];
    const int side = 2 * ps + 1;
    for (int k = threadIdx.x; k < side * side; k += blockDim.x) kern[k] = psf[k];
    __syncthreads();
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)Nx * Ny) return;
    const int y = (int)(i / Nx), x = (int)(i - (int64_t)y * Nx);
    double a0 = 0, a1 = 0, a2 = 0, a3 = 0;
    for (int j = 0; j < side; j++) {
        const int yy = y + ps - j;  // (f * g)[y] = sum_j g[j] f[y - (j - ps)]
        if (yy < 0 || yy >= Ny) continue;
        for (int k = 0; k < side; k++) {
            const int xx = x + ps - k;
            if (xx < 0 || xx >= Nx) continue;
            const double g = kern[j * side + k];
            if (g == 0.0) continue;
            const double* h = in + ((int64_t)yy * Nx + xx) * 4;
            a0 += g * h[0];
            a1 += g * h[1];
            a2 += g * h[2];
            a3 += g * h[3];
        }
    }
    double* o = out + i * 4;
    o[0] = fmax(a0, 0.0);
    o[1] = fmax(a1, 0.0);
    o[2] = fmax(a2, 0.0);
    o[3] = fmax(a3, 0.0);
}
