// Per-pixel colour arithmetic shared by the image stage (ot_image.hpp, behind RenderImage.get and convolve()) and the colour
// stage (ot_color.hpp, behind ot.color): color.xyz_to_luv / luv_to_xyz / luv_* luv.py, the sRGB matrix and gamma curve and both
// gamut-triangle projections of srgb.py, xyz_to_xyY xyz.py, the observer lookup of observers.py.  Device functions only, no
// kernels: any unit may include it.  One copy of every formula -- both stages give the same bits for the same pixel.
#pragma once
#include "ot_device.hpp"
#include "cie_observer_table.inc"

OT_DEV void to_rgbl(double X, double Y, double Z, double& r, double& g, double& b) {  // srgb.py:124-128
    r = 3.2404542 * X + -1.5371385 * Y + -0.4985314 * Z;
    g = -0.9692660 * X + 1.8760108 * Y + 0.0415560 * Z;
    b = 0.0556434 * X + -0.2040259 * Y + 1.0572252 * Z;
}

// luv.py xyz_to_luv for one pixel (xyz already clipped at 0 by the caller where the reference clips)
OT_DEV void xyz_to_luv1(double X, double Y, double Z, double Yn, double& L, double& u, double& v) {
    X = fmax(X, 0.0);
    Y = fmax(Y, 0.0);
    Z = fmax(Z, 0.0);
    L = u = v = 0.0;
    if (!(Y > 0)) return;
    const double un = 0.19783982, vn = 0.4683363;
    double t = 1 / Yn * Y;
    L = (t > 0.008856) ? 116 * cbrt(t) - 16 : 903.3 * t;
    double D = 1 / (X + 15 * Y + 3 * Z);
    double uu = 4 * X * D, vv = 9 * Y * D;
    double L13 = 13 * L;
    u = L13 * (uu - un);
    v = L13 * (vv - vn);
}

OT_DEV void luv_to_xyz1(double L, double u, double v, double& X, double& Y, double& Z) {  // luv.py luv_to_xyz
    X = Y = Z = 0.0;
    if (!(L > 0)) return;
    const double un = 0.19783982, vn = 0.4683363;
    if (L > 903.3 * 0.008856) {
        double q = 1.0 / 116 * (L + 16);
        Y = q * q * q;
    } else {
        Y = 1 / 903.3 * L;
    }
    double L13 = 13 * L;
    X = 9.0 / 4 * Y * (u + L13 * un) / (v + L13 * vn);
    Z = 3 * Y * (L13 / (v + L13 * vn) - 5.0 / 3) - 1.0 / 3 * X;
}

// srgb.py:_triangle_intersect: project (x, y) towards the whitepoint w onto the gamut triangle r, g, b
OT_DEV void triangle_intersect(double rx, double ry, double gx, double gy, double bx, double by, double wx, double wy,
                               double& x, double& y) {
    double phir = atan2(ry - wy, rx - wx);
    double phig = atan2(gy - wy, gx - wx);
    double phib = atan2(by - wy, bx - wx) + 2 * M_PI;
    double phi = atan2(y - wy, x - wx);
    if (phi < 0) phi += 2 * M_PI;
    double aw = tan(phi);
    double abg = (gy - by) / (gx - bx), abr = (ry - by) / (rx - bx), agr = (ry - gy) / (rx - gx);
    bool is_bg = (phi <= phib) && (phi > phig);
    bool is_gr = (phi <= phig) && (phi > phir);
    if (is_bg) {
        x = (y - x * aw + (bx * abg - by)) / (abg - aw);
        y = x * abg + (by - bx * abg);
    } else if (is_gr) {
        x = (y - x * aw + (gx * agr - gy)) / (agr - aw);
        y = x * agr + (gy - gx * agr);
    } else {
        x = (y - x * aw + (bx * abr - by)) / (abr - aw);
        y = x * abr + (by - bx * abr);
    }
}

OT_DEV double srgb_gamma(double v) {  // srgb_linear_to_srgb srgb.py:358-376
    double a = 0.055, av = fabs(v);
    if (av <= 0.0031308) return v * 12.92;
    double sg = (v > 0) - (v < 0);
    return sg * ((1 + a) * pow(av, 1 / 2.4) - a);
}

OT_DEV double srgb_inverse_gamma(double v) {  // srgb_to_srgb_linear srgb.py:30-47
    double a = 0.055, av = fabs(v);
    if (av <= 0.04045) return 1 / 12.92 * v;
    double sg = (v > 0) - (v < 0);
    return sg * pow(1 / (1 + a) * (av + a), 2.4);
}

OT_DEV void wave_atomic_max(double* addr, double v) {  // NaN-ignoring maximum (np.nanmax)
    double m = wave_max(isnan(v) ? -__builtin_inf() : v);
    if (__lane_id() == 0 && m > -__builtin_inf()) atomic_max_f64(addr, m);
}

OT_DEV void wave_atomic_min(double* addr, double v) {
    double m = wave_min(isnan(v) ? __builtin_inf() : v);
    if (__lane_id() == 0 && m < __builtin_inf()) atomic_min_f64(addr, m);
}

// srgb.py:_get_chroma_scale for one pixel: valid-colour mask and squared chroma factor towards the sRGB triangle
OT_DEV void chroma_scale1(double L, double u, double v, bool& in_gamut, double& cr2) {
    const double un = 0.19783982, vn = 0.4683363;
    double u_ = un, v_ = vn;
    if (L > 0) {
        u_ += 1.0 / 13 * u / L;
        v_ += 1.0 / 13 * v / L;
    }
    bool l1 = v_ > (0.5065 - 0.013) / (0.6235 - 0.255) * (u_ - 0.2555) + 0.01373;
    bool l2 = v_ < (0.5065 - 0.6) / (0.6235 - 0.0) * u_ + 0.6;
    bool l3 = u_ > 0;
    bool l4 = v_ > (0.013 - 0.28) / (0.255 - 0) * u_ + 0.28;
    bool l5 = v_ > (0.0 - 0.48) / (0.18 - 0) * u_ + 0.48;
    in_gamut = l1 && l2 && l3 && l4 && l5;
    double cr0 = (u_ - un) * (u_ - un) + (v_ - vn) * (v_ - vn);
    triangle_intersect(0.4507042254, 0.5228873239, 0.125, 0.5625, 0.1754385965, 0.1578947368, un, vn, u_, v_);
    double cr1 = (u_ - un) * (u_ - un) + (v_ - vn) * (v_ - vn);
    cr2 = cr1 / (cr0 + 1e-9);
}

// srgb.py:313-352 for one pixel: XYZ -> XYZ' of the rendering intent
//   intent 0 = Ignore, 1 = Absolute, 2 = Perceptual with the final per-image chroma_scale
OT_DEV void intent_correct1(double& X, double& Y, double& Z, int intent, double chroma_scale, int use_ones) {
    double r, g, b;
    to_rgbl(X, Y, Z, r, g, b);
    if (intent == 1) {
        if (r < 0 || g < 0 || b < 0) {  // chroma-clip towards the whitepoint in xy (srgb.py:322-330)
            double s = X + Y + Z;
            double x = 0.31272, y = 0.32903;
            if (s > 0) {
                x = X / s;
                y = Y / s;
            }
            triangle_intersect(0.64, 0.33, 0.30, 0.60, 0.15, 0.06, 0.31272, 0.32903, x, y);
            double k = Y / ((y > 0) ? y : __builtin_inf());
            X = k * x;
            Z = k * (1 - x - y);
        }
    } else if (intent == 2) {
        double L, u, v;
        xyz_to_luv1(X, Y, Z, 1.0, L, u, v);
        bool in_gamut;
        double cr2 = 1.0;
        if (!use_ones) chroma_scale1(L, u, v, in_gamut, cr2);  // srgb.py:209-210: all ones if nothing is in gamut
        double cr = sqrt(cr2);
        if (cr > chroma_scale) cr = chroma_scale;
        luv_to_xyz1(L, u * cr, v * cr, X, Y, Z);
    }
}

// _to_srgb's normalisation (`if normalize and (nmax := np.nanmax(RGBL_))`, srgb.py:120) and xyz_to_srgb's clip (srgb.py:403)
OT_DEV void rgbl_finish1(double& r, double& g, double& b, double nmax, bool normalize, bool clip) {
    if (normalize && nmax != 0 && !isnan(nmax) && isfinite(nmax)) {
        double s = 1 / nmax;
        r *= s;
        g *= s;
        b *= s;
    }
    if (clip) {
        r = fmin(fmax(r, 0.0), 1.0);
        g = fmin(fmax(g, 0.0), 1.0);
        b = fmin(fmax(b, 0.0), 1.0);
    }
}

OT_DEV double luv_chroma1(double u, double v) { return sqrt(u * u + v * v); }                 // luv.py luv_chroma
OT_DEV double luv_saturation1(double L, double u, double v) { return (L > 0) ? sqrt(u * u + v * v) / L : 0.0; }  // luv_saturation
OT_DEV double luv_hue1(double u, double v) {                                                   // luv_hue
    double hue = 180 / M_PI * atan2(v, u);
    if (hue < 0) hue += 360;
    return hue;
}

// color.x/y/z_observer observers.py:14-41 = np.interp on the 1 nm CIE grid: the interval index is floor(wl - 360);
// obs: the 471 x 3 table (LDS copy)
OT_DEV void observer_xyz_at(const double* obs, double l, double& xo, double& yo, double& zo) {
    xo = yo = zo = 0.0;
    double u = l - OT_OBS_WL0;
    if (u >= 0.0 && u <= (double)(OT_OBS_N - 1)) {
        int j = (int)floor(u);
        if (j >= OT_OBS_N - 1) {
            xo = obs[3 * (OT_OBS_N - 1)];
            yo = obs[3 * (OT_OBS_N - 1) + 1];
            zo = obs[3 * (OT_OBS_N - 1) + 2];
        } else {
            double t = l - (OT_OBS_WL0 + (double)j);
            const double* f0 = &obs[3 * j];
            xo = (f0[3] - f0[0]) / 1.0 * t + f0[0];
            yo = (f0[4] - f0[1]) / 1.0 * t + f0[1];
            zo = (f0[5] - f0[2]) / 1.0 * t + f0[2];
        }
    } else if (l != l) {
        xo = yo = zo = l;  // np.interp hands a NaN wavelength through
    }
}

