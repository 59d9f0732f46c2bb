// Per-ray device functions of the wavefront analysis that more than one translation unit needs (ot_wavefront.hpp: focus,
// paths, map and fit; ot_psf.hpp: the ray records of the Huygens sum; ot_fans.hpp: the pupil cuts; ot_wavefield.hpp: the paths and
// the fit per field and band): the rays of a section, their sphere step and path, the slots of the moments record, the unit-disc
// coordinates of an entry, the Zernike polynomials.  No kernels here.
#pragma once
#include "ot_device.hpp"

// slots of the focus record and the moments record (include/optrace_amd.h)
enum { WFF_W = 0, WFF_COUNT, WFF_P, WFF_S = 5, WFF_A = 8, WFF_B = 14, WFF_M = 17 };
enum { WF_W = 0, WF_COUNT, WF_WOPL, WF_WU, WF_WV, WF_WWL, WF_OPL_MIN, WF_OPL_MAX, WF_WOPD2, WF_R2MAX, WF_PUPIL_R, WF_M };

// ---- the rays of a section ------------------------------------------------------------------------------------------
struct WfRay {
    V3 p, s;  // start of the section and its direction, re-derived from the stored positions
    double w;
    bool used;  // w > 0 and a section of positive length
};

OT_DEV V3 wf_position(const ot_rays& R, int64_t r, int j) {
    const int64_t N = R.N, nt = R.nt;
    V3 p = {R.p[r + N * j], R.p[r + N * (j + nt)], R.p[r + N * (j + 2 * nt)]};
    return p;
}

// (p0: the start of section k where the caller holds it already)
OT_DEV WfRay wf_section(const ot_rays& R, int64_t r, int k, const V3& p0) {
    WfRay q;
    q.p = p0;
    q.w = (double)R.w[r + R.N * k];
    const V3 p1 = wf_position(R, r, k + 1);
    const double dx = p1.x - p0.x, dy = p1.y - p0.y, dz = p1.z - p0.z;
    const double L = ot_sqrt(dx * dx + dy * dy + dz * dz);
    q.used = q.w > 0.0 && L > 0.0;
    q.s.x = dx / L;
    q.s.y = dy / L;
    q.s.z = dz / L;
    return q;
}

// The sphere step of a ray (definition, step 4), shared by wf_paths_kernel and psf_rays_kernel: where the line of section k from
// p0 = p[k] meets the sphere about (cx, cy, cz).  used: the ray counts (wf_section); hit: its line meets the sphere (a NaN
// discriminant does not: the ray has no place on it); t and h = p0 + t s - c hold numbers only then.
struct WfSphere {
    V3 h;
    double t, w;
    bool used, hit;
};
OT_DEV WfSphere wf_sphere(const ot_rays& R, int64_t r, int k, const V3& p0, double cx, double cy, double cz, double radius) {
    WfSphere o;
    const WfRay q = wf_section(R, r, k, p0);
    o.used = q.used;
    o.hit = false;
    o.w = q.w;
    o.t = o.h.x = o.h.y = o.h.z = 0.0;
    if (q.used) {
        const double sg = radius > 0.0 ? 1.0 : -1.0;
        const double qx = p0.x - cx, qy = p0.y - cy, qz = p0.z - cz;
        const double b = q.s.x * qx + q.s.y * qy + q.s.z * qz;
        const double c = (qx * qx + qy * qy + qz * qz) - radius * radius;
        const double D = b * b - c;
        if (D >= 0.0) {
            o.hit = true;
            o.t = -b - sg * ot_sqrt(D);
            o.h.x = qx + o.t * q.s.x;
            o.h.y = qy + o.t * q.s.y;
            o.h.z = qz + o.t * q.s.z;
        }
    }
    return o;
}

// The path of a ray to the sphere (definition, steps 4 to 6), shared by wf_paths_kernel and wvf_paths_kernel (ot_wavefield.hpp):
// the path sum over the sections before k in ascending j, the sphere step, opl and the pupil coordinates (u, v).  A ray that is
// not used, or whose line misses the sphere (-> true), gets wi = 0 and NaN elsewhere.  Reads p, w and n.
OT_DEV bool wf_path(const ot_rays& R, int64_t r, int k, double cx, double cy, double cz, double radius, double& ui, double& vi, double& li,
                    float& wi) {
    const int64_t N = R.N;
    const double nan = __builtin_nan("");
    bool miss = false;
    ui = vi = li = nan;
    wi = 0.f;
    if (R.w[r + N * k] > 0.f) {
        V3 p0 = wf_position(R, r, 0);
        double sum = 0.0;
        for (int j = 0; j < k; j++) {  // ascending j, as the definition says
            const V3 p1 = wf_position(R, r, j + 1);
            const double dx = p1.x - p0.x, dy = p1.y - p0.y, dz = p1.z - p0.z;
            sum += R.n[r + N * j] * ot_sqrt(dx * dx + dy * dy + dz * dz);
            p0 = p1;
        }
        const WfSphere h = wf_sphere(R, r, k, p0, cx, cy, cz, radius);
        if (h.hit) {
            const double ax = fabs(radius);
            li = sum + R.n[r + N * k] * h.t;
            ui = h.h.x / ax;
            vi = h.h.y / ax;
            wi = (float)h.w;
        }
        miss = h.used && !h.hit;
    }
    return miss;
}

// the means every later pass subtracts: the same IEEE quotients as the host forms from the record
struct WfMeans {
    double opl, u, v;
};
OT_DEV WfMeans wf_means(const double* __restrict__ mom) { return {mom[WF_WOPL] / mom[WF_W], mom[WF_WU] / mom[WF_W], mom[WF_WV] / mom[WF_W]}; }

// Unit-disc coordinates of an entry.  pupil_radius NaN: the largest distance from the pupil centre (moments), every entry
// inside; otherwise the caller's, and entries beyond it are left out.  All entries in one place: the centre of the disc.
struct WfPupil {
    double cu, cv, radius;
    bool given;
};
OT_DEV WfPupil wf_pupil(const double* __restrict__ mom, double pupil_radius) {
    const WfMeans c = wf_means(mom);
    const bool given = pupil_radius == pupil_radius;
    return {c.u, c.v, given ? pupil_radius : mom[WF_PUPIL_R], given};
}
OT_DEV bool wf_unit_disc(const WfPupil& P, double u, double v, double* x, double* y) {
    const bool spread = P.radius > 0.0;
    *x = spread ? (u - P.cu) / P.radius : 0.0;
    *y = spread ? (v - P.cv) / P.radius : 0.0;
    return !(P.given && *x * *x + *y * *y > 1.0);
}

// ---- Zernike polynomials, Noll's order -------------------------------------------------------------------------------
// Z_j = N_n^m R_n^|m|(rho) cos(m theta) for even j, sin(|m| theta) for odd j, 1 for m = 0.  rho^m cos / sin (m theta) are the
// real and imaginary parts of (x + i y)^m, and R_n^m / rho^m is a polynomial in rho^2 whose coefficients, times the norm, are
// compile-time constants: no trigonometry, no division, no special case at the centre.
constexpr int wf_noll_n(int j) {  // radial order of Z_j, j from 1
    int n = 0;
    while ((n + 1) * (n + 2) / 2 < j) n++;
    return n;
}
constexpr int wf_noll_m(int j) {  // azimuthal order |m|
    const int n = wf_noll_n(j), p = j - n * (n + 1) / 2 - 1;
    return n % 2 ? 2 * (p / 2) + 1 : 2 * ((p + 1) / 2);
}
constexpr double wf_factorial(int k) { return k < 2 ? 1.0 : k * wf_factorial(k - 1); }
// coefficient of rho^(n - 2 i) in R_n^m
constexpr double wf_radial_coeff(int n, int m, int i) {
    return (i % 2 ? -1.0 : 1.0) * wf_factorial(n - i) / (wf_factorial(i) * wf_factorial((n + m) / 2 - i) * wf_factorial((n - m) / 2 - i));
}
// sqrt(n + 1) and sqrt(2 n + 2), n = 0 .. 7
constexpr double wf_norm0[8] = {1.0, 1.4142135623730951, 1.7320508075688772, 2.0, 2.23606797749979, 2.449489742783178,
                                2.6457513110645907, 2.8284271247461903};
constexpr double wf_normm[8] = {1.4142135623730951, 2.0, 2.449489742783178, 2.8284271247461903, 3.1622776601683795,
                                3.4641016151377544, 3.7416573867739413, 4.0};

template <int J>
struct WfZernikeTerm {
    static constexpr int n = wf_noll_n(J), m = wf_noll_m(J), deg = (n - m) / 2;
    static constexpr double norm = m ? wf_normm[n] : wf_norm0[n];
    // norm times the coefficients of R_n^m / rho^m, highest power of t = rho^2 first (at most four: n <= 7); constants of the
    // class, so that the compiler holds numbers and no calls
    static constexpr double c0 = norm * wf_radial_coeff(n, m, 0), c1 = deg >= 1 ? norm * wf_radial_coeff(n, m, 1) : 0.0,
                            c2 = deg >= 2 ? norm * wf_radial_coeff(n, m, 2) : 0.0, c3 = deg >= 3 ? norm * wf_radial_coeff(n, m, 3) : 0.0;
    static_assert(deg <= 3, "radial orders up to 7");
    // cm[i], sm[i]: real and imaginary part of (x + i y)^i; t = x^2 + y^2
    static OT_DEV double eval(const double (&cm)[8], const double (&sm)[8], double t) {
        double r = c0;
        if constexpr (deg >= 1) r = r * t + c1;
        if constexpr (deg >= 2) r = r * t + c2;
        if constexpr (deg >= 3) r = r * t + c3;
        return r * (m == 0 ? 1.0 : J % 2 ? sm[m] : cm[m]);
    }
};
template <int JT, int J = 1>
struct WfZernikeAll {
    static OT_DEV void eval(double (&Z)[JT], const double (&cm)[8], const double (&sm)[8], double t) {
        Z[J - 1] = WfZernikeTerm<J>::eval(cm, sm, t);
        if constexpr (J < JT) WfZernikeAll<JT, J + 1>::eval(Z, cm, sm, t);
    }
};
template <int JT>
OT_DEV void wf_zernike_all(double x, double y, double (&Z)[JT]) {
    double cm[8], sm[8];
    cm[0] = 1.0;
    sm[0] = 0.0;
#pragma unroll
    for (int i = 1; i < 8; i++) {
        cm[i] = cm[i - 1] * x - sm[i - 1] * y;
        sm[i] = cm[i - 1] * y + sm[i - 1] * x;
    }
    WfZernikeAll<JT>::eval(Z, cm, sm, x * x + y * y);
}
