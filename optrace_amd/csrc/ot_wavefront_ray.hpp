// Per-ray device functions of the wavefront analysis that more than one translation unit needs (ot_wavefront.hpp: focus,
// paths, map and fit; ot_psf.hpp: the ray records of the Huygens sum; ot_fans.hpp: the pupil cuts): the rays of a section, their
// sphere step, the slots of the moments record, the unit-disc coordinates of an entry.  No kernels here.
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
