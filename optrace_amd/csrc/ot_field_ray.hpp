// What the analyses of ray lines per field and band share (field analysis: ot_field.hpp; MTF analysis: ot_mtf.hpp): the planes of a
// section from a piece's first ray on, and the test and the line (a, m) of one ray -- steps 1 and 2 of DESIGN.md "Field analysis",
// one body, so that both form the same bits.
#pragma once
#include "ot_device.hpp"

#define FD_NO_BAND 255u

// The planes of section k from the first ray of a piece on.  Workgroup-uniform.
struct FdSection {
    const uint8_t* key;
    const float *w, *wl;
    const double *x0, *y0, *z0, *x1, *y1, *z1;
};
OT_DEV FdSection fd_section(const double* __restrict__ p, const float* __restrict__ w, const float* __restrict__ wl,
                            const uint8_t* __restrict__ key, int64_t N, int nt, int k) {
    return {key, w + N * k, wl, p + N * k, p + N * (k + nt), p + N * (k + 2 * (int64_t)nt), p + N * (k + 1), p + N * (k + 1 + nt),
            p + N * (k + 1 + 2 * (int64_t)nt)};
}

// Ray r, whose key is a band (definition, steps 1 and 2): used?  Then its weight, d_z, and, where d_z != 0, the line (a, m).
struct FdRay {
    double w, dz, ax, ay, mx, my;
};
OT_DEV bool fd_ray(const FdSection& S, uint32_t r, double ox, double oy, double oz, FdRay& q) {
    const float wi = S.w[r];
    if (!(wi > 0.f)) return false;
    const double px = S.x0[r], py = S.y0[r], pz = S.z0[r];
    const double dx = S.x1[r] - px, dy = S.y1[r] - py, dz = S.z1[r] - pz;
    if (!(dx * dx + dy * dy + dz * dz > 0.0)) return false;  // (the square of a length above 0, and no NaN)
    q.w = (double)wi;
    q.dz = dz;
    if (dz == 0.0) return true;
    const double qx = px - ox, qy = py - oy, qz = pz - oz;
    q.mx = dx / dz;
    q.my = dy / dz;
    q.ax = qx - qz * q.mx;
    q.ay = qy - qz * q.my;
    return true;
}
