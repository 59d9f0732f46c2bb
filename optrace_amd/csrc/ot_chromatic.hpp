// Chromatic analysis of a stored trace (Raytracer.chromatic_analysis): per band of wavelengths the sums for the point closest to
// the band's ray lines in section k, and where the band's rays cross a plane z = z0 -- power, centroid, second moments about the
// band's own centroid, largest distance from it.  Definition: DESIGN.md "Chromatic analysis"; the record's slots:
// include/optrace_amd.h.
//   focus    per band the 17 sums of ot_wavefront_focus (ot_wavefront.hpp, wf_focus_kernel: the same terms)
//   pass 1   over the band's used rays with d_z != 0: sum w, count, sum w x, sum w y, sum w wl at the crossing points
//   pass 2   about the centroid c of pass 1, (dx, dy) = (x, y) - c formed before squaring: sum w dx^2, sum w dy^2, sum w dx dy,
//            the largest dx^2 + dy^2, and the band's used rays with d_z == 0
// All bands go in one launch per pass: workgroup (i, b) walks the rays as workgroup i of gridDim.x and takes those of band b.  A
// lane reads its ray's key, one byte, and the weight, the positions and the wavelength only when the key is its band's: a wave
// without a ray of the band touches none of their lines.  The passes add in the fixed order of ot_block_reduce.hpp.
// Defines kernels that are no templates: included by ot_chromatic_api.hip alone.
#pragma once
#include "ot_block_reduce.hpp"
#include "ot_device.hpp"
#include "ot_wavefront_ray.hpp"  // the slots of the focus record

// slots of the record (include/optrace_amd.h, ot_chromatic_plane): pass 1 carries the first CH_M1 of them, pass 2 the rest
enum { CH_W = 0, CH_COUNT, CH_WX, CH_WY, CH_WWL, CH_M1, CH_WDX2 = CH_M1, CH_WDY2, CH_WDXDY, CH_R2MAX, CH_PARALLEL, CH_M };
static_assert(CH_M == OT_CHROM_M && CH_M1 == 5 && WFF_M == OT_WF_FOCUS_M, "the records of the header");
#define CH_M2 (CH_M - CH_M1)

// The planes of section k from the first ray of a launch on: the host has added that ray's index to p, w and wl and its place in
// the range to key, so that n <= 2^28 rays are addressed with 32-bit offsets.  Workgroup-uniform.
struct ChSection {
    const uint8_t* key;
    const float *w, *wl;
    const double *x0, *y0, *z0, *x1, *y1, *z1;
};
OT_DEV ChSection ch_section(const double* __restrict__ p, const float* __restrict__ w, const float* __restrict__ wl,
                            const uint8_t* __restrict__ key, int64_t N, int nt, int k) {
    return {key, w + N * k, wl, p + N * k, p + N * (k + nt), p + N * (k + 2 * (int64_t)nt), p + N * (k + 1), p + N * (k + 1 + nt),
            p + N * (k + 1 + 2 * (int64_t)nt)};
}

// Ray r if it is a used ray of `band` (definition, step 1): its weight, the start p of the section, d = p[k + 1] - p and |d|
struct ChRay {
    double w, px, py, pz, dx, dy, dz, L;
};
OT_DEV bool ch_ray(const ChSection& S, uint32_t r, unsigned band, ChRay& q) {
    if (S.key[r] != band) return false;
    const float wi = S.w[r];
    if (!(wi > 0.f)) return false;
    q.w = (double)wi;
    q.px = S.x0[r];
    q.py = S.y0[r];
    q.pz = S.z0[r];
    q.dx = S.x1[r] - q.px;
    q.dy = S.y1[r] - q.py;
    q.dz = S.z1[r] - q.pz;
    q.L = ot_sqrt(q.dx * q.dx + q.dy * q.dy + q.dz * q.dz);
    return q.L > 0.0;
}

// part[n_bands][blocks_total][WFF_M]; this launch fills the workgroups block0 .. block0 + gridDim.x - 1 of every band
__global__ __launch_bounds__(OT_RED_THREADS) void ch_focus_kernel(const double* __restrict__ p, const float* __restrict__ w,
                                                                  const uint8_t* __restrict__ key, int64_t N, int nt, int k, uint32_t n,
                                                                  unsigned block0, unsigned blocks_total, double ox, double oy, double oz,
                                                                  double* __restrict__ part) {
    const unsigned b = blockIdx.y;
    const ChSection S = ch_section(p, w, nullptr, key, N, nt, k);
    double v[WFF_M];
#pragma unroll
    for (int m = 0; m < WFF_M; m++) v[m] = 0.0;
    const uint32_t stride = gridDim.x * OT_RED_THREADS;  // (at most 2^18 beyond n <= 2^28: no wrap)
    for (uint32_t r = blockIdx.x * OT_RED_THREADS + threadIdx.x; r < n; r += stride) {
        ChRay q;
        if (!ch_ray(S, r, b, q)) continue;
        const double wd = q.w, px = q.px - ox, py = q.py - oy, pz = q.pz - oz;
        const double sx = q.dx / q.L, sy = q.dy / q.L, sz = q.dz / q.L;
        const double sp = sx * px + sy * py + sz * pz;
        v[WFF_W] += wd;
        v[WFF_COUNT] += 1.0;  // (exact up to 2^53 rays)
        v[WFF_P + 0] += wd * px;
        v[WFF_P + 1] += wd * py;
        v[WFF_P + 2] += wd * pz;
        v[WFF_S + 0] += wd * sx;
        v[WFF_S + 1] += wd * sy;
        v[WFF_S + 2] += wd * sz;
        v[WFF_A + 0] += wd * (1.0 - sx * sx);
        v[WFF_A + 1] -= wd * (sx * sy);
        v[WFF_A + 2] -= wd * (sx * sz);
        v[WFF_A + 3] += wd * (1.0 - sy * sy);
        v[WFF_A + 4] -= wd * (sy * sz);
        v[WFF_A + 5] += wd * (1.0 - sz * sz);
        v[WFF_B + 0] += wd * (px - sx * sp);
        v[WFF_B + 1] += wd * (py - sy * sp);
        v[WFF_B + 2] += wd * (pz - sz * sp);
    }
    block_reduce_fixed<WFF_M, red_max()>(v, part + ((int64_t)b * blocks_total + block0 + blockIdx.x) * WFF_M);
}

// part[n_bands][blocks_total][CH_M1]
__global__ __launch_bounds__(OT_RED_THREADS) void ch_first_kernel(const double* __restrict__ p, const float* __restrict__ w,
                                                                  const float* __restrict__ wl, const uint8_t* __restrict__ key, int64_t N,
                                                                  int nt, int k, uint32_t n, unsigned block0, unsigned blocks_total,
                                                                  double z0, double* __restrict__ part) {
    const unsigned b = blockIdx.y;
    const ChSection S = ch_section(p, w, wl, key, N, nt, k);
    double v[CH_M1] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const uint32_t stride = gridDim.x * OT_RED_THREADS;
    for (uint32_t r = blockIdx.x * OT_RED_THREADS + threadIdx.x; r < n; r += stride) {
        ChRay q;
        if (!ch_ray(S, r, b, q) || q.dz == 0.0) continue;
        const double t = (z0 - q.pz) / q.dz, x = q.px + t * q.dx, y = q.py + t * q.dy;
        v[CH_W] += q.w;
        v[CH_COUNT] += 1.0;
        v[CH_WX] += q.w * x;
        v[CH_WY] += q.w * y;
        v[CH_WWL] += q.w * (double)S.wl[r];
    }
    block_reduce_fixed<CH_M1, red_max()>(v, part + ((int64_t)b * blocks_total + block0 + blockIdx.x) * CH_M1);
}

// part[n_bands][blocks_total][CH_M2]; rec: the records with the slots of pass 1 in place
__global__ __launch_bounds__(OT_RED_THREADS) void ch_central_kernel(const double* __restrict__ p, const float* __restrict__ w,
                                                                    const uint8_t* __restrict__ key, int64_t N, int nt, int k, uint32_t n,
                                                                    unsigned block0, unsigned blocks_total, double z0,
                                                                    const double* __restrict__ rec, double* __restrict__ part) {
    const unsigned b = blockIdx.y;
    const ChSection S = ch_section(p, w, nullptr, key, N, nt, k);
    const double* m = rec + (int64_t)CH_M * b;
    // the centroid: the same two IEEE quotients as the host forms from the record (no ray in the sums: NaN, and nothing reads it)
    const double cx = m[CH_WX] / m[CH_W], cy = m[CH_WY] / m[CH_W];
    double v[CH_M2] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const uint32_t stride = gridDim.x * OT_RED_THREADS;
    for (uint32_t r = blockIdx.x * OT_RED_THREADS + threadIdx.x; r < n; r += stride) {
        ChRay q;
        if (!ch_ray(S, r, b, q)) continue;
        if (q.dz == 0.0) {
            v[CH_PARALLEL - CH_M1] += 1.0;
            continue;
        }
        const double t = (z0 - q.pz) / q.dz, x = q.px + t * q.dx, y = q.py + t * q.dy, dx = x - cx, dy = y - cy;
        v[CH_WDX2 - CH_M1] += q.w * (dx * dx);
        v[CH_WDY2 - CH_M1] += q.w * (dy * dy);
        v[CH_WDXDY - CH_M1] += q.w * (dx * dy);
        v[CH_R2MAX - CH_M1] = fmax(v[CH_R2MAX - CH_M1], dx * dx + dy * dy);
    }
    block_reduce_fixed<CH_M2, red_max(CH_R2MAX - CH_M1)>(v, part + ((int64_t)b * blocks_total + block0 + blockIdx.x) * CH_M2);
}

// A band without a ray in the sums has no second moments: NaN in place of the zeros that were added up (the largest distance
// stays the 0 the lanes started from).  One thread per band.
__global__ void ch_finish_kernel(int n_bands, double* __restrict__ rec) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bands) return;
    double* m = rec + (int64_t)CH_M * b;
    if (m[CH_COUNT] == 0.0)
        for (int s = CH_WDX2; s <= CH_WDXDY; s++) m[s] = __builtin_nan("");
}
