// Huygens point spread function of a traced bundle (Raytracer.huygens_psf): the coherent sum of one spherical wavelet per ray
// over the points of an image plane.  Definition: DESIGN.md "Huygens PSF".
//   rays  per ray of the range its record: q = h / |R| (the point on the reference sphere about the focus), tau0 = OPD / lambda
//         in turns, kappa = n / lambda, a = sqrt(w); all zero for a ray that is not used
//   sum   U(x) = sum_i a_i exp(2 pi i tau_i(x)) at n_px^2 image points and once more on the axis, A = sum a, sum a^2
// The sum is a dense rays x points product bound by the f64 vector pipe: a workgroup holds a tile of points in registers,
// OT_PSF_PPL per lane, and walks one chunk of the rays, whose records are the same for every lane and arrive by scalar loads.
// Partial sums per (chunk, point) go to the workspace; a last kernel adds the chunks in index order.  Tiles and chunks follow
// from (n, n_px) alone: two calls return the same bits.
// Defines kernels that are no templates: included by ot_psf_api.hip alone.
#pragma once
#include "ot_device.hpp"
#include "ot_wavefront_ray.hpp"

#define OT_PSF_THREADS 256
#define OT_PSF_PPL 4                                // image points per lane
#define OT_PSF_TILE (OT_PSF_THREADS * OT_PSF_PPL)  // image points per workgroup
#define OT_PSF_GROUPS 1024                          // workgroups aimed at: four waves per SIMD on 256 CUs, one round
#define OT_PSF_MIN_CHUNK 128                        // rays per chunk at least, so that the tile's set-up and stores stay small

// planes of the record list rec[OT_PSF_REC][n]
enum { PSF_QX = 0, PSF_QY, PSF_QZ, PSF_TAU0, PSF_KAPPA, PSF_A };

// (n, n_px) -> tiles of the points, chunks of the rays, doubles per chunk of the workspace: re[P] | im[P] | sum a | sum a^2
struct PsfShape {
    int64_t P, tiles, chunks, chunk_len, stride;
};
static inline PsfShape psf_shape(int64_t n, int n_px) {
    PsfShape s;
    s.P = (int64_t)n_px * n_px + 1;  // the last point lies on the axis
    s.tiles = (s.P + OT_PSF_TILE - 1) / OT_PSF_TILE;
    const int64_t by_n = (n + OT_PSF_MIN_CHUNK - 1) / OT_PSF_MIN_CHUNK;
    int64_t c = OT_PSF_GROUPS / s.tiles;
    if (c > by_n) c = by_n;
    s.chunks = c < 1 ? 1 : c;
    s.chunk_len = (n + s.chunks - 1) / s.chunks;
    s.stride = 2 * s.P + 2;
    return s;
}

// One thread per ray of [first, first + count): the sphere step of wf_paths_kernel on p, w and n of the storage, the wavelength,
// the path that ot_wavefront_paths left in `opl` and its mean from the moments record.  rec[6][count].
__global__ __launch_bounds__(OT_PSF_THREADS) void psf_rays_kernel(ot_rays R, int64_t first, int64_t count, int k, double cx, double cy,
                                                                  double cz, double radius, const double* __restrict__ opl,
                                                                  const double* __restrict__ mom, double* __restrict__ rec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int64_t r = first + i, N = R.N;
    double qx = 0.0, qy = 0.0, qz = 0.0, tau0 = 0.0, kappa = 0.0, a = 0.0;
    if (R.w[r + N * k] > 0.f) {
        const WfSphere h = wf_sphere(R, r, k, wf_position(R, r, k), cx, cy, cz, radius);
        const double l = opl[i];
        if (h.hit && l == l) {  // (a path that is no number belongs to no used ray: nothing of it may reach the sum)
            const double ax = fabs(radius), lambda = (double)R.wl[r] * 1e-6;  // nm -> mm
            qx = h.h.x / ax;
            qy = h.h.y / ax;
            qz = h.h.z / ax;
            tau0 = (l - wf_means(mom).opl) / lambda;
            kappa = R.n[r + N * k] / lambda;
            a = ot_sqrt(h.w);
        }
    }
    rec[i + count * PSF_QX] = qx;
    rec[i + count * PSF_QY] = qy;
    rec[i + count * PSF_QZ] = qz;
    rec[i + count * PSF_TAU0] = tau0;
    rec[i + count * PSF_KAPPA] = kappa;
    rec[i + count * PSF_A] = a;
}

// a ray's record in scalar registers (the index is the same in every lane: the constant address space makes these scalar loads)
struct PsfRec {
    double qx, qy, qz, tau0, kappa, a;
};
OT_DEV PsfRec psf_load(const OT_CONST double* rec, int64_t n, int64_t i) {
    return {rec[i + n * PSF_QX], rec[i + n * PSF_QY], rec[i + n * PSF_QZ], rec[i + n * PSF_TAU0], rec[i + n * PSF_KAPPA], rec[i + n * PSF_A]};
}

// The hot kernel.  Workgroup (tile, chunk): wave wv, lane l holds the points tile * OT_PSF_TILE + (wv * OT_PSF_PPL + j) * 64 + l,
// j < OT_PSF_PPL, point p at row p / n_px, column p % n_px, the point n_px^2 on the axis; a wave whose points all lie beyond the
// last one leaves at once.  Per ray and point, with delta = x - c, ax = |R| and sg = sign(R):
//   dq = delta . q                    num = delta . delta - 2 ax dq             dist = sqrt(num + ax^2 q . q) = |delta - h|
//   e = num / (dist + ax)  = |delta - h| - ax without cancellation              tau = tau0 + sg kappa e
// then r = tau - rint(tau), exact, and sin, cos (2 pi r) from the polynomial kernels of sincospi_small.  A record of zeros gives
// dist >= 0, a denominator ax > 0, tau = 0 and adds a = 0: no NaN.  Every lane also adds a and a^2 of the chunk, ray by ray; the lane
// that holds the axis point stores them.  part[chunks][2 P + 2].
__global__ __launch_bounds__(OT_PSF_THREADS, 4) void psf_sum_kernel(int64_t n, const double* __restrict__ rec_, double ax, double sg, int n_px,
                                                                    double size, double dz, int64_t chunk_len, double* __restrict__ part) {
    const int P = n_px * n_px + 1;  // (n_px <= 1024: 32-bit point indices)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int p0 = (int)blockIdx.x * OT_PSF_TILE + wv * (OT_PSF_PPL * 64);
    if (p0 >= P) return;  // (wave-uniform)
    const double step = size / (double)n_px, half = 0.5 * (double)n_px;
    double dx[OT_PSF_PPL], dy[OT_PSF_PPL], dd[OT_PSF_PPL], re[OT_PSF_PPL], im[OT_PSF_PPL];
#pragma unroll
    for (int j = 0; j < OT_PSF_PPL; j++) {
        const int p = p0 + j * 64 + lane;
        const bool image = p < P - 1;  // (points beyond the list are summed as the axis point and not stored)
        const int row = image ? p / n_px : 0, col = image ? p - row * n_px : 0;
        dx[j] = image ? ((double)col + 0.5 - half) * step : 0.0;
        dy[j] = image ? ((double)row + 0.5 - half) * step : 0.0;
        dd[j] = dx[j] * dx[j] + dy[j] * dy[j] + dz * dz;
        re[j] = im[j] = 0.0;
    }
    double sa = 0.0, sa2 = 0.0;
    const double m2ax = -2.0 * ax, ax2 = ax * ax;
    const OT_CONST double* rec = as_const(rec_);
    const int64_t c = blockIdx.y, i0 = c * chunk_len, i1 = i0 + chunk_len < n ? i0 + chunk_len : n;
    if (i0 < i1) {
        PsfRec next = psf_load(rec, n, i0);
        for (int64_t i = i0; i < i1; i++) {
            const PsfRec q = next;
            next = psf_load(rec, n, i + 1 < i1 ? i + 1 : i);  // (one ray ahead; the SIMD's other waves cover what is left of the latency)
            const double dzq = dz * q.qz, r2 = ax2 * (q.qx * q.qx + q.qy * q.qy + q.qz * q.qz), ks = sg * q.kappa;
            sa += q.a;
            sa2 = __builtin_fma(q.a, q.a, sa2);
#pragma unroll
            for (int j = 0; j < OT_PSF_PPL; j++) {
                const double dq = __builtin_fma(dx[j], q.qx, __builtin_fma(dy[j], q.qy, dzq));
                const double num = __builtin_fma(m2ax, dq, dd[j]);
                const double den = ot_sqrt(num + r2) + ax;
                const double e = ot_div_r(num, den, ot_rcp3(den));
                const double tau = __builtin_fma(ks, e, q.tau0);
                double sn, cs;
                sincospi_small(2.0 * (tau - rint(tau)), &sn, &cs);
                re[j] = __builtin_fma(q.a, cs, re[j]);
                im[j] = __builtin_fma(q.a, sn, im[j]);
            }
        }
    }
    double* out = part + c * (2 * (int64_t)P + 2);
#pragma unroll
    for (int j = 0; j < OT_PSF_PPL; j++) {
        const int p = p0 + j * 64 + lane;
        if (p < P) {
            out[p] = re[j];
            out[(int64_t)P + p] = im[j];
        }
        if (p == P - 1) {
            out[2 * (int64_t)P] = sa;
            out[2 * (int64_t)P + 1] = sa2;
        }
    }
}

// part[chunks][2 P + 2] -> field[2][n_px^2] and centre[4] = Re U, Im U on the axis | sum a | sum a^2: one thread per slot adds
// its partials in index order
__global__ __launch_bounds__(OT_PSF_THREADS) void psf_final_kernel(const double* __restrict__ part, int64_t chunks, int64_t P,
                                                                   double* __restrict__ field, double* __restrict__ centre) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = 2 * P + 2;
    if (s >= stride) return;
    double r = 0.0;
    for (int64_t c = 0; c < chunks; c++) r += part[c * stride + s];
    const int64_t px = P - 1;
    if (s < px)
        field[s] = r;
    else if (s == px)
        centre[0] = r;
    else if (s < 2 * P - 1)
        field[s - 1] = r;  // Im of point s - P, behind the px values of Re
    else if (s == 2 * P - 1)
        centre[1] = r;
    else
        centre[2 + (s - 2 * P)] = r;
}
