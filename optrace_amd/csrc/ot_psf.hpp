// Huygens point spread function of a traced bundle (Raytracer.huygens_psf): the coherent sum of one spherical wavelet per ray
// over the points of an image plane.  Definition: DESIGN.md "Huygens PSF".
//   rays  per ray of the range its record: q = h / |R| (the point on the reference sphere about the focus), tau0 = OPD / lambda
//         in turns, kappa = n / lambda, a = sqrt(w); all zero for a ray that is not used
//   sum   U(x) = sum_i a_i exp(2 pi i tau_i(x)) at n_px^2 image points and once more on the axis, A = sum a, sum a^2 -- per band
//         of the rays and per image plane (ot_psf_stack, Raytracer.huygens_stack); ot_psf_sum is one band and one plane
//   combine  the bands' fields into intensity, Strehl ratios, band weights and noise floor (ot_psf_combine)
// The sum is a dense rays x points product bound by the f64 vector pipe: a workgroup holds a tile of points in registers,
// OT_PSF_PPL per lane, and walks one chunk of the rays, whose records are the same for every lane and arrive by scalar loads.
// Partial sums per (plane, chunk, point) go to the workspace; a last kernel adds the chunks of a band in index order.  Tiles and
// chunks follow from (n, n_px, the starts and the number of planes) alone: two calls return the same bits.
// Defines kernels that are no templates: included by ot_psf_api.hip alone -- and, with OT_PSF_NO_KERNELS defined, for the lanes'
// arithmetic and the chunk rule without the kernels, by ot_psf_field_api.hip.
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

#ifndef OT_PSF_NO_KERNELS
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

#endif  // OT_PSF_NO_KERNELS

// a ray's record in scalar registers (the index is the same in every lane: the constant address space makes these scalar loads)
struct PsfRec {
    double qx, qy, qz, tau0, kappa, a;
};
OT_DEV PsfRec psf_load(const OT_CONST double* rec, int64_t n, int64_t i) {
    return {rec[i + n * PSF_QX], rec[i + n * PSF_QY], rec[i + n * PSF_QZ], rec[i + n * PSF_TAU0], rec[i + n * PSF_KAPPA], rec[i + n * PSF_A]};
}

// What a lane holds of its OT_PSF_PPL image points: delta_x, delta_y, delta . delta and the sums Re U, Im U.
struct PsfLane {
    double dx[OT_PSF_PPL], dy[OT_PSF_PPL], dd[OT_PSF_PPL], re[OT_PSF_PPL], im[OT_PSF_PPL];
};
// the points p0 + j * 64 + lane, j < OT_PSF_PPL, of the plane dz: point p at row p / n_px, column p % n_px, the point n_px^2 on the axis
OT_DEV void psf_lane_points(PsfLane& L, int p0, int lane, int P, int n_px, double size, double dz) {
    const double step = size / (double)n_px, half = 0.5 * (double)n_px;
#pragma unroll
    for (int j = 0; j < OT_PSF_PPL; j++) {
        const int p = p0 + j * 64 + lane;
        const bool image = p < P - 1;  // (points beyond the list are summed as the axis point and not stored)
        const int row = image ? p / n_px : 0, col = image ? p - row * n_px : 0;
        L.dx[j] = image ? ((double)col + 0.5 - half) * step : 0.0;
        L.dy[j] = image ? ((double)row + 0.5 - half) * step : 0.0;
        L.dd[j] = L.dx[j] * L.dx[j] + L.dy[j] * L.dy[j] + dz * dz;
        L.re[j] = L.im[j] = 0.0;
    }
}
// The arithmetic of one ray at the points of a lane.  With
// delta = x - c, ax = |R| (m2ax = -2 ax, ax2 = ax^2) and sg = sign(R):
//   dq = delta . q                    num = delta . delta - 2 ax dq             dist = sqrt(num + ax^2 q . q) = |delta - h|
//   e = num / (dist + ax)  = |delta - h| - ax without cancellation              tau = tau0 + sg kappa e
// then r = tau - rint(tau), exact, and sin, cos (2 pi r) from the polynomial kernels of sincospi_small.  A record of zeros gives
// dist >= 0, a denominator ax > 0, tau = 0 and adds a = 0: no NaN.
OT_DEV void psf_ray_points(PsfLane& L, const PsfRec& q, double dz, double ax, double m2ax, double ax2, double sg) {
    const double dzq = dz * q.qz, r2 = ax2 * (q.qx * q.qx + q.qy * q.qy + q.qz * q.qz), ks = sg * q.kappa;
#pragma unroll
    for (int j = 0; j < OT_PSF_PPL; j++) {
        const double dq = __builtin_fma(L.dx[j], q.qx, __builtin_fma(L.dy[j], q.qy, dzq));
        const double num = __builtin_fma(m2ax, dq, L.dd[j]);
        const double den = ot_sqrt(num + r2) + ax;
        const double e = ot_div_r(num, den, ot_rcp3(den));
        const double tau = __builtin_fma(ks, e, q.tau0);
        double sn, cs;
        sincospi_small(2.0 * (tau - rint(tau)), &sn, &cs);
        L.re[j] = __builtin_fma(q.a, cs, L.re[j]);
        L.im[j] = __builtin_fma(q.a, sn, L.im[j]);
    }
}
// out[2 P + 2] = re[P] | im[P] | sum a | sum a^2 of one chunk; the lane that holds the axis point stores the two sums
OT_DEV void psf_store(const PsfLane& L, double* out, int p0, int lane, int P, double sa, double sa2) {
#pragma unroll
    for (int j = 0; j < OT_PSF_PPL; j++) {
        const int p = p0 + j * 64 + lane;
        if (p < P) {
            out[p] = L.re[j];
            out[(int64_t)P + p] = L.im[j];
        }
        if (p == P - 1) {
            out[2 * (int64_t)P] = sa;
            out[2 * (int64_t)P + 1] = sa2;
        }
    }
}

// ---- the sum: per band of the rays and per image plane in one launch (ot_psf_stack); ot_psf_sum is one band and one plane ------------
#define OT_PSF_MAX_BANDS_ 32
#define OT_PSF_MAX_PLANES_ 64
#ifndef OT_PSF_STACK_ROUNDS
#define OT_PSF_STACK_ROUNDS 4  // rounds of OT_PSF_GROUPS workgroups that a stack of that many planes or more is cut into
#endif

// By value to the kernels: band b holds the records [start[b], start[b + 1]) and the chunks [chunk0[b], chunk0[b + 1]), each of
// chunk_len rays at the most, so that no chunk straddles a band; plane z lies at dz[z].  The index into these arrays is the same
// in every lane: scalar loads from the kernel's argument segment.
struct PsfStack {
    int64_t start[OT_PSF_MAX_BANDS_ + 1];
    int32_t chunk0[OT_PSF_MAX_BANDS_ + 1];
    int32_t n_bands;
    int64_t chunk_len;
    double dz[OT_PSF_MAX_PLANES_];
};

// psf_shape for the stack: the chunk length is that of psf_shape for all n records with the workgroups aimed at divided by
// tiles x planes; with one plane this is psf_shape(n, n_px) itself
static inline PsfShape psf_stack_shape(int64_t n, int n_px, int n_planes) {
    PsfShape s = psf_shape(n, n_px);
    const int64_t by_n = (n + OT_PSF_MIN_CHUNK - 1) / OT_PSF_MIN_CHUNK;
    int64_t c = OT_PSF_GROUPS * (n_planes < OT_PSF_STACK_ROUNDS ? n_planes : OT_PSF_STACK_ROUNDS) / (s.tiles * n_planes);
    if (c > by_n) c = by_n;
    s.chunks = c < 1 ? 1 : c;
    s.chunk_len = (n + s.chunks - 1) / s.chunks;
    return s;
}

#ifndef OT_PSF_NO_KERNELS
// The hot kernel.  Workgroup (tile, chunk, plane): wave wv, lane l holds the points tile * OT_PSF_TILE + (wv * OT_PSF_PPL + j) * 64 + l,
// j < OT_PSF_PPL, of the plane's dz; a wave whose points all lie beyond the last one leaves at once.  The chunk finds its band and
// its ray range from the starts; a chunk behind its band's last ray stores zeros.  part[planes][chunks][2 P + 2].
__global__ __launch_bounds__(OT_PSF_THREADS, 4) void psf_sum_kernel(int64_t n, const double* __restrict__ rec_, double ax, double sg,
                                                                    int n_px, double size, const PsfStack S,
                                                                    double* __restrict__ part) {
    const int P = n_px * n_px + 1;  // (n_px <= 1024: 32-bit point indices)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int p0 = (int)blockIdx.x * OT_PSF_TILE + wv * (OT_PSF_PPL * 64);
    if (p0 >= P) return;  // (wave-uniform)
    const int c = blockIdx.y;
    int b = 0;
    while (b + 1 < S.n_bands && c >= S.chunk0[b + 1]) b++;  // (uniform; empty bands own no chunk and are passed over)
    const double dz = S.dz[blockIdx.z];
    PsfLane L;
    psf_lane_points(L, p0, lane, P, n_px, size, dz);
    double sa = 0.0, sa2 = 0.0;
    const int64_t end = S.start[b + 1], i0 = S.start[b] + (int64_t)(c - S.chunk0[b]) * S.chunk_len,
                  i1 = i0 + S.chunk_len < end ? i0 + S.chunk_len : end;
    const double m2ax = -2.0 * ax, ax2 = ax * ax;
    const OT_CONST double* rec = as_const(rec_);
    if (i0 < i1) {
        PsfRec next = psf_load(rec, n, i0);
        for (int64_t i = i0; i < i1; i++) {
            const PsfRec q = next;
            next = psf_load(rec, n, i + 1 < i1 ? i + 1 : i);  // (one ray ahead; the SIMD's other waves cover what is left of the latency)
            sa += q.a;  // (every lane adds a and a^2 of the chunk, ray by ray; the lane that holds the axis point stores them)
            sa2 = __builtin_fma(q.a, q.a, sa2);
            psf_ray_points(L, q, dz, ax, m2ax, ax2, sg);
        }
    }
    psf_store(L, part + ((int64_t)blockIdx.z * gridDim.y + c) * (2 * (int64_t)P + 2), p0, lane, P, sa, sa2);
}

// part[planes][chunks][2 P + 2] -> field[planes][bands][2][n_px^2] and sums[planes][bands][5] = Re U, Im U on the axis | sum a |
// sum a^2 | (sum a^2 kappa: psf_band_kappa_kernel, for ot_psf_stack alone): one thread per (plane, band, slot) adds the band's
// chunks in index order; a band without a chunk gives zeros.  With one band and one plane: field[2][n_px^2] and the four doubles
// that ot_psf_sum calls centre.
__global__ __launch_bounds__(OT_PSF_THREADS) void psf_final_kernel(const double* __restrict__ part, int64_t chunks, int64_t P,
                                                                   const PsfStack S, double* __restrict__ field,
                                                                   double* __restrict__ sums) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = 2 * P + 2;
    if (s >= stride) return;
    const int64_t b = blockIdx.y, z = blockIdx.z, K = S.n_bands, px = P - 1;
    const double* in = part + z * chunks * stride + s;
    double r = 0.0;
    for (int64_t c = S.chunk0[b]; c < S.chunk0[b + 1]; c++) r += in[c * stride];
    double* f = field + (z * K + b) * 2 * px;
    double* o = sums + (z * K + b) * 5;
    if (s < px)
        f[s] = r;
    else if (s == px)
        o[0] = r;
    else if (s < 2 * P - 1)
        f[s - 1] = r;  // Im of point s - P, behind the px values of Re
    else if (s == 2 * P - 1)
        o[1] = r;
    else
        o[2 + (s - 2 * P)] = r;
}

// sum a^2 kappa of band b, the one sum that no plane and no tile needs, by one workgroup: thread t adds the records start + t,
// start + t + 256, ... in that order, then the 256 partial sums are added pairwise in LDS, 128 apart first: an order fixed by the
// starts alone.  sums[planes][bands][5], slot 4 of every plane.
__global__ __launch_bounds__(OT_PSF_THREADS) void psf_band_kappa_kernel(int64_t n, const double* __restrict__ rec, const PsfStack S,
                                                                        int n_planes, double* __restrict__ sums) {
    __shared__ double sh[OT_PSF_THREADS];
    const int b = blockIdx.x, t = threadIdx.x;
    double r = 0.0;
    for (int64_t i = S.start[b] + t; i < S.start[b + 1]; i += OT_PSF_THREADS) {
        const double a = rec[i + n * PSF_A];
        r = __builtin_fma(a * a, rec[i + n * PSF_KAPPA], r);
    }
    sh[t] = r;
    __syncthreads();
    for (int h = OT_PSF_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) sh[t] += sh[t + h];
        __syncthreads();
    }
    if (t < n_planes) sums[((int64_t)t * S.n_bands + b) * 5 + 4] = sh[0];
}

// field and sums of ot_psf_stack -> the figures of DESIGN.md "Polychromatic through-focus PSF".  One thread per (plane, point), the
// point n_px^2 on the axis.  With A, W, S4 = sums[z][b][2 .. 4] of the thread's own plane and bands in ascending order, those with
// W > 0 alone:  kb = S4 / W,  t_b = W * (kb * kb),  T = (..(0 + t_0) + t_1 ..),  g_b = t_b / T,
//   v_b = (re * re + im * im) / (A * A),  value = (..(0 + g_0 * v_0) + g_1 * v_1 ..)
// -> intensity[z][point], or strehl[z] on the axis, where band_strehl[z][b] = v_b too (NaN for a band without a ray); the thread
// of plane 0 on the axis also writes g[b] (0 for such a band) and noise_floor = (..(0 + g_0 * (W_0 / (A_0 * A_0))) + ..).
__global__ __launch_bounds__(OT_PSF_THREADS) void psf_combine_kernel(int K, int n_px, const double* __restrict__ field,
                                                                     const double* __restrict__ sums, double* __restrict__ intensity,
                                                                     double* __restrict__ band_strehl, double* __restrict__ strehl,
                                                                     double* __restrict__ g, double* __restrict__ noise_floor) {
    const int64_t px = (int64_t)n_px * n_px, p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.y;
    if (p > px) return;
    const double* sz = sums + z * K * 5;
    double T = 0.0;
    for (int b = 0; b < K; b++) {
        const double W = sz[b * 5 + 3];
        if (W > 0.0) {
            const double kb = sz[b * 5 + 4] / W;
            T += W * (kb * kb);
        }
    }
    double value = 0.0, floor_ = 0.0;
    for (int b = 0; b < K; b++) {
        const double A = sz[b * 5 + 2], W = sz[b * 5 + 3];
        double gb = 0.0, v = __builtin_nan("");
        if (W > 0.0) {
            const double kb = sz[b * 5 + 4] / W;
            gb = W * (kb * kb) / T;
            const double* f = field + (z * K + b) * 2 * px;
            const double re = p < px ? f[p] : sz[b * 5], im = p < px ? f[px + p] : sz[b * 5 + 1];
            v = (re * re + im * im) / (A * A);
            value += gb * v;
            floor_ += gb * (W / (A * A));
        }
        if (p == px) {
            band_strehl[z * K + b] = v;
            if (z == 0) g[b] = gb;
        }
    }
    if (p < px)
        intensity[z * px + p] = value;
    else {
        strehl[z] = value;
        if (z == 0) noise_floor[0] = floor_;
    }
}
#endif  // OT_PSF_NO_KERNELS
