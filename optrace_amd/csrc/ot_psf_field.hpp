// Huygens PSF across the field (Raytracer.huygens_field): the sum of ot_psf.hpp for the cells (field f, band b) of a field
// series in one launch, every field against a reference sphere of its own, then per field the combine step of the stack and a
// transfer function along the field's tangential and sagittal directions.  Definition: DESIGN.md "Huygens PSF across the field".
//   rays     per ray of the span the record of psf_rays_kernel against the sphere and the mean path of the ray's cell
//   sum      U per (cell, plane) at n_px^2 image points and on the axis, A = sum a, sum a^2, sum a^2 kappa: the workgroups,
//            lanes and arithmetic of psf_sum_kernel (psf_lane_points, psf_ray_points, psf_store: included, not copied), with the
//            cells -- up to 64 x 32, too many for a by-value argument -- in a table in device memory
//   combine  psf_combine_kernel per field
//   otf      sum_p J_p exp(-2 pi i nu (d . x_p)) along d = t_f and d = s_f, and its modulus over that at nu = 0
// Chunks and orders follow from (n, n_px, the starts and the numbers of fields and planes) alone: two calls return the same bits, and with
// one field they are those of ot_psf_stack.
// Expects ot_psf.hpp before it; defines kernels that are no templates: included by ot_psf_field_api.hip alone.
#pragma once
#include "ot_block_reduce.hpp"

#define OT_PSFF_FREQ_BLOCK 4                   // frequencies per workgroup of the transfer function
#define OT_PSFF_OTF_M (4 * OT_PSFF_FREQ_BLOCK + 1)  // its sums: per frequency sum J cos, sum J sin along t and along s; sum J

// The cell table, 8-byte words in device memory, C = F K cells, cell f K + b: start[C + 1] | chunk0[C + 1] | |R|[C] | sign R[C]
// (the two doubles as their bits).  Cell c holds the records [start[c], start[c + 1]) and the chunks [chunk0[c], chunk0[c + 1]),
// each of chunk_len rays at the most: no chunk straddles a cell, an empty cell owns none.  The index is the same in every lane:
// scalar loads through the constant address space.
OT_DEV int64_t psff_start(const OT_CONST int64_t* tab, int cells, int c) { return tab[c]; }
OT_DEV int64_t psff_chunk0(const OT_CONST int64_t* tab, int cells, int c) { return tab[cells + 1 + c]; }
OT_DEV double psff_ax(const OT_CONST int64_t* tab, int cells, int c) { return __longlong_as_double(tab[2 * cells + 2 + c]); }
OT_DEV double psff_sg(const OT_CONST int64_t* tab, int cells, int c) { return __longlong_as_double(tab[3 * cells + 2 + c]); }

// by value to the kernels: the ray ranges of the fields; the planes; the directions and frequencies of the transfer function
struct PsfFieldRanges {
    int64_t first[OT_FIELD_MAX_FIELDS], count[OT_FIELD_MAX_FIELDS];
};
struct PsfFieldPlanes {
    double dz[OT_PSF_MAX_PLANES_];
};
struct PsfFieldOtf {
    double t[OT_FIELD_MAX_FIELDS][2], nu[OT_PSFF_MAX_FREQ];
};

// One thread per entry of the span, entry i ray key_first + i: psf_rays_kernel with the sphere spheres[f][b] = (c, R) and the
// mean path moments[f][b][2] / moments[f][b][0] of the ray's cell -- f the field whose range holds the ray, b its key.  A ray of
// no field or no band, of a cell without a sphere, a ray that is not used, one that misses the sphere and one whose path is no
// number: six zeros.  rec[6][span].
__global__ __launch_bounds__(OT_PSF_THREADS) void psf_field_rays_kernel(ot_rays R, const PsfFieldRanges G, int F, int k,
                                                                        const uint8_t* __restrict__ key, int64_t key_first,
                                                                        int64_t span, int K, const double* __restrict__ spheres,
                                                                        const double* __restrict__ opl,
                                                                        const double* __restrict__ moments, double* __restrict__ rec) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= span) return;
    const int64_t r = key_first + i, N = R.N;
    int f = -1;
    for (int g = 0; g < F; g++)  // (uniform trip count; the ranges of the fields do not overlap)
        if (r >= G.first[g] && r - G.first[g] < G.count[g]) f = g;
    const int kb = key[i];
    double qx = 0.0, qy = 0.0, qz = 0.0, tau0 = 0.0, kappa = 0.0, a = 0.0;
    if (f >= 0 && kb < K && R.w[r + N * k] > 0.f) {
        const double* s = spheres + ((int64_t)f * K + kb) * 4;
        const double inf = __builtin_inf();
        if (fabs(s[0]) < inf && fabs(s[1]) < inf && fabs(s[2]) < inf && fabs(s[3]) < inf && s[3] != 0.0) {
            const double radius = s[3];
            const WfSphere h = wf_sphere(R, r, k, wf_position(R, r, k), s[0], s[1], s[2], radius);
            const double l = opl[i];
            if (h.hit && l == l) {
                const double* m = moments + ((int64_t)f * K + kb) * OT_WFF_M;
                const double ax = fabs(radius), lambda = (double)R.wl[r] * 1e-6;  // nm -> mm
                qx = h.h.x / ax;
                qy = h.h.y / ax;
                qz = h.h.z / ax;
                tau0 = (l - m[2] / m[0]) / lambda;
                kappa = R.n[r + N * k] / lambda;
                a = ot_sqrt(h.w);
            }
        }
    }
    rec[i + span * PSF_QX] = qx;
    rec[i + span * PSF_QY] = qy;
    rec[i + span * PSF_QZ] = qz;
    rec[i + span * PSF_TAU0] = tau0;
    rec[i + span * PSF_KAPPA] = kappa;
    rec[i + span * PSF_A] = a;
}

// The hot kernel: psf_sum_kernel with the cell of a chunk found in the table, grid (tiles, chunks, planes).  The chunk's cell is
// the last one whose first chunk is not behind it (a bisection on scalar registers: chunk0 ascends, chunk0[0] = 0 and
// chunk0[C] is the number of chunks); its sphere is the cell's.  part[planes][chunks][2 P + 2].
__global__ __launch_bounds__(OT_PSF_THREADS, 4) void psf_field_sum_kernel(int64_t n, const double* __restrict__ rec_,
                                                                         const int64_t* __restrict__ table_, int cells,
                                                                         int64_t chunk_len, int n_px, double size,
                                                                         const PsfFieldPlanes Z, double* __restrict__ part) {
    const int P = n_px * n_px + 1;  // (n_px <= 1024: 32-bit point indices)
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int p0 = (int)blockIdx.x * OT_PSF_TILE + wv * (OT_PSF_PPL * 64);
    if (p0 >= P) return;  // (wave-uniform)
    const int c = blockIdx.y;
    const OT_CONST int64_t* tab = as_const(table_);
    int cell = 0, above = cells;
    while (above - cell > 1) {  // (uniform)
        const int mid = (cell + above) >> 1;
        if (psff_chunk0(tab, cells, mid) <= c)
            cell = mid;
        else
            above = mid;
    }
    const double dz = Z.dz[blockIdx.z], ax = psff_ax(tab, cells, cell), sg = psff_sg(tab, cells, cell);
    PsfLane L;
    psf_lane_points(L, p0, lane, P, n_px, size, dz);
    double sa = 0.0, sa2 = 0.0;
    const int64_t end = psff_start(tab, cells, cell + 1),
                  i0 = psff_start(tab, cells, cell) + (int64_t)(c - psff_chunk0(tab, cells, cell)) * chunk_len,
                  i1 = i0 + chunk_len < end ? i0 + chunk_len : end;
    const double m2ax = -2.0 * ax, ax2 = ax * ax;
    const OT_CONST double* rec = as_const(rec_);
    if (i0 < i1) {
        PsfRec next = psf_load(rec, n, i0);
        for (int64_t i = i0; i < i1; i++) {
            const PsfRec q = next;
            next = psf_load(rec, n, i + 1 < i1 ? i + 1 : i);  // (one ray ahead, as in psf_sum_kernel)
            sa += q.a;
            sa2 = __builtin_fma(q.a, q.a, sa2);
            psf_ray_points(L, q, dz, ax, m2ax, ax2, sg);
        }
    }
    psf_store(L, part + ((int64_t)blockIdx.z * gridDim.y + c) * (2 * (int64_t)P + 2), p0, lane, P, sa, sa2);
}

// part[planes][chunks][2 P + 2] -> field[F][planes][K][2][n_px^2] and sums[F][planes][K][5] = Re U, Im U on the axis | sum a |
// sum a^2 | (sum a^2 kappa: psf_field_kappa_kernel): psf_final_kernel per cell, grid (threads over the slots, cells, planes).  One
// thread per (cell, plane, slot) adds the cell's chunks in index order; a cell without a chunk gives zeros.
__global__ __launch_bounds__(OT_PSF_THREADS) void psf_field_final_kernel(const double* __restrict__ part, int64_t chunks, int64_t P,
                                                                         const int64_t* __restrict__ table_, int cells, int K,
                                                                         double* __restrict__ field, double* __restrict__ sums) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = 2 * P + 2;
    if (s >= stride) return;
    const OT_CONST int64_t* tab = as_const(table_);
    const int cell = blockIdx.y;
    const int64_t f = cell / K, b = cell % K, z = blockIdx.z, Z = gridDim.z, px = P - 1;
    const double* in = part + z * chunks * stride + s;
    double r = 0.0;
    for (int64_t c = psff_chunk0(tab, cells, cell); c < psff_chunk0(tab, cells, cell + 1); c++) r += in[c * stride];
    double* fo = field + ((f * Z + z) * K + b) * 2 * px;
    double* o = sums + ((f * Z + z) * K + b) * 5;
    if (s < px)
        fo[s] = r;
    else if (s == px)
        o[0] = r;
    else if (s < 2 * P - 1)
        fo[s - 1] = r;  // Im of point s - P, behind the px values of Re
    else if (s == 2 * P - 1)
        o[1] = r;
    else
        o[2 + (s - 2 * P)] = r;
}

// sum a^2 kappa of a cell, the order of psf_band_kappa_kernel: thread t adds the records start + t, start + t + 256, ... in that
// order, then the 256 partial sums are added pairwise in LDS, 128 apart first.  One workgroup per cell; slot 4 of every plane.
__global__ __launch_bounds__(OT_PSF_THREADS) void psf_field_kappa_kernel(int64_t n, const double* __restrict__ rec,
                                                                         const int64_t* __restrict__ table_, int cells, int K,
                                                                         int n_planes, double* __restrict__ sums) {
    __shared__ double sh[OT_PSF_THREADS];
    const OT_CONST int64_t* tab = as_const(table_);
    const int cell = blockIdx.x, t = threadIdx.x;
    double r = 0.0;
    for (int64_t i = psff_start(tab, cells, cell) + t; i < psff_start(tab, cells, cell + 1); i += OT_PSF_THREADS) {
        const double a = rec[i + n * PSF_A];
        r = __builtin_fma(a * a, rec[i + n * PSF_KAPPA], r);
    }
    sh[t] = r;
    __syncthreads();
    for (int h = OT_PSF_THREADS / 2; h > 0; h >>= 1) {
        if (t < h) sh[t] += sh[t + h];
        __syncthreads();
    }
    const int64_t f = cell / K, b = cell % K;
    if (t < n_planes) sums[((f * n_planes + t) * K + b) * 5 + 4] = sh[0];
}

// psf_combine_kernel per field: grid (threads over the points and the axis, planes, fields), the same formulas in the same
// association on field[F][Z][K][2][px] and sums[F][Z][K][5] -> intensity[F][Z][px], band_strehl[F][Z][K], strehl[F][Z], g[F][K],
// noise_floor[F].  A field without a band of W > 0 has no image: NaN in intensity, strehl and noise_floor (g = 0, band_strehl NaN
// as for every band without a ray).
__global__ __launch_bounds__(OT_PSF_THREADS) void psf_field_combine_kernel(int K, int n_px, const double* __restrict__ field,
                                                                           const double* __restrict__ sums,
                                                                           double* __restrict__ intensity,
                                                                           double* __restrict__ band_strehl, double* __restrict__ strehl,
                                                                           double* __restrict__ g, double* __restrict__ noise_floor) {
    const int64_t px = (int64_t)n_px * n_px, p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, z = blockIdx.y, Z = gridDim.y,
                  f = blockIdx.z, fz = f * Z + z;
    if (p > px) return;
    const double* sz = sums + fz * K * 5;
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
            const double* fb = field + (fz * K + b) * 2 * px;
            const double re = p < px ? fb[p] : sz[b * 5], im = p < px ? fb[px + p] : sz[b * 5 + 1];
            v = (re * re + im * im) / (A * A);
            value += gb * v;
            floor_ += gb * (W / (A * A));
        }
        if (p == px) {
            band_strehl[fz * K + b] = v;
            if (z == 0) g[f * K + b] = gb;
        }
    }
    if (!(T > 0.0)) value = floor_ = __builtin_nan("");
    if (p < px)
        intensity[fz * px + p] = value;
    else {
        strehl[fz] = value;
        if (z == 0) noise_floor[f] = floor_;
    }
}

// The transfer function of a field's image along t = (tx, ty) and s = (-ty, tx).  Workgroup (block of frequencies, plane, field),
// thread l walks the pixels p = l, l + 256, ... in that order: with J = intensity - noise_floor, x = (column + 1/2 - n_px / 2) step,
// y = (row + 1/2 - n_px / 2) step, step = size / n_px -- the grid of psf_lane_points --, u_t = tx x + ty y and u_s = -ty x + tx y
// (two products and one sum each, not fused), per frequency nu the phase ph = nu u in turns, r = ph - rint(ph), exact, sin and cos
// (2 pi r) from sincospi_small, and  C += J cos,  S += J sin  (a product and a sum each, not fused); once per pixel J0 += J.  The
// 4 n + 1 sums of the 256 threads are then added by block_reduce_fixed: across the lanes of a wave 32, 16, .. 1 apart, then the four
// waves in ascending order.  out[F][Z][M][6] = C_t, -S_t, C_s, -S_s (the transfer function sum_p J_p exp(-2 pi i nu u_p)),
// sqrt(C_t^2 + S_t^2) / |J0| and the same along s.
__global__ __launch_bounds__(OT_RED_THREADS) void psf_field_otf_kernel(int n_px, double size, int M, const PsfFieldOtf D,
                                                                       const double* __restrict__ intensity,
                                                                       const double* __restrict__ noise_floor, double* __restrict__ out) {
    __shared__ double red[OT_PSFF_OTF_M];
    const int64_t px = (int64_t)n_px * n_px, z = blockIdx.y, Z = gridDim.y, f = blockIdx.z;
    const int m0 = blockIdx.x * OT_PSFF_FREQ_BLOCK;
    const double tx = D.t[f][0], ty = D.t[f][1], floor_ = noise_floor[f];
    const double step = size / (double)n_px, half = 0.5 * (double)n_px;
    const double* in = intensity + (f * Z + z) * px;
    double nu[OT_PSFF_FREQ_BLOCK], acc[OT_PSFF_OTF_M];
#pragma unroll
    for (int j = 0; j < OT_PSFF_FREQ_BLOCK; j++) nu[j] = D.nu[m0 + j < M ? m0 + j : M - 1];  // (behind the last: repeated, not stored)
#pragma unroll
    for (int j = 0; j < OT_PSFF_OTF_M; j++) acc[j] = 0.0;
    for (int64_t p = threadIdx.x; p < px; p += OT_RED_THREADS) {
        const int row = (int)(p / n_px), col = (int)(p - (int64_t)row * n_px);
        const double x = ((double)col + 0.5 - half) * step, y = ((double)row + 0.5 - half) * step, J = in[p] - floor_;
        const double ut = tx * x + ty * y, us = tx * y - ty * x;
#pragma unroll
        for (int j = 0; j < OT_PSFF_FREQ_BLOCK; j++) {
            double sn, cs;
            const double pt = nu[j] * ut, ps = nu[j] * us;
            sincospi_small(2.0 * (pt - rint(pt)), &sn, &cs);
            acc[4 * j + 0] += J * cs;
            acc[4 * j + 1] += J * sn;
            sincospi_small(2.0 * (ps - rint(ps)), &sn, &cs);
            acc[4 * j + 2] += J * cs;
            acc[4 * j + 3] += J * sn;
        }
        acc[4 * OT_PSFF_FREQ_BLOCK] += J;
    }
    block_reduce_fixed<OT_PSFF_OTF_M, red_max()>(acc, red);
    __syncthreads();
    const int j = threadIdx.x;
    if (j < OT_PSFF_FREQ_BLOCK && m0 + j < M) {
        double* o = out + (((f * Z + z) * M) + m0 + j) * 6;
        const double ct = red[4 * j], st = red[4 * j + 1], cs = red[4 * j + 2], ss = red[4 * j + 3], j0 = fabs(red[4 * OT_PSFF_FREQ_BLOCK]);
        o[0] = ct;
        o[1] = -st;
        o[2] = cs;
        o[3] = -ss;
        o[4] = ot_sqrt(ct * ct + st * st) / j0;
        o[5] = ot_sqrt(cs * cs + ss * ss) / j0;
    }
}
