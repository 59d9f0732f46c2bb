// Wavefront analysis of a traced bundle (Raytracer.wavefront_analysis): optical path to a reference sphere, its moments, a pupil
// map and the normal equations of a Zernike fit, from the ray storage's planes.  Definition: DESIGN.md "Wavefront analysis".
//   focus    sums for the point closest to all ray lines of section k and for the bundle's mean start and direction
//   paths    per ray OPL = sum_{j<k} n_j |p_{j+1} - p_j| + n_k t to the sphere (centre c, signed radius R) and the pupil
//            coordinates (u, v) of the intersection: four dense planes, w_out = 0 for rays that are not used
//   moments  two passes over those planes: sums, then central sums about the means of the first
//   map      sum w and sum w OPD per cell of an n_grid x n_grid pupil grid (f64 atomics)
//   zernike  G = sum w Z Z^T (upper triangle) and g = sum w Z OPD for the Noll polynomials Z_1 .. Z_J
// focus, moments and zernike add in the fixed order of ot_block_reduce.hpp and a last kernel over the workgroups' partials
// (its reduce_final_kernel; wf_zernike_final_kernel): two calls return the same bits.  Every pass reads the results of those
// before it from device memory.
// Defines kernels that are no templates: included by ot_wavefront_api.hip alone.
#pragma once
#include "ot_block_reduce.hpp"
#include "ot_device.hpp"
#include "ot_hit_list.hpp"       // dense_for_each: the walk of the planes
#include "ot_wavefront_ray.hpp"  // the rays of a section, their sphere step, the slots of the records

// part[gridDim.x][17]: W | count | sum w (p - origin) | sum w s | sum w (I - s s^T): xx xy xz yy yz zz | sum w (I - s s^T) (p - origin)
__global__ __launch_bounds__(OT_RED_THREADS) void wf_focus_kernel(ot_rays R, int64_t first, int64_t count, int k, double ox, double oy,
                                                                  double oz, double* __restrict__ part) {
    double v[WFF_M];
#pragma unroll
    for (int m = 0; m < WFF_M; m++) v[m] = 0.0;
    dense_for_each(count, [&](int64_t i) {
        const int64_t r = first + i;
        const WfRay q = wf_section(R, r, k, wf_position(R, r, k));
        if (!q.used) return;
        const double w = q.w, px = q.p.x - ox, py = q.p.y - oy, pz = q.p.z - oz;
        const V3 s = q.s;
        const double sp = s.x * px + s.y * py + s.z * pz;
        v[WFF_W] += w;
        v[WFF_COUNT] += 1.0;
        v[WFF_P + 0] += w * px;
        v[WFF_P + 1] += w * py;
        v[WFF_P + 2] += w * pz;
        v[WFF_S + 0] += w * s.x;
        v[WFF_S + 1] += w * s.y;
        v[WFF_S + 2] += w * s.z;
        v[WFF_A + 0] += w * (1.0 - s.x * s.x);
        v[WFF_A + 1] -= w * (s.x * s.y);
        v[WFF_A + 2] -= w * (s.x * s.z);
        v[WFF_A + 3] += w * (1.0 - s.y * s.y);
        v[WFF_A + 4] -= w * (s.y * s.z);
        v[WFF_A + 5] += w * (1.0 - s.z * s.z);
        v[WFF_B + 0] += w * (px - s.x * sp);
        v[WFF_B + 1] += w * (py - s.y * sp);
        v[WFF_B + 2] += w * (pz - s.z * sp);
    });
    block_reduce_fixed<WFF_M, red_max()>(v, part + WFF_M * (int64_t)blockIdx.x);
}

// The hot pass, one thread per ray of [first, first + count): (k + 2) positions and (k + 1) indices read plane by plane
// (coalesced: neighbouring lanes, neighbouring rays), four dense planes written.  Rays that are not used leave NaN in u, v and
// opl and 0 in w_out; those whose line misses the sphere are counted in `missed` besides.
__global__ __launch_bounds__(OT_RED_THREADS) void wf_paths_kernel(ot_rays R, int64_t first, int64_t count, int k, double cx, double cy,
                                                                  double cz, double radius, double* __restrict__ u, double* __restrict__ v,
                                                                  double* __restrict__ opl, float* __restrict__ w_out,
                                                                  unsigned long long* __restrict__ missed) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    bool miss = false;
    if (i < count) {
        double ui, vi, li;
        float wi;
        const int64_t r = first + i;
        miss = wf_path(R, r, k, cx, cy, cz, radius, ui, vi, li, wi);
        u[i] = ui;
        v[i] = vi;
        opl[i] = li;
        w_out[i] = wi;
    }
    const unsigned long long m = __ballot(miss);
    if (__lane_id() == 0 && m) atomicAdd(missed, (unsigned long long)__popcll(m));
}

// ---- moments of the planes -------------------------------------------------------------------------------------------
// part[gridDim.x][8]: the first eight slots of the record, the minimum as the maximum of -opl
__global__ __launch_bounds__(OT_RED_THREADS) void wf_first_kernel(int64_t n, const double* __restrict__ u, const double* __restrict__ v,
                                                                  const double* __restrict__ opl, const float* __restrict__ w,
                                                                  const float* __restrict__ wl, double* __restrict__ part) {
    const double inf = __builtin_inf();
    double a[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -inf, -inf};
    dense_for_each(n, [&](int64_t i) {
        const float wi = w[i];
        if (!(wi > 0.f)) return;
        const double wd = (double)wi, l = opl[i];
        a[WF_W] += wd;
        a[WF_COUNT] += 1.0;
        a[WF_WOPL] += wd * l;
        a[WF_WU] += wd * u[i];
        a[WF_WV] += wd * v[i];
        if (wl) a[WF_WWL] += wd * (double)wl[i];
        a[WF_OPL_MIN] = fmax(a[WF_OPL_MIN], -l);
        a[WF_OPL_MAX] = fmax(a[WF_OPL_MAX], l);
    });
    block_reduce_fixed<8, red_max(WF_OPL_MIN, WF_OPL_MAX)>(a, part + 8 * (int64_t)blockIdx.x);
}

// part[gridDim.x][2]: sum w opd^2 | max (du^2 + dv^2)
__global__ __launch_bounds__(OT_RED_THREADS) void wf_central_kernel(int64_t n, const double* __restrict__ u, const double* __restrict__ v,
                                                                    const double* __restrict__ opl, const float* __restrict__ w,
                                                                    const double* __restrict__ mom, double* __restrict__ part) {
    const WfMeans c = wf_means(mom);
    double a[2] = {0.0, 0.0};
    dense_for_each(n, [&](int64_t i) {
        const float wi = w[i];
        if (!(wi > 0.f)) return;
        const double d = opl[i] - c.opl, du = u[i] - c.u, dv = v[i] - c.v;
        a[0] += (double)wi * (d * d);
        a[1] = fmax(a[1], du * du + dv * dv);
    });
    block_reduce_fixed<2, red_max(1)>(a, part + 2 * (int64_t)blockIdx.x);
}

// The pupil radius the later passes divide by when the caller gives none, stored so that the host reports this very number
__global__ void wf_pupil_radius_kernel(double* __restrict__ mom) { mom[WF_PUPIL_R] = ot_sqrt(mom[WF_R2MAX]); }

// (the unit-disc coordinates of an entry, wf_pupil and wf_unit_disc: ot_wavefront_ray.hpp)

// map[2][n_grid][n_grid] += w | w opd, row = cell of y, column = cell of x, cell = min(floor((x + 1) / 2 n_grid), n_grid - 1).
// LDS-privatised when the sums fit (lds_cells = 2 n_grid^2), otherwise global atomics.
__global__ __launch_bounds__(1024) void wf_map_kernel(int64_t n, const double* __restrict__ u, const double* __restrict__ v,
                                                      const double* __restrict__ opl, const float* __restrict__ w,
                                                      const double* __restrict__ mom, double pupil_radius, int n_grid, int lds_cells,
                                                      double* __restrict__ map) {
    extern __shared__ double sh[];  // [lds_cells] sums
    if (lds_cells) {
        for (int i = threadIdx.x; i < lds_cells; i += blockDim.x) sh[i] = 0.0;
        __syncthreads();
    }
    const WfPupil P = wf_pupil(mom, pupil_radius);
    const double mean = wf_means(mom).opl, fn = (double)n_grid;
    const int64_t cells = (int64_t)n_grid * n_grid;
    // (dense_for_each written out: through it the selects of the cell index compile to branches; profiles/analysis_core)
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float wi = w[i];
        if (!(wi > 0.f)) continue;
        double x, y;
        if (!wf_unit_disc(P, u[i], v[i], &x, &y)) continue;
        const double qx = floor((x + 1.0) / 2.0 * fn), qy = floor((y + 1.0) / 2.0 * fn);
        // (x >= -1 up to rounding: a value an ulp outside, or no number at all, must not index outside the map)
        const int ix = !(qx >= 0.0) ? 0 : qx < fn - 1.0 ? (int)qx : n_grid - 1;
        const int iy = !(qy >= 0.0) ? 0 : qy < fn - 1.0 ? (int)qy : n_grid - 1;
        const int64_t cell = (int64_t)iy * n_grid + ix;
        const double wd = (double)wi, wo = wd * (opl[i] - mean);
        if (lds_cells) {
            unsafeAtomicAdd(&sh[cell], wd);
            unsafeAtomicAdd(&sh[cells + cell], wo);
        } else {
            unsafeAtomicAdd(&map[cell], wd);
            unsafeAtomicAdd(&map[cells + cell], wo);
        }
    }
    if (lds_cells) {
        __syncthreads();
        for (int i = threadIdx.x; i < lds_cells; i += blockDim.x) {
            const double s = sh[i];
            if (s != 0.0) unsafeAtomicAdd(&map[i], s);
        }
    }
}

// (the Zernike polynomials in Noll's order, wf_zernike_all: ot_wavefront_ray.hpp)

// Normal equations for the first JT polynomials, JT the table size at or above the caller's J.  Workgroup (bx, c) walks the list
// as workgroup bx of gridDim.x for chunk c < (JT + 1) / 2: rows a = c and b = JT - 1 - c of the upper triangle, JT + 1 entries of
// G between them, and their two entries of g.  Slot s of the JT + 3 accumulators per lane:
//   s >= c      G[a][s]             s < c   G[b][JT - 1 - s]          s = JT  G[b][b]       JT + 1, JT + 2   g[a], g[b]
// (a = b in the middle chunk of an odd JT: its slots s < c, JT and JT + 2 repeat others of the chunk and are dropped).  Every Z index but
// a and b is a compile-time one, so Z and the accumulators stay in registers.  part[gridDim.x][gridDim.y][JT + 3].
template <int JT>
__global__ __launch_bounds__(OT_RED_THREADS) void wf_zernike_kernel(int64_t n, const double* __restrict__ u, const double* __restrict__ v,
                                                                    const double* __restrict__ opl, const float* __restrict__ w,
                                                                    const double* __restrict__ mom, double pupil_radius,
                                                                    double* __restrict__ part) {
    constexpr int S = JT + 3;
    const WfPupil P = wf_pupil(mom, pupil_radius);
    const double mean = wf_means(mom).opl;
    const int c = blockIdx.y;
    double acc[S];
#pragma unroll
    for (int s = 0; s < S; s++) acc[s] = 0.0;
    // (dense_for_each written out: through it the JT = 15 kernel's scalar-register spills move by two; profiles/analysis_core)
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float wi = w[i];
        if (!(wi > 0.f)) continue;
        double x, y;
        if (!wf_unit_disc(P, u[i], v[i], &x, &y)) continue;
        double Z[JT];
        wf_zernike_all<JT>(x, y, Z);
        double za = Z[0], zb = Z[JT - 1];
#pragma unroll
        for (int s = 1; s < (JT + 1) / 2; s++) {  // (wave-uniform selects)
            za = s == c ? Z[s] : za;
            zb = s == c ? Z[JT - 1 - s] : zb;
        }
        const double wd = (double)wi, wa = wd * za, wb = wd * zb;
#pragma unroll
        for (int s = 0; s < JT; s++) acc[s] += s >= c ? wa * Z[s] : wb * Z[JT - 1 - s];
        acc[JT] += wb * zb;
        const double opd = opl[i] - mean;
        acc[JT + 1] += wa * opd;
        acc[JT + 2] += wb * opd;
    }
    block_reduce_fixed<S, red_max()>(acc, part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * S);
}

// part[nblocks][chunks][JT + 3] -> out: G's upper triangle row by row (i <= j < J), then g[J].  One thread per slot of a chunk
// adds its partials in index order and stores the sum where its (i, j) belongs, if that lies within J.
__global__ __launch_bounds__(OT_RED_THREADS) void wf_zernike_final_kernel(const double* __restrict__ part, int nblocks, int JT, int J,
                                                                          double* __restrict__ out) {
    const int S = JT + 3, chunks = (JT + 1) / 2;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= chunks * S) return;
    const int c = q / S, s = q % S, a = c, b = JT - 1 - c;
    int i, j;  // j = -1: an entry of g
    if (s < JT) {
        i = s >= c ? a : b;
        j = s >= c ? s : JT - 1 - s;
    } else if (s == JT) {
        i = j = b;
    } else {
        i = s == JT + 1 ? a : b;
        j = -1;
    }
    if (a == b && (s < c || s == JT || s == JT + 2)) return;  // the middle chunk's repeats
    if (i >= J || j >= J) return;
    double r = 0.0;
    for (int k = 0; k < nblocks; k++) r += part[((int64_t)k * chunks + c) * S + s];
    const int tri = J * (J + 1) / 2;
    out[j < 0 ? tri + i : i * J - i * (i - 1) / 2 + (j - i)] = r;
}
