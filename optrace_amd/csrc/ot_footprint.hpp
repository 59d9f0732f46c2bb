// Beam footprints of a stored trace (Raytracer.footprints): per section of the ray storage the living and the arriving rays, their
// power, and where the living ones cross the surface -- centroid, extent, second moments, largest distance from the surface's axis
// -- and optionally a power map.  Definition: DESIGN.md "Footprints"; the record's slots: include/optrace_amd.h.
//   pass 1  over T = {w[i] > 0} and A = {w[i - 1] > 0} (A = T in section 0): sum w, counts, sum w p, the extremes of p
//   pass 2  about the centroid c of pass 1, d = (x, y) - c formed before squaring: sum w dx^2, sum w dy^2, sum w dx dy, and the
//           largest squared distance from the axis
//   maps    sum w per cell of an n_px x n_px grid over axis +- sqrt(slot 16)  (f64 atomics)
// All sections go in one launch: workgroup (b, i) walks section i as workgroup b of gridDim.x.  A plane of one section is
// contiguous, lanes read neighbouring rays; the positions are loaded by living lanes only, so a wave without a living ray (behind
// an aperture, in the last section) touches no position line.  Passes 1 and 2 add in the fixed order of ot_block_reduce.hpp.  The
// arriving sums of section i and the living sums of section i - 1 are the same additions over the same plane in the same
// order: they agree bit for bit.
// Defines kernels that are no templates: included by ot_footprint_api.hip alone.
#pragma once
#include "ot_block_reduce.hpp"
#include "ot_device.hpp"

// slots of the record (include/optrace_amd.h, ot_footprint_moments); pass 1 carries the first FP_M1 of them, the minima negated
enum {
    FP_W = 0, FP_COUNT, FP_W_IN, FP_COUNT_IN, FP_WX, FP_WY, FP_WZ, FP_XMIN, FP_XMAX, FP_YMIN, FP_YMAX, FP_ZMIN, FP_ZMAX,
    FP_M1, FP_WDX2 = FP_M1, FP_WDY2, FP_WDXDY, FP_R2MAX, FP_M
};
static_assert(FP_M == OT_FP_M && FP_M1 == 13, "the record of the header");
#define FP_M2 (FP_M - FP_M1)

// The planes of one section from the first ray of a launch on: the host has added that ray's index to p and w, so that n <= 2^28
// rays are addressed with 32-bit offsets.  Workgroup-uniform.
struct FpSection {
    const float *w, *w_in;
    const double *x, *y, *z;
};
OT_DEV FpSection fp_section(const double* __restrict__ p, const float* __restrict__ w, int64_t N, int nt, int i) {
    return {w + N * i, w + N * (i > 0 ? i - 1 : 0), p + N * i, p + N * (i + nt), p + N * (i + 2 * (int64_t)nt)};
}

// part[nt][blocks_total][FP_M1]; this launch fills the workgroups block0 .. block0 + gridDim.x - 1 of every section
__global__ __launch_bounds__(OT_RED_THREADS) void fp_first_kernel(const double* __restrict__ p, const float* __restrict__ w, int64_t N,
                                                                  int nt, uint32_t n, unsigned block0, unsigned blocks_total,
                                                                  double* __restrict__ part) {
    const int i = blockIdx.y;
    const FpSection S = fp_section(p, w, N, nt, i);
    const double inf = __builtin_inf();
    double v[FP_M1] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -inf, -inf, -inf, -inf, -inf, -inf};
    const uint32_t stride = gridDim.x * OT_RED_THREADS;  // (at most 2^18 beyond n <= 2^28: no wrap)
    for (uint32_t r = blockIdx.x * OT_RED_THREADS + threadIdx.x; r < n; r += stride) {
        const float wi = S.w[r], wa = S.w_in[r];
        if (wa > 0.f) {
            v[FP_W_IN] += (double)wa;
            v[FP_COUNT_IN] += 1.0;  // (exact up to 2^53 rays)
        }
        if (wi > 0.f) {
            const double wd = (double)wi, x = S.x[r], y = S.y[r], z = S.z[r];
            v[FP_W] += wd;
            v[FP_COUNT] += 1.0;
            v[FP_WX] += wd * x;
            v[FP_WY] += wd * y;
            v[FP_WZ] += wd * z;
            v[FP_XMIN] = fmax(v[FP_XMIN], -x);
            v[FP_XMAX] = fmax(v[FP_XMAX], x);
            v[FP_YMIN] = fmax(v[FP_YMIN], -y);
            v[FP_YMAX] = fmax(v[FP_YMAX], y);
            v[FP_ZMIN] = fmax(v[FP_ZMIN], -z);
            v[FP_ZMAX] = fmax(v[FP_ZMAX], z);
        }
    }
    block_reduce_fixed<FP_M1, red_max_range(FP_XMIN, FP_M1)>(v, part + ((int64_t)i * blocks_total + block0 + blockIdx.x) * FP_M1);
}

// part[nt][blocks_total][FP_M2]; rec: the records with the slots of pass 1 in place
__global__ __launch_bounds__(OT_RED_THREADS) void fp_central_kernel(const double* __restrict__ p, const float* __restrict__ w, int64_t N,
                                                                    int nt, uint32_t n, unsigned block0, unsigned blocks_total,
                                                                    const double* __restrict__ axis, const double* __restrict__ rec,
                                                                    double* __restrict__ part) {
    const int i = blockIdx.y;
    const FpSection S = fp_section(p, w, N, nt, i);
    const double* m = rec + (int64_t)FP_M * i;
    // the centroid: the same two IEEE quotients as the host forms from the record (no living ray: NaN, and nothing reads it)
    const double cx = m[FP_WX] / m[FP_W], cy = m[FP_WY] / m[FP_W], ax = axis[2 * i], ay = axis[2 * i + 1];
    double v[FP_M2] = {0.0, 0.0, 0.0, 0.0};
    const uint32_t stride = gridDim.x * OT_RED_THREADS;
    for (uint32_t r = blockIdx.x * OT_RED_THREADS + threadIdx.x; r < n; r += stride) {
        const float wi = S.w[r];
        if (!(wi > 0.f)) continue;
        const double wd = (double)wi, x = S.x[r], y = S.y[r], dx = x - cx, dy = y - cy, ux = x - ax, uy = y - ay;
        v[FP_WDX2 - FP_M1] += wd * (dx * dx);
        v[FP_WDY2 - FP_M1] += wd * (dy * dy);
        v[FP_WDXDY - FP_M1] += wd * (dx * dy);
        v[FP_R2MAX - FP_M1] = fmax(v[FP_R2MAX - FP_M1], ux * ux + uy * uy);
    }
    block_reduce_fixed<FP_M2, red_max(FP_R2MAX - FP_M1)>(v, part + ((int64_t)i * blocks_total + block0 + blockIdx.x) * FP_M2);
}

// A section without a living ray has no extremes: NaN in place of the +-inf the fold started from.  One thread per section.
__global__ void fp_finish_kernel(int nt, double* __restrict__ rec) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nt) return;
    double* m = rec + (int64_t)FP_M * i;
    if (m[FP_COUNT] == 0.0)
        for (int s = FP_XMIN; s <= FP_ZMAX; s++) m[s] = __builtin_nan("");
}

// maps[nt][n_px][n_px] += w, row from y and column from x by min(floor(((x - ax) + R) / (2 R) n_px), n_px - 1), R = sqrt(slot 16) of
// the section's record; cell 0, 0 when R = 0.  LDS-privatised when the cells fit (lds_cells = n_px^2), otherwise global atomics.
__global__ __launch_bounds__(1024) void fp_map_kernel(const double* __restrict__ p, const float* __restrict__ w, int64_t N, int nt, uint32_t n,
                                                      const double* __restrict__ axis, const double* __restrict__ rec, int n_px,
                                                      int lds_cells, double* __restrict__ maps) {
    extern __shared__ double sh[];  // [lds_cells] sums
    const int i = blockIdx.y;
    const int cells = n_px * n_px;
    double* map = maps + (int64_t)cells * i;
    const double R = __builtin_sqrt(rec[(int64_t)FP_M * i + FP_R2MAX]);
    if (rec[(int64_t)FP_M * i + FP_COUNT] == 0.0) return;  // (workgroup-uniform: nothing to add, nothing to flush)
    if (lds_cells) {
        for (int c = threadIdx.x; c < lds_cells; c += blockDim.x) sh[c] = 0.0;
        __syncthreads();
    }
    const FpSection S = fp_section(p, w, N, nt, i);
    const double ax = axis[2 * i], ay = axis[2 * i + 1], fn = (double)n_px, two_R = 2.0 * R;
    const uint32_t stride = gridDim.x * blockDim.x;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n; r += stride) {
        const float wi = S.w[r];
        if (!(wi > 0.f)) continue;
        int ix = 0, iy = 0;
        if (R > 0.0) {
            const double qx = floor(((S.x[r] - ax) + R) / two_R * fn), qy = floor(((S.y[r] - ay) + R) / two_R * fn);
            // (|x - ax| <= R up to the rounding of the root: a value an ulp outside, or no number at all, must not index outside the map)
            ix = !(qx >= 0.0) ? 0 : qx < fn - 1.0 ? (int)qx : n_px - 1;
            iy = !(qy >= 0.0) ? 0 : qy < fn - 1.0 ? (int)qy : n_px - 1;
        }
        const int cell = iy * n_px + ix;
        if (lds_cells)
            unsafeAtomicAdd(&sh[cell], (double)wi);
        else
            unsafeAtomicAdd(&map[cell], (double)wi);
    }
    if (lds_cells) {
        __syncthreads();
        for (int c = threadIdx.x; c < lds_cells; c += blockDim.x) {
            const double s = sh[c];
            if (s != 0.0) unsafeAtomicAdd(&map[c], s);
        }
    }
}
