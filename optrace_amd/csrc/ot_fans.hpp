// Ray fans of a stored trace (Raytracer.ray_fans): per band of wavelengths the transverse ray aberration and the optical path
// difference against the pupil coordinate, along the tangential and the sagittal cut of the pupil, and the band's own wavefront
// and spot figures.  Definition: DESIGN.md "Ray fans"; the slots of the records: include/optrace_amd.h.
//   transverse  per ray where its line of section k crosses the plane z = focus z, minus the focus: ex, ey; a ray that runs
//               within a plane z = const loses its weight and is counted
//   bands       two passes over the dense planes opl, ex, ey, w, wl per band: sums and extremes, then central sums about the
//               means of the first; workgroup (i, b) walks the rays as workgroup i of gridDim.x and takes those of band b
//               (the grid of ot_chromatic.hpp), a lane reads its ray's key byte first and the other planes for its band only
//   bins        one walk over the rays for all bands: six sums per band, cut and bin of the pupil coordinate (f64 atomics)
// The band passes add in the fixed order of ot_block_reduce.hpp: two calls return the same bits.
// Defines kernels that are no templates: included by ot_fans_api.hip alone.
#pragma once
#include "ot_block_reduce.hpp"
#include "ot_device.hpp"
#include "ot_wavefront_ray.hpp"  // the moments record, the unit-disc coordinates of an entry

// slots of the band record (include/optrace_amd.h, ot_fans_bands): pass 1 carries the first FAN_M1 of them, pass 2 the rest
enum {
    FAN_W = 0, FAN_COUNT, FAN_WOPL, FAN_WEX, FAN_WEY, FAN_WWL, FAN_OPL_MIN, FAN_OPL_MAX, FAN_M1,
    FAN_WOPD2 = FAN_M1, FAN_WDEX2, FAN_WDEY2, FAN_WDEXDEY, FAN_R2MAX, FAN_M
};
#define FAN_M2 (FAN_M - FAN_M1)
// sums of a bin (ot_fans_bins)
enum { FB_W = 0, FB_COUNT, FB_WC, FB_WEX, FB_WEY, FB_WOPD, FB_M };
static_assert(FAN_M == OT_FAN_M && FAN_M1 == 8 && FB_M == OT_FAN_BIN_M, "the records of the header");

// One thread per ray of a launch: p from the launch's first ray on, w, ex and ey from its place in the range, so that n <= 2^28
// rays are addressed with 32-bit offsets.  The six position planes of sections k and k + 1 are read plane by plane (coalesced:
// neighbouring lanes, neighbouring rays) and only by lanes whose ray has a weight.  Rays without one get NaN in ex and ey.
__global__ __launch_bounds__(OT_RED_THREADS) void fan_transverse_kernel(const double* __restrict__ p, int64_t N, int nt, int k, uint32_t n,
                                                                        double fx, double fy, double fz, float* __restrict__ w,
                                                                        double* __restrict__ ex, double* __restrict__ ey,
                                                                        unsigned long long* __restrict__ parallel) {
    const uint32_t r = blockIdx.x * OT_RED_THREADS + threadIdx.x;
    bool flat = false;
    if (r < n) {
        const double nan = __builtin_nan("");
        double exi = nan, eyi = nan;
        if (w[r] > 0.f) {
            const double *x0 = p + N * k, *y0 = p + N * (k + nt), *z0 = p + N * (k + 2 * (int64_t)nt);
            const double *x1 = x0 + N, *y1 = y0 + N, *z1 = z0 + N;
            const double pz = z0[r], dz = z1[r] - pz;
            flat = dz == 0.0;
            if (flat) {
                w[r] = 0.f;
            } else {
                const double px = x0[r], py = y0[r], dx = x1[r] - px, dy = y1[r] - py;
                const double t = (fz - pz) / dz;
                exi = px + t * dx - fx;
                eyi = py + t * dy - fy;
            }
        }
        ex[r] = exi;
        ey[r] = eyi;
    }
    const unsigned long long m = __ballot(flat);
    if (__lane_id() == 0 && m) atomicAdd(parallel, (unsigned long long)__popcll(m));
}

// The dense planes from the first entry of a launch on.  Workgroup-uniform.
struct FanPlanes {
    const uint8_t* key;
    const float *w, *wl;
    const double *opl, *ex, *ey;
};

// part[n_bands][blocks_total][FAN_M1]; this launch fills the workgroups block0 .. block0 + gridDim.x - 1 of every band.  The
// minimum is carried as the maximum of -opl.
__global__ __launch_bounds__(OT_RED_THREADS) void fan_first_kernel(FanPlanes S, uint32_t n, unsigned block0, unsigned blocks_total,
                                                                   double* __restrict__ part) {
    const unsigned b = blockIdx.y;
    const double inf = __builtin_inf();
    double v[FAN_M1] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, -inf, -inf};
    const uint32_t stride = gridDim.x * OT_RED_THREADS;  // (at most 2^18 beyond n <= 2^28: no wrap)
    for (uint32_t r = blockIdx.x * OT_RED_THREADS + threadIdx.x; r < n; r += stride) {
        if (S.key[r] != b) continue;
        const float wi = S.w[r];
        if (!(wi > 0.f)) continue;
        const double wd = (double)wi, l = S.opl[r];
        v[FAN_W] += wd;
        v[FAN_COUNT] += 1.0;  // (exact up to 2^53 rays)
        v[FAN_WOPL] += wd * l;
        v[FAN_WEX] += wd * S.ex[r];
        v[FAN_WEY] += wd * S.ey[r];
        v[FAN_WWL] += wd * (double)S.wl[r];
        v[FAN_OPL_MIN] = fmax(v[FAN_OPL_MIN], -l);
        v[FAN_OPL_MAX] = fmax(v[FAN_OPL_MAX], l);
    }
    block_reduce_fixed<FAN_M1, red_max(FAN_OPL_MIN, FAN_OPL_MAX)>(v, part + ((int64_t)b * blocks_total + block0 + blockIdx.x) * FAN_M1);
}

// part[n_bands][blocks_total][FAN_M2]; rec: the records with the slots of pass 1 in place
__global__ __launch_bounds__(OT_RED_THREADS) void fan_central_kernel(FanPlanes S, uint32_t n, unsigned block0, unsigned blocks_total,
                                                                     const double* __restrict__ rec, double* __restrict__ part) {
    const unsigned b = blockIdx.y;
    const double* m = rec + (int64_t)FAN_M * b;
    // the means: the same three IEEE quotients as the host forms from the record (no ray in the sums: NaN, and nothing reads them)
    const double mo = m[FAN_WOPL] / m[FAN_W], mx = m[FAN_WEX] / m[FAN_W], my = m[FAN_WEY] / m[FAN_W];
    double v[FAN_M2] = {0.0, 0.0, 0.0, 0.0, 0.0};
    const uint32_t stride = gridDim.x * OT_RED_THREADS;
    for (uint32_t r = blockIdx.x * OT_RED_THREADS + threadIdx.x; r < n; r += stride) {
        if (S.key[r] != b) continue;
        const float wi = S.w[r];
        if (!(wi > 0.f)) continue;
        const double wd = (double)wi, d = S.opl[r] - mo, dx = S.ex[r] - mx, dy = S.ey[r] - my;
        v[FAN_WOPD2 - FAN_M1] += wd * (d * d);
        v[FAN_WDEX2 - FAN_M1] += wd * (dx * dx);
        v[FAN_WDEY2 - FAN_M1] += wd * (dy * dy);
        v[FAN_WDEXDEY - FAN_M1] += wd * (dx * dy);
        v[FAN_R2MAX - FAN_M1] = fmax(v[FAN_R2MAX - FAN_M1], dx * dx + dy * dy);
    }
    block_reduce_fixed<FAN_M2, red_max(FAN_R2MAX - FAN_M1)>(v, part + ((int64_t)b * blocks_total + block0 + blockIdx.x) * FAN_M2);
}

// A band without a ray: zeros where the extremes of pass 1 left their starts, and no second moments of the transverse
// aberration -- NaN in place of the zeros that were added up, as ch_finish_kernel (ot_chromatic.hpp) has it.  One thread per band.
__global__ void fan_finish_kernel(int n_bands, double* __restrict__ rec) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= n_bands) return;
    double* m = rec + (int64_t)FAN_M * b;
    if (m[FAN_COUNT] == 0.0) {
        m[FAN_OPL_MIN] = m[FAN_OPL_MAX] = 0.0;
        for (int s = FAN_WDEX2; s <= FAN_WDEXDEY; s++) m[s] = __builtin_nan("");
    }
}

// bin = min(floor((c + 1) / 2 n_bins), n_bins - 1) (c >= -1 up to rounding: a value an ulp outside, or no number at all, must
// not index outside the table; the guards of wf_map_kernel)
OT_DEV int fan_bin(double c, int n_bins) {
    const double fn = (double)n_bins, q = floor((c + 1.0) / 2.0 * fn);
    return !(q >= 0.0) ? 0 : q < fn - 1.0 ? (int)q : n_bins - 1;
}

// the six sums of a bin; t: the bin's slots, in LDS or in global memory (one function, inlined at either kind of address)
OT_DEV void fan_add(double* t, double wd, double c, double exi, double eyi, double opd) {
    unsafeAtomicAdd(t + FB_W, wd);
    unsafeAtomicAdd(t + FB_COUNT, 1.0);
    unsafeAtomicAdd(t + FB_WC, wd * c);
    unsafeAtomicAdd(t + FB_WEX, wd * exi);
    unsafeAtomicAdd(t + FB_WEY, wd * eyi);
    unsafeAtomicAdd(t + FB_WOPD, wd * opd);
}

// out[n_bands][2][n_bins][FB_M] += the sums of the rays of a cut: fan 0 (tangential) takes |x| <= slab and bins y, fan 1
// (sagittal) takes |y| <= slab and bins x.  A lane reads w, u and v, and the other planes only when its ray is in a cut.
// LDS-privatised when the table fits (lds_cells = n_bands 2 n_bins FB_M), flushed with one global atomic per slot that is not
// zero; otherwise global atomics.
__global__ __launch_bounds__(1024) void fan_bins_kernel(int64_t n, const double* __restrict__ u, const double* __restrict__ v,
                                                        const double* __restrict__ opl, const double* __restrict__ ex,
                                                        const double* __restrict__ ey, const float* __restrict__ w,
                                                        const uint8_t* __restrict__ key, const double* __restrict__ mom,
                                                        double pupil_radius, const double* __restrict__ rec, int n_bands, int n_bins,
                                                        double slab, int lds_cells, double* __restrict__ out) {
    extern __shared__ double sh[];  // [lds_cells] sums
    for (int i = threadIdx.x; i < lds_cells; i += blockDim.x) sh[i] = 0.0;
    __syncthreads();
    const WfPupil P = wf_pupil(mom, pupil_radius);
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const float wi = w[i];
        if (!(wi > 0.f)) continue;
        double x, y;
        if (!wf_unit_disc(P, u[i], v[i], &x, &y)) continue;
        const bool tang = fabs(x) <= slab, sagi = fabs(y) <= slab;
        if (!(tang || sagi)) continue;
        const int b = key[i];
        if (b >= n_bands) continue;
        // (the band's mean path: the same IEEE quotient as the host forms from the record)
        const double mean = rec[FAN_M * b + FAN_WOPL] / rec[FAN_M * b + FAN_W];
        const double wd = (double)wi, exi = ex[i], eyi = ey[i], opd = opl[i] - mean;
        const int at_t = ((b * 2 + 0) * n_bins + fan_bin(y, n_bins)) * FB_M, at_s = ((b * 2 + 1) * n_bins + fan_bin(x, n_bins)) * FB_M;
        if (lds_cells) {
            if (tang) fan_add(&sh[at_t], wd, y, exi, eyi, opd);
            if (sagi) fan_add(&sh[at_s], wd, x, exi, eyi, opd);
        } else {
            if (tang) fan_add(&out[at_t], wd, y, exi, eyi, opd);
            if (sagi) fan_add(&out[at_s], wd, x, exi, eyi, opd);
        }
    }
    if (lds_cells) {
        __syncthreads();
        for (int i = threadIdx.x; i < lds_cells; i += blockDim.x) {
            const double s = sh[i];
            if (s != 0.0) unsafeAtomicAdd(&out[i], s);
        }
    }
}
