// Sampler stage: the sampling helpers of optrace/tracer/random.py, Surface.random_positions and
// color.random_wavelengths_from_srgb (srgb.py:513-553) as kernels of their own, behind ot.random and the random_positions of
// the source shapes.  One lane per sample, struct-of-arrays float64 outputs.
//
// Nothing is sampled here: every kernel fills a GenCtx the way the generation kernel does (ot_trace_kernel.hpp::generate_lane --
// seed, global index as the Philox counter, index / count / id of the sample's range, the host's per-range constants) and calls
// the generator's own strat_interval / strat_rect / strat_ring / inv_cdf_discrete / inv_cdf_linear (ot_generate.hpp), with the
// stream and the dither block the generator uses for that quantity.  A position drawn here is therefore the start position
// the generator gives the ray with the same (seed, ranges, index).
// What is written out a second time, because ot_generate.hpp stays as it is: the mapping of a sample onto the source shape
// (generate_ray, "start position") and the placing of a wavelength inside an sRGB primary (generate_ray, OT_SRC_IMAGE_RGB).
// Defines kernels that are no templates: included by ot_sample_api.hip alone.
#pragma once
#include "ot_color_px.hpp"
#include "ot_trace_kernel.hpp"

struct StratArgs {
    int32_t kind, flag;  // OT_SAMPLE_*; interval: shuffle, ring: polar
    double a, b, c, d;   // interval [a, b]; rectangle [a, b] x [c, d]; ring: a = ri, b = r
};

struct ShapeArgs {  // the shape fields of an ot_source, rotation as cos / sin like SourceDev
    int32_t shape, _pad;
    double pos[3], r, ri, dim[2], ca, sa;
};

// -> false for an index no range covers
OT_DEV bool sample_ctx(const RangeArgs& rg, int64_t i, uint64_t seed, GenCtx& g) {
    g.seed = seed;
    g.gidx = (uint64_t)i;
    int k = -1, src = 0;
    if (!locate_range(rg, i, g, k, src)) return false;
    g.range = (uint32_t)k;
    return true;
}

// random.stratified_interval_sampling / _rectangle_sampling / _ring_sampling
__global__ __launch_bounds__(256) void sample_stratified_kernel(StratArgs A, RangeArgs rg, uint64_t seed, int64_t n,
                                                                double* __restrict__ out0, double* __restrict__ out1) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    GenCtx g;
    if (!sample_ctx(rg, i, seed, g)) return;
    fill_dither(g, true, false);  // ST_POS reads block B
    if (A.kind == OT_SAMPLE_INTERVAL) {
        // shuffle off: the identity instead of the keyed permutation (the reference's result is ascending, random.py:63-66)
        out0[i] = A.flag ? strat_interval(g, ST_POS, A.a, A.b) : strat_interval_at(g, g.j, ST_POS, A.a, A.b);
        return;
    }
    double o0, o1;
    if (A.kind == OT_SAMPLE_RECTANGLE) {
        strat_rect(g, ST_POS, A.a, A.b, A.c, A.d, o0, o1);
    } else {
        strat_ring(g, ST_POS, A.a, A.b, A.flag != 0, o0, o1);
        if (A.flag) o1 *= M_PI;  // strat_ring gives theta / pi
    }
    out0[i] = o0;
    out1[i] = o1;
}

// Point / Line / CircularSurface / RingSurface / RectangularSurface .random_positions: generate_ray's start position
__global__ __launch_bounds__(256) void sample_positions_kernel(ShapeArgs S, RangeArgs rg, uint64_t seed, int64_t n,
                                                               double* __restrict__ p) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    GenCtx g;
    if (!sample_ctx(rg, i, seed, g)) return;
    fill_dither(g, true, false);
    double px = S.pos[0], py = S.pos[1];
    switch (S.shape) {
        case OT_SRC_POINT: break;
        case OT_SRC_LINE: {
            double t = strat_interval(g, ST_POS, -S.r, S.r);
            px += S.ca * t;
            py += S.sa * t;
            break;
        }
        case OT_SRC_CIRCLE:
        case OT_SRC_RING: {
            double x, y;
            strat_ring(g, ST_POS, S.shape == OT_SRC_RING ? S.ri : 0.0, S.r, false, x, y);
            px += x;
            py += y;
            break;
        }
        default: {  // OT_SRC_RECT
            double x, y;
            strat_rect(g, ST_POS, -S.dim[0] / 2, S.dim[0] / 2, -S.dim[1] / 2, S.dim[1] / 2, x, y);
            px += x * S.ca - y * S.sa;
            py += x * S.sa + y * S.ca;
        }
    }
    p[i] = px;
    p[i + n] = py;
    p[i + 2 * n] = S.pos[2];
}

// random.inverse_transform_sampling.  discrete: tab = x[m] | F[m] (entries with f > 0, F their running sum); continuous:
// tab = (F_j, x_j) pairs of the cumulative trapezoid.  total = F[m - 1].  S: the caller's uniform variable in [0, 1], or
// nullptr: stratified over the ranges (the generator's wavelength stream)
__global__ __launch_bounds__(256) void sample_inverse_kernel(const double* __restrict__ tab, int m, int kind, CdfGuide G,
                                                             double total, const double* __restrict__ S, RangeArgs rg,
                                                             uint64_t seed, int64_t n, double* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double X;
    if (S) {
        X = total * S[i];  // random.py:146, 157 (F[0] = 0 in both kinds)
    } else {
        GenCtx g;
        if (!sample_ctx(rg, i, seed, g)) return;
        fill_dither(g, false, false);  // ST_WL reads block A
        X = strat_interval(g, ST_WL, 0.0, total);
    }
    out[i] = (kind == OT_SAMPLE_DISCRETE) ? inv_cdf_discrete(tab, m, X, G) : inv_cdf_linear(tab, m, X, G);
}

// color.random_wavelengths_from_srgb srgb.py:513-553: the mix of the three primaries from the row's linear sRGB values, the
// primary from a variable stratified over the rows of the range, the wavelength inside the primary from that variable
// rescaled (as generate_ray does for the pixels of an RGB image; prim_inv: SourceDev::prim_inv)
__global__ __launch_bounds__(256) void sample_srgb_kernel(const double* __restrict__ rgb, const double* __restrict__ prim_inv,
                                                          RangeArgs rg, uint64_t seed, int64_t n, double* __restrict__ wl) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    GenCtx g;
    if (!sample_ctx(rg, i, seed, g)) return;
    fill_dither(g, false, true);  // ST_RGB_CHOICE: a 16-bit dither out of block A, as for image sources
    const double fr = 0.885651229244, fb = 0.775993481741;  // srgb.py:24-26
    const double r = srgb_inverse_gamma(rgb[3 * i]) * fr;
    const double gr = srgb_inverse_gamma(rgb[3 * i + 1]);
    const double b = srgb_inverse_gamma(rgb[3 * i + 2]) * fb;
    const double c0 = r, c1 = r + gr, c2 = r + gr + b;
    const double den = (c2 != 0.0) ? c2 : 1.0;
    const double c_r = ot_div(c0, den), c_rg = ot_div(c1, den);
    const double choice = strat_interval(g, ST_RGB_CHOICE, 0.0, 1.0);
    // (a black row: c_r = c_rg = 0, blue -- also for a choice of exactly 0, which the reference's `choice > 0` sends to green
    // once in 2^53 draws and a 16-bit dither would once in 2^16)
    const int prim = (choice < c_r) ? 0 : ((choice > c_rg || c2 == 0.0) ? 2 : 1);
    const double lo = (prim == 0) ? 0.0 : ((prim == 1) ? c_r : c_rg);
    const double hi = (prim == 0) ? c_r : ((prim == 1) ? c_rg : 1.0);
    const double t = (hi > lo) ? ot_div(choice - lo, hi - lo) : 0.5;
    const double tm = t * (double)OT_PRIM_M;
    int m = (int)tm;
    m = m < 0 ? 0 : (m > OT_PRIM_M - 1 ? OT_PRIM_M - 1 : m);
    const double* inv = prim_inv + (size_t)prim * (OT_PRIM_M + 1) + m;
    const double x0 = inv[0], x1 = inv[1];
    wl[i] = x0 + (tm - (double)m) * (x1 - x0);
}
