// Spot analysis of a hit list (Raytracer.spot_analysis): weighted moments, radial histogram and the geometric OTF of the
// hits of one detector.  Entries are x, y (f64 planes) and w (f32), dense or compact (ot_hit_list.hpp); an entry counts
// when w > 0, and the positions of the others are never read into arithmetic (they may hold anything).
//   pass 1  sum w, sum w x, sum w y, count
//   pass 2  about the centroid c of pass 1, d = p - c formed before squaring: sum w dx^2, sum w dy^2, sum w dx dy, max r^2
//   pass 3  sum w per radial bin min(floor(r / r_max * n_radii), n_radii - 1)
//   pass 4  sum w exp(-2 pi i nu d) for K frequencies and both axes
// Passes 1, 2 and 4 add in the fixed order of ot_block_reduce.hpp -- lane accumulators over the walk, the workgroup's fold, one
// partial per workgroup, a last kernel over the partials (reduce_final_kernel for the moments) -- so two calls return the
// same bits.  Pass 3 adds with f64 atomics.  Every pass reads the results of those before it from device memory: nothing
// comes back to the host in between.
// Defines kernels that are no templates: included by ot_spot_api.hip alone.
#pragma once
#include "ot_block_reduce.hpp"
#include "ot_device.hpp"
#include "ot_hit_list.hpp"

#define OT_SPOT_CHUNK 8  // frequencies per workgroup of pass 4: 32 f64 accumulators per lane
// slots of the moments record (include/optrace_amd.h, ot_spot_moments)
enum { SPOT_W = 0, SPOT_WX, SPOT_WY, SPOT_COUNT, SPOT_WDX2, SPOT_WDY2, SPOT_WDXDY, SPOT_R2MAX, SPOT_M };

// part[gridDim.x][4]
__global__ __launch_bounds__(OT_RED_THREADS) void spot_first_kernel(int64_t n, const double* __restrict__ x, const double* __restrict__ y,
                                                                    const float* __restrict__ w, const unsigned int* __restrict__ fill,
                                                                    double* __restrict__ part) {
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    hit_list_for_each(n, fill, [&](int64_t i) {
        const float wi = w[i];
        if (!(wi > 0.f)) return;
        const double wd = (double)wi;
        v[0] += wd;
        v[1] += wd * x[i];
        v[2] += wd * y[i];
        v[3] += 1.0;  // (exact up to 2^53 hits)
    });
    block_reduce_fixed<4, red_max()>(v, part + 4 * (int64_t)blockIdx.x);
}

// the centroid every later pass subtracts: the same two IEEE quotients as the host forms from the record
struct SpotCentre {
    double x, y;
};
OT_DEV SpotCentre spot_centre(const double* __restrict__ mom) { return {mom[SPOT_WX] / mom[SPOT_W], mom[SPOT_WY] / mom[SPOT_W]}; }

// part[gridDim.x][4]
__global__ __launch_bounds__(OT_RED_THREADS) void spot_central_kernel(int64_t n, const double* __restrict__ x, const double* __restrict__ y,
                                                                      const float* __restrict__ w, const unsigned int* __restrict__ fill,
                                                                      const double* __restrict__ mom, double* __restrict__ part) {
    const SpotCentre c = spot_centre(mom);
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    hit_list_for_each(n, fill, [&](int64_t i) {
        const float wi = w[i];
        if (!(wi > 0.f)) return;
        const double wd = (double)wi, dx = x[i] - c.x, dy = y[i] - c.y;
        v[0] += wd * (dx * dx);
        v[1] += wd * (dy * dy);
        v[2] += wd * (dx * dy);
        v[3] = fmax(v[3], dx * dx + dy * dy);
    });
    block_reduce_fixed<4, red_max(3)>(v, part + 4 * (int64_t)blockIdx.x);
}

// pass 3: hist[n_radii] += w.  LDS-privatised when the bins fit (lds_bins > 0), otherwise global atomics.
__global__ __launch_bounds__(1024) void spot_radial_kernel(int64_t n, const double* __restrict__ x, const double* __restrict__ y,
                                                           const float* __restrict__ w, const unsigned int* __restrict__ fill,
                                                           const double* __restrict__ mom, int n_radii, int lds_bins,
                                                           double* __restrict__ hist) {
    extern __shared__ double sh[];  // [lds_bins] sums
    if (lds_bins) {
        for (int i = threadIdx.x; i < lds_bins; i += blockDim.x) sh[i] = 0.0;
        __syncthreads();
    }
    const SpotCentre c = spot_centre(mom);
    const double r_max = __builtin_sqrt(mom[SPOT_R2MAX]);
    const double fn = (double)n_radii;
    hit_list_for_each(n, fill, [&](int64_t i) {
        const float wi = w[i];
        if (!(wi > 0.f)) return;
        const double dx = x[i] - c.x, dy = y[i] - c.y;
        const double r = __builtin_sqrt(dx * dx + dy * dy);
        int idx = 0;  // (all hits in one place: r_max = 0, everything in the first bin)
        if (r_max > 0.0) {
            const double q = floor(r / r_max * fn);
            idx = q < fn - 1.0 ? (int)q : n_radii - 1;
        }
        if (lds_bins)
            unsafeAtomicAdd(&sh[idx], (double)wi);
        else
            unsafeAtomicAdd(&hist[idx], (double)wi);
    });
    if (lds_bins) {
        __syncthreads();
        for (int i = threadIdx.x; i < lds_bins; i += blockDim.x) {
            const double v = sh[i];
            if (v != 0.0) unsafeAtomicAdd(&hist[i], v);
        }
    }
}

// pass 4: workgroup (bx, by) walks the list as workgroup bx of gridDim.x for the frequencies [8 by, 8 by + 8).
// part[gridDim.x][gridDim.y][4][8]: re x | im x | re y | im y of the chunk.  The phase is kept in turns: t = nu d, t -= rint(t), so that
// sincospi_small sees |2 t| <= 1 whatever nu and d are.  Four waves per SIMD (128 VGPRs): the accumulators take 64 of them.
__global__ __launch_bounds__(OT_RED_THREADS, 4) void spot_otf_kernel(int64_t n, const double* __restrict__ x, const double* __restrict__ y,
                                                                     const float* __restrict__ w, const unsigned int* __restrict__ fill,
                                                                     const double* __restrict__ mom, const double* __restrict__ freq, int K,
                                                                     double* __restrict__ part) {
    const SpotCentre c = spot_centre(mom);
    const int k0 = blockIdx.y * OT_SPOT_CHUNK;
    double nu[OT_SPOT_CHUNK];
#pragma unroll
    for (int j = 0; j < OT_SPOT_CHUNK; j++) nu[j] = freq[k0 + j < K ? k0 + j : K - 1];  // (wave-uniform; the tail repeats the last one)
    double v[4 * OT_SPOT_CHUNK];  // [re x | im x | re y | im y][8]
#pragma unroll
    for (int j = 0; j < 4 * OT_SPOT_CHUNK; j++) v[j] = 0.0;
    hit_list_for_each(n, fill, [&](int64_t i) {
        const float wi = w[i];
        if (!(wi > 0.f)) return;
        const double wd = (double)wi, dx = x[i] - c.x, dy = y[i] - c.y;
#pragma unroll
        for (int j = 0; j < OT_SPOT_CHUNK; j++) {
            double tx = nu[j] * dx, ty = nu[j] * dy, sn, cs;
            tx -= rint(tx);
            ty -= rint(ty);
            sincospi_small(2.0 * tx, &sn, &cs);
            v[j] += wd * cs;
            v[OT_SPOT_CHUNK + j] -= wd * sn;
            sincospi_small(2.0 * ty, &sn, &cs);
            v[2 * OT_SPOT_CHUNK + j] += wd * cs;
            v[3 * OT_SPOT_CHUNK + j] -= wd * sn;
        }
    });
    block_reduce_fixed<4 * OT_SPOT_CHUNK, red_max()>(v, part + ((int64_t)blockIdx.x * gridDim.y + blockIdx.y) * (4 * OT_SPOT_CHUNK));
}

// part[nblocks][chunks][4][8] -> out[4][K]: thread (q, k) adds its partials in index order
__global__ __launch_bounds__(OT_RED_THREADS) void spot_otf_final_kernel(const double* __restrict__ part, int nblocks, int K,
                                                                        double* __restrict__ out) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= 4 * K) return;
    const int q = j / K, k = j % K, chunks = (K + OT_SPOT_CHUNK - 1) / OT_SPOT_CHUNK;
    const double* col = part + ((int64_t)(k / OT_SPOT_CHUNK) * 4 + q) * OT_SPOT_CHUNK + k % OT_SPOT_CHUNK;
    double r = 0.0;
    for (int b = 0; b < nblocks; b++) r += col[(int64_t)b * chunks * (4 * OT_SPOT_CHUNK)];
    out[j] = r;
}
