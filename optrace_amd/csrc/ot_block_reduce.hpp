// The fixed-order workgroup reduction of the analysis passes (spot analysis, wavefront analysis): lane accumulators, __shfl_down
// across the wave, LDS across the four waves, one partial per workgroup.  The order of the additions depends on the launch
// shape alone, so two calls return the same bits.
// Holds no kernels: any unit may include it.
#pragma once
#include "ot_device.hpp"

#define OT_SPOT_THREADS 256
#define OT_SPOT_WAVES (OT_SPOT_THREADS / 64)

// v[0..M) of all lanes of the workgroup -> out[0..M), by thread m < M: sums, but the maximum for m == MAXI and m == MAXJ
template <int M, int MAXI, int MAXJ = MAXI>
OT_DEV void spot_block_reduce(double (&v)[M], double* __restrict__ out) {
    static_assert(M <= OT_SPOT_THREADS, "one thread per quantity writes the partial");
    __shared__ double sh[OT_SPOT_WAVES][M];
    const bool first_lane = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int m = 0; m < M; m++) {  // (stored as soon as folded: the 32 of the spot OTF pass folded side by side spill under its 128-register cap)
        double r = v[m];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_down(r, o);
            r = (m == MAXI || m == MAXJ) ? fmax(r, other) : r + other;
        }
        if (first_lane) sh[threadIdx.x >> 6][m] = r;
    }
    __syncthreads();
    if (threadIdx.x < M) {
        const bool is_max = (int)threadIdx.x == MAXI || (int)threadIdx.x == MAXJ;
        double r = sh[0][threadIdx.x];
        for (int wv = 1; wv < OT_SPOT_WAVES; wv++) r = is_max ? fmax(r, sh[wv][threadIdx.x]) : r + sh[wv][threadIdx.x];
        out[threadIdx.x] = r;
    }
}
