// The fixed-order reduction of the analysis passes (spot analysis, wavefront analysis, footprints), whole: lane accumulators,
// __shfl_down across the wave, LDS across the four waves, one partial per workgroup (block_reduce_fixed), and a last kernel over
// the workgroups' partials (reduce_final_kernel).  The order of the additions depends on the launch shape alone -- which
// reduce_blocks (ot_host.hpp) takes from the length of the list, not from the device -- so two calls return the same bits.
// Its one kernel has internal linkage: every unit that includes this header gets a kernel of its own, and none collides.
#pragma once
#include "ot_device.hpp"

#define OT_RED_THREADS 256
#define OT_RED_WAVES (OT_RED_THREADS / 64)
static_assert(OT_RED_THREADS == 256, "reduce_blocks (ot_host.hpp) counts workgroups of 256");

// the mask of the quantities that are maxima: red_max(i, j, ...), none for an index below 0; red_max_range(i, j): i .. j - 1
typedef unsigned long long red_mask;
constexpr red_mask red_max() { return 0; }
template <class... T>
constexpr red_mask red_max(int i, T... more) {
    return (i < 0 ? 0 : (red_mask)1 << i) | red_max(more...);
}
constexpr red_mask red_max_range(int i, int j) { return i < j ? ((red_mask)1 << i) | red_max_range(i + 1, j) : 0; }

// v[0..M) of all lanes of the workgroup -> out[0..M), by thread m < M: sums, but the maximum for the quantities in MAXMASK
template <int M, red_mask MAXMASK>
OT_DEV void block_reduce_fixed(double (&v)[M], double* __restrict__ out) {
    static_assert(M <= OT_RED_THREADS, "one thread per quantity writes the partial");
    static_assert(M >= 64 || (MAXMASK >> M) == 0, "a maximum beyond the quantities");
    __shared__ double sh[OT_RED_WAVES][M];
    const bool first_lane = (threadIdx.x & 63) == 0;
#pragma unroll
    for (int m = 0; m < M; m++) {  // (stored as soon as folded: the 32 of the spot OTF pass folded side by side spill under its 128-register cap)
        double r = v[m];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_down(r, o);
            r = (m < 64 && ((MAXMASK >> m) & 1)) ? fmax(r, other) : r + other;
        }
        if (first_lane) sh[threadIdx.x >> 6][m] = r;
    }
    __syncthreads();
    if (threadIdx.x < M) {
        const bool is_max = threadIdx.x < 64 && ((MAXMASK >> threadIdx.x) & 1);
        double r = sh[0][threadIdx.x];
        for (int wv = 1; wv < OT_RED_WAVES; wv++) r = is_max ? fmax(r, sh[wv][threadIdx.x]) : r + sh[wv][threadIdx.x];
        out[threadIdx.x] = r;
    }
}

// part[nblocks][M] -> out[M]: wave wv takes the quantities wv, wv + 4, ..., lane l the partials l, l + 64, ... in that order,
// then the lanes fold as in the workgroups.  Bit m of maxmask: quantity m is a maximum; of negmask: it is stored negated (a
// minimum carried as the maximum of the negated values).  A maximum starts from -inf, also where every partial is >= 0 (the
// squared radii of the spot and wavefront passes): there is at least one partial, fmax of either start and a partial >= 0 is
// the partial, lanes without one lose to it in the fold: a start from 0 gives the same bits.  One workgroup of four waves per
// list: workgroup g of a batch (the sections of the footprints) folds part + g * part_stride into out + g * out_stride, each
// list in the order of a single one.
static __global__ __launch_bounds__(OT_RED_THREADS) void reduce_final_kernel(const double* __restrict__ part, int nblocks, int M,
                                                                            unsigned maxmask, unsigned negmask, double* __restrict__ out,
                                                                            int64_t part_stride, int64_t out_stride) {
    part += part_stride * blockIdx.x;
    out += out_stride * blockIdx.x;
    const int lane = threadIdx.x & 63;
    for (int m = threadIdx.x >> 6; m < M; m += OT_RED_WAVES) {  // (wave-uniform)
        const bool is_max = (maxmask >> m) & 1u;
        double r = is_max ? -__builtin_inf() : 0.0;
        for (int b = lane; b < nblocks; b += 64) {
            const double p = part[(int64_t)M * b + m];
            r = is_max ? fmax(r, p) : r + p;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_down(r, o);
            r = is_max ? fmax(r, other) : r + other;
        }
        if (lane == 0) out[m] = ((negmask >> m) & 1u) ? -r : r;
    }
}
