// Hit lists behind the detector stage: their layout and the index walk of the kernels that stream them (spectrum, spot
// analysis; the wavefront analysis walks its planes as a dense list).  A list is dense (one entry per ray of the bundle,
// weight 0 = no valid hit, as ot_detector_hits leaves it) or compact (ot_detector_req.fill: 1024 pieces of hit_piece_len(n)
// entries, piece k holding fill[k] valid hits at its front).
// Holds no kernels: any unit may include it.
#pragma once
#include "ot_device.hpp"

#define OT_HIT_PIECES_N 1024
// entries per piece of a compact hit list of capacity n: the power of two at or above n / 1024 (at least 1024), so that a
// ray's piece is a shift of its index; the last pieces of the 1024 stay empty
__host__ __device__ static inline int hit_piece_shift(int64_t n) {
    int s = 10;
    while (((int64_t)OT_HIT_PIECES_N << s) < n) s++;
    return s;
}
__host__ __device__ static inline int64_t hit_piece_len(int64_t n) { return (int64_t)1 << hit_piece_shift(n); }

#define OT_HIT_SLICE 8192  // entries of a compact list a workgroup takes at a time

// body(i) for i in [0, n), grid-stride: the walk of a dense list, and of the dense planes of the wavefront analysis.  `return`
// in the body goes on to the next entry.
template <class F>
OT_DEV void dense_for_each(int64_t n, F&& body) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) body(i);
}

// body(i) for the entries of a list: dense = dense_for_each; compact = the workgroup takes whole slices of pieces.
// Which workgroup and lane sees which entry depends on the launch shape alone (blockIdx.x / gridDim.x: a second grid
// dimension may carry something else).
template <class F>
OT_DEV void hit_list_for_each(int64_t n, const unsigned int* __restrict__ fill, F&& body) {
    if (!fill) {
        dense_for_each(n, body);
        return;
    }
    // work items = (piece, slice of OT_HIT_SLICE entries): a workgroup per whole piece left the 1024 pieces of a long list
    // (2e8 rays: 7e4 filled entries each) to 1024 workgroups walking them serially -- 0.54 / 0.84 ms for the two spectrum
    // passes over 0.56 GB; slices beyond a piece's fill cost one comparison
    const int shift = hit_piece_shift(n);
    const int64_t slices = (((int64_t)1 << shift) + OT_HIT_SLICE - 1) / OT_HIT_SLICE;  // per piece
    for (int64_t it = blockIdx.x; it < OT_HIT_PIECES_N * slices; it += gridDim.x) {
        const int64_t sl = it / OT_HIT_PIECES_N, pc = it % OT_HIT_PIECES_N;  // slice-major: the filled front slices spread over all workgroups
        const int64_t i0 = (pc << shift) + sl * OT_HIT_SLICE;
        int64_t i1 = (pc << shift) + (int64_t)fill[pc];
        if (i1 > i0 + OT_HIT_SLICE) i1 = i0 + OT_HIT_SLICE;
        for (int64_t i = i0 + threadIdx.x; i < i1; i += blockDim.x) body(i);
    }
}
