// The read-once sums per field and band that the field analysis (ot_field.hpp) and the wavefront across the field
// (ot_wavefield.hpp) share: the piece list of a launch, and the band sums a wave forms with its lanes in a second role, each lane
// the owner of one slot of some bands.  A slot named in MAXMASK is a maximum and not a sum (none in the field analysis: its
// code is what it was without the mask).  No kernels here.
#pragma once
#include "ot_block_reduce.hpp"
#include "ot_device.hpp"
#include "ot_field_ray.hpp"

// One launch takes up to FD_PIECES pieces; a piece is a field's range, or 2^28 rays of it: 32-bit offsets from `base`.
#define FD_PIECES 64
struct FdPiece {
    int64_t base;     // first ray of the piece in the storage
    uint32_t n;       // its rays, at most 2^28
    uint32_t blocks;  // workgroups that walk it
    uint32_t block0;  // place of its first workgroup's partial in the field's list
    uint32_t field;   // bits 0 .. 30 the field; bit 31: the field's last piece, which zeroes the rest of the list
};
struct FdBatch {
    FdPiece piece[FD_PIECES];
};

// The band sums of a wave.  The lanes change roles: lane (t, j) = (lane / J, lane % J), J = 64 / M, owns slot t of the bands
// j, j + J, ..., NC of them, in registers for the whole walk.  Per step every lane puts the M values of its ray into the wave's
// stage in LDS; then the wave goes through its rays of a band in lane order (a wave-uniform loop over the ballot), and the owner
// of (slot, band of the ray) adds the staged value: one addition per slot and ray whatever the number of bands, each sum a chain
// in the order of the rays.  stage[M][65]: a row per slot, one double of padding between rows.
template <int M>
struct FdRoles {
    static constexpr int J = 64 / M;
};
#define FD_STAGE 65

// what a sum starts from: 0, and -inf for the slots that are maxima
template <int M, int NC, red_mask MAXMASK = 0>
OT_DEV void fd_init_roles(double (&acc)[NC]) {
    constexpr int J = FdRoles<M>::J;
    const unsigned lane = threadIdx.x & 63, t = lane / J < M ? lane / J : M - 1;
    const bool is_max = MAXMASK && ((MAXMASK >> t) & 1);
#pragma unroll
    for (int n = 0; n < NC; n++) acc[n] = is_max ? -__builtin_inf() : 0.0;
}

template <int M, int NC, red_mask MAXMASK = 0>
OT_DEV void fd_add_rays(unsigned kb, const double (&v)[M], double (*stage)[FD_STAGE], double (&acc)[NC]) {
    constexpr int J = FdRoles<M>::J;
    const unsigned lane = threadIdx.x & 63, t = lane / J < M ? lane / J : M - 1, j = lane % J;
    const bool owner = lane < M * J;
    const bool is_max = MAXMASK && ((MAXMASK >> t) & 1);  // (of the lane's slot; no mask: a constant)
    const double idle = is_max ? -__builtin_inf() : 0.0;
    __builtin_amdgcn_wave_barrier();  // (the reads of the step before are done: the wave runs in step, LDS takes its requests in order)
#pragma unroll
    for (int m = 0; m < M; m++) stage[m][lane] = v[m];
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    unsigned long long pending = __ballot(kb != FD_NO_BAND);
    while (pending) {  // (wave-uniform: a ballot)
        const int i = __ffsll((long long)pending) - 1;
        pending &= pending - 1;
        const unsigned b = (unsigned)__builtin_amdgcn_readlane((int)kb, i);  // (wave-uniform)
        const double x = (owner && b % J == j) ? stage[t][i] : idle;
        const unsigned c = b / J;
#pragma unroll
        for (int n = 0; n < NC; n++)
            if (c == (unsigned)n) acc[n] = is_max ? fmax(acc[n], x) : acc[n] + x;  // (a wave-uniform choice; x + 0 changes no bit)
    }
}

// the lanes' sums -> the wave's acc[K][M] in LDS
template <int M, int NC>
OT_DEV void fd_store_roles(const double (&acc)[NC], unsigned K, double (*out)[M]) {
    constexpr int J = FdRoles<M>::J;
    const unsigned lane = threadIdx.x & 63, t = lane / J, j = lane % J;
    if (lane >= M * J) return;
#pragma unroll
    for (int n = 0; n < NC; n++)
        if (j + n * J < K) out[j + n * J][t] = acc[n];
}

// acc[waves][K][SLOTS] in LDS -> part[K][SLOTS], the waves in their order
template <int SLOTS, red_mask MAXMASK = 0>
OT_DEV void fd_write_partial(const double (*acc)[OT_CHROM_MAX_BANDS][SLOTS], unsigned K, double* __restrict__ part) {
    __syncthreads();
    for (unsigned t = threadIdx.x; t < K * SLOTS; t += OT_RED_THREADS) {
        const unsigned b = t / SLOTS, m = t % SLOTS;
        const bool is_max = MAXMASK && ((MAXMASK >> m) & 1);
        double r = acc[0][b][m];
        for (int wv = 1; wv < OT_RED_WAVES; wv++) r = is_max ? fmax(r, acc[wv][b][m]) : r + acc[wv][b][m];
        part[t] = r;
    }
}

// A workgroup beyond its piece's: nothing to walk.  Those of a field's last piece fill the rest of the field's list with zeros
// (-inf for a maximum), which the last kernel adds without changing a bit of the sums.  cell = K * SLOTS.  -> true: the
// workgroup has rays.
template <int SLOTS = 1, red_mask MAXMASK = 0>
OT_DEV bool fd_my_piece(const FdPiece& P, unsigned list_len, unsigned cell, double* __restrict__ part_field) {
    if (blockIdx.x < P.blocks) return true;
    const unsigned at = P.block0 + blockIdx.x;
    if ((P.field >> 31) && at < list_len)
        for (unsigned t = threadIdx.x; t < cell; t += OT_RED_THREADS)
            part_field[(int64_t)at * cell + t] = MAXMASK && ((MAXMASK >> (t % SLOTS)) & 1) ? -__builtin_inf() : 0.0;
    return false;
}
