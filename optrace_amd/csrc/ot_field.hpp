// Field analysis of a stored trace (Raytracer.field_analysis): per field point -- the rays of one source, one contiguous range of
// the storage -- and per band of wavelengths the first and second moments of the ray lines of section k, written as
// x(z) = origin_xy + a + (z - origin_z) m.  Definition: DESIGN.md "Field analysis"; the record's slots: include/optrace_amd.h.
//   pass 1   per (field, band) over the used rays with d_z != 0: sum w, count, sum w a, sum w m, sum w wl; used rays with d_z == 0
//   pass 2   about the means of pass 1, (da, dm) = (a, m) - mean formed before multiplying: the ten second moments of (a, m)
// Read-once shape: a workgroup walks the rays of ONE field; a lane reads its ray's key, one byte, and the weight, the positions
// and the wavelength when the key is a band -- once per ray, whatever the number of fields and bands.  The band sums are formed
// by the wave with its lanes in a second role (fd_add_rays): one addition per slot and ray, in registers.  At the end the lanes'
// sums go to LDS and the four waves' are added in wave order: the workgroup's partial [K][slots].  Every addition's place in
// the order follows from the counts and K alone.
// Included by ot_field_api.hip alone.
#pragma once
#include "ot_block_reduce.hpp"
#include "ot_device.hpp"
#include "ot_field_ray.hpp"

// slots of the record (include/optrace_amd.h, ot_field_sums): pass 1 carries the first FD_M1 of them, pass 2 the rest
enum { FD_W = 0, FD_COUNT, FD_WAX, FD_WAY, FD_WMX, FD_WMY, FD_WWL, FD_PARALLEL, FD_M1,
       FD_AXAX = FD_M1, FD_AXAY, FD_AYAY, FD_AXMX, FD_AXMY, FD_AYMX, FD_AYMY, FD_MXMX, FD_MXMY, FD_MYMY, FD_M };
static_assert(FD_M == OT_FIELD_M && FD_M1 == 8, "the record of the header");
#define FD_M2 (FD_M - FD_M1)

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

template <int M, int NC>
OT_DEV void fd_add_rays(unsigned kb, const double (&v)[M], double (*stage)[FD_STAGE], double (&acc)[NC]) {
    constexpr int J = FdRoles<M>::J;
    const unsigned lane = threadIdx.x & 63, t = lane / J < M ? lane / J : M - 1, j = lane % J;
    const bool owner = lane < M * J;
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
        const double x = (owner && b % J == j) ? stage[t][i] : 0.0;
        const unsigned c = b / J;
#pragma unroll
        for (int n = 0; n < NC; n++)
            if (c == (unsigned)n) acc[n] += x;  // (a wave-uniform choice; x + 0 changes no bit)
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
template <int SLOTS>
OT_DEV void fd_write_partial(const double (*acc)[OT_CHROM_MAX_BANDS][SLOTS], unsigned K, double* __restrict__ part) {
    __syncthreads();
    for (unsigned t = threadIdx.x; t < K * SLOTS; t += OT_RED_THREADS) {
        const unsigned b = t / SLOTS, m = t % SLOTS;
        double r = acc[0][b][m];
        for (int wv = 1; wv < OT_RED_WAVES; wv++) r += acc[wv][b][m];
        part[t] = r;
    }
}

// A workgroup beyond its piece's: nothing to walk.  Those of a field's last piece fill the rest of the field's list with zeros,
// which the last kernel adds without changing a bit of the sums.  -> true: the workgroup has rays.
OT_DEV bool fd_my_piece(const FdPiece& P, unsigned list_len, unsigned cell, double* __restrict__ part_field) {
    if (blockIdx.x < P.blocks) return true;
    const unsigned at = P.block0 + blockIdx.x;
    if ((P.field >> 31) && at < list_len)
        for (unsigned t = threadIdx.x; t < cell; t += OT_RED_THREADS) part_field[(int64_t)at * cell + t] = 0.0;
    return false;
}

// part[F][list_len][K][FD_M1]; grid (list_len, pieces of the batch).  NC: bands a lane owns, NC * (64 / FD_M1) >= K
template <int NC>
__global__ __launch_bounds__(OT_RED_THREADS) void fd_first_kernel(const double* __restrict__ p, const float* __restrict__ w,
                                                                  const float* __restrict__ wl, const uint8_t* __restrict__ key,
                                                                  int64_t key_first, int64_t N, int nt, int k, FdBatch batch, unsigned K,
                                                                  unsigned list_len, double ox, double oy, double oz,
                                                                  double* __restrict__ part) {
    __shared__ double sums[OT_RED_WAVES][OT_CHROM_MAX_BANDS][FD_M1];
    __shared__ double stage[OT_RED_WAVES][FD_M1][FD_STAGE];
    const FdPiece P = batch.piece[blockIdx.y];
    const unsigned cell = K * FD_M1;
    double* part_field = part + (int64_t)(P.field & 0x7fffffffu) * list_len * cell;
    if (!fd_my_piece(P, list_len, cell, part_field)) return;  // (workgroup-uniform)
    const FdSection S = fd_section(p + P.base, w + P.base, wl + P.base, key + (P.base - key_first), N, nt, k);
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc[NC];
#pragma unroll
    for (int n = 0; n < NC; n++) acc[n] = 0.0;

    const uint32_t stride = P.blocks * OT_RED_THREADS;  // (at most 2^18 beyond n <= 2^28: no wrap)
    for (uint32_t r0 = blockIdx.x * OT_RED_THREADS + wave * 64; r0 < P.n; r0 += stride) {  // (wave-uniform)
        const uint32_t r = r0 + lane;
        unsigned kb = r < P.n ? S.key[r] : FD_NO_BAND;
        if (kb >= K) kb = FD_NO_BAND;
        double v[FD_M1] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (kb != FD_NO_BAND) {
            FdRay q;
            if (!fd_ray(S, r, ox, oy, oz, q)) {
                kb = FD_NO_BAND;
            } else if (q.dz == 0.0) {
                v[FD_PARALLEL] = 1.0;
            } else {
                v[FD_W] = q.w;
                v[FD_COUNT] = 1.0;  // (exact up to 2^53 rays)
                v[FD_WAX] = q.w * q.ax;
                v[FD_WAY] = q.w * q.ay;
                v[FD_WMX] = q.w * q.mx;
                v[FD_WMY] = q.w * q.my;
                v[FD_WWL] = q.w * (double)S.wl[r];
            }
        }
        fd_add_rays<FD_M1, NC>(kb, v, stage[wave], acc);
    }
    fd_store_roles<FD_M1, NC>(acc, K, sums[wave]);
    fd_write_partial<FD_M1>(sums, K, part_field + (int64_t)(P.block0 + blockIdx.x) * cell);
}

// part[F][list_len][K][FD_M2]; first[F][K][FD_M1]: the sums of pass 1.  NC * (64 / FD_M2) >= K
template <int NC>
__global__ __launch_bounds__(OT_RED_THREADS) void fd_central_kernel(const double* __restrict__ p, const float* __restrict__ w,
                                                                    const uint8_t* __restrict__ key, int64_t key_first, int64_t N, int nt,
                                                                    int k, FdBatch batch, unsigned K, unsigned list_len, double ox,
                                                                    double oy, double oz, const double* __restrict__ first,
                                                                    double* __restrict__ part) {
    __shared__ double sums[OT_RED_WAVES][OT_CHROM_MAX_BANDS][FD_M2];
    __shared__ double stage[OT_RED_WAVES][FD_M2][FD_STAGE];
    __shared__ double mean[OT_CHROM_MAX_BANDS][4];
    const FdPiece P = batch.piece[blockIdx.y];
    const unsigned cell = K * FD_M2, f = P.field & 0x7fffffffu;
    double* part_field = part + (int64_t)f * list_len * cell;
    if (!fd_my_piece(P, list_len, cell, part_field)) return;  // (workgroup-uniform)
    const FdSection S = fd_section(p + P.base, w + P.base, nullptr, key + (P.base - key_first), N, nt, k);
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc[NC];
#pragma unroll
    for (int n = 0; n < NC; n++) acc[n] = 0.0;
    if (threadIdx.x < K * 4) {
        // the means: the same IEEE quotients as the host forms from the record (no ray in the sums: NaN, and nothing reads it)
        const double* m = first + ((int64_t)f * K + threadIdx.x / 4) * FD_M1;
        mean[threadIdx.x / 4][threadIdx.x % 4] = m[FD_WAX + threadIdx.x % 4] / m[FD_W];
    }
    __syncthreads();

    const uint32_t stride = P.blocks * OT_RED_THREADS;
    for (uint32_t r0 = blockIdx.x * OT_RED_THREADS + wave * 64; r0 < P.n; r0 += stride) {  // (wave-uniform)
        const uint32_t r = r0 + lane;
        unsigned kb = r < P.n ? S.key[r] : FD_NO_BAND;
        if (kb >= K) kb = FD_NO_BAND;
        double v[FD_M2];
#pragma unroll
        for (int m = 0; m < FD_M2; m++) v[m] = 0.0;
        if (kb != FD_NO_BAND) {
            FdRay q;
            if (!fd_ray(S, r, ox, oy, oz, q) || q.dz == 0.0) {
                kb = FD_NO_BAND;
            } else {
                const double dax = q.ax - mean[kb][0], day = q.ay - mean[kb][1], dmx = q.mx - mean[kb][2], dmy = q.my - mean[kb][3];
                v[FD_AXAX - FD_M1] = q.w * (dax * dax);
                v[FD_AXAY - FD_M1] = q.w * (dax * day);
                v[FD_AYAY - FD_M1] = q.w * (day * day);
                v[FD_AXMX - FD_M1] = q.w * (dax * dmx);
                v[FD_AXMY - FD_M1] = q.w * (dax * dmy);
                v[FD_AYMX - FD_M1] = q.w * (day * dmx);
                v[FD_AYMY - FD_M1] = q.w * (day * dmy);
                v[FD_MXMX - FD_M1] = q.w * (dmx * dmx);
                v[FD_MXMY - FD_M1] = q.w * (dmx * dmy);
                v[FD_MYMY - FD_M1] = q.w * (dmy * dmy);
            }
        }
        fd_add_rays<FD_M2, NC>(kb, v, stage[wave], acc);
    }
    fd_store_roles<FD_M2, NC>(acc, K, sums[wave]);
    fd_write_partial<FD_M2>(sums, K, part_field + (int64_t)(P.block0 + blockIdx.x) * cell);
}

// first[cells][FD_M1], central[cells][FD_M2] -> rec[cells][FD_M]; a cell without a ray in the sums has no second moments: NaN in
// place of the zeros that were added up (the policy of ch_finish_kernel).  One thread per cell (field, band).
__global__ void fd_finish_kernel(int cells, const double* __restrict__ first, const double* __restrict__ central,
                                 double* __restrict__ rec) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= cells) return;
    double* m = rec + (int64_t)FD_M * c;
    for (int s = 0; s < FD_M1; s++) m[s] = first[(int64_t)FD_M1 * c + s];
    const bool none = m[FD_COUNT] == 0.0;
    for (int s = 0; s < FD_M2; s++) m[FD_M1 + s] = none ? __builtin_nan("") : central[(int64_t)FD_M2 * c + s];
}
