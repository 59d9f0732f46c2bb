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
#include "ot_field_roles.hpp"

// slots of the record (include/optrace_amd.h, ot_field_sums): pass 1 carries the first FD_M1 of them, pass 2 the rest
enum { FD_W = 0, FD_COUNT, FD_WAX, FD_WAY, FD_WMX, FD_WMY, FD_WWL, FD_PARALLEL, FD_M1,
       FD_AXAX = FD_M1, FD_AXAY, FD_AYAY, FD_AXMX, FD_AXMY, FD_AYMX, FD_AYMY, FD_MXMX, FD_MXMY, FD_MYMY, FD_M };
static_assert(FD_M == OT_FIELD_M && FD_M1 == 8, "the record of the header");
#define FD_M2 (FD_M - FD_M1)

// (the piece list of a launch and the lanes' second role, fd_add_rays: ot_field_roles.hpp)

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
