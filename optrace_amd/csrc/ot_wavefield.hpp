// Wavefront across the field (Raytracer.wavefront_field): per field point -- the rays of one source, one contiguous range of the
// storage -- and per band of wavelengths the optical path to a reference sphere of the cell's own, its moments and the normal
// equations of a Zernike fit.  Definition: DESIGN.md "Wavefront across the field"; the records: include/optrace_amd.h.
//   focus    per cell the 17 sums of ot_wavefront_focus (wf_focus_kernel: the same terms)
//   paths    per ray the path to the sphere of its cell, looked up in a table [F][K][4] on the device: wf_path, the function of
//            wf_paths_kernel, so a ray's u, v, opl and w_out are the bits of ot_wavefront_paths with that sphere
//   moments  per cell the sums of the dense planes, then, about the means of those, sum w opd^2 and the largest squared
//            distance from the field's pupil centre
//   zernike  per cell G = sum w Z Z^T and g = sum w Z opd, Z on the field's pupil
// focus and moments have the read-once shape of the field analysis (ot_field_roles.hpp): a workgroup walks the rays of ONE field,
// a lane reads its ray's key and, for a ray with a band, the ray's data, once whatever F and K are; the wave adds with its lanes
// in their second role.  paths is one thread per ray.  zernike is a grid over (walker, chunk of the triangle, cell): a workgroup
// reads the key bytes of its share of the field and the planes of its own band's entries only, and adds as wf_zernike_kernel does.
// Every sum is added in an order that follows from the field's count, K and J alone.
// Defines kernels that are no templates: included by ot_wavefield_api.hip alone.
#pragma once
#include "ot_block_reduce.hpp"
#include "ot_device.hpp"
#include "ot_field_roles.hpp"
#include "ot_wavefront_ray.hpp"

// slots of the moments record of a cell and of the pupil record of a field (include/optrace_amd.h)
enum { WVF_W = 0, WVF_COUNT, WVF_WOPL, WVF_WU, WVF_WV, WVF_WWL, WVF_OPL_MIN, WVF_OPL_MAX, WVF_M1, WVF_WOPD2 = WVF_M1, WVF_M };
enum { WVF_CU = 0, WVF_CV, WVF_R2MAX, WVF_PUPIL_R, WVF_PUPIL_M };
static_assert(WVF_M == OT_WFF_M && WVF_PUPIL_M == OT_WFF_PUPIL_M && WVF_M1 == 8, "the records of the header");
#define WVF_M2 2  // the second pass of a cell: sum w opd^2 | max of the squared distance from the field's pupil centre
constexpr red_mask WVF_MAX1 = red_max(WVF_OPL_MIN, WVF_OPL_MAX), WVF_MAX2 = red_max(1);

// part[F][list_len][K][WFF_M]; grid (list_len, pieces of the batch).  NC: bands a lane owns, NC * (64 / WFF_M) >= K
template <int NC>
__global__ __launch_bounds__(OT_RED_THREADS) void wvf_focus_kernel(ot_rays R, const uint8_t* __restrict__ key, int64_t key_first, int k,
                                                                   FdBatch batch, unsigned K, unsigned list_len, double ox, double oy,
                                                                   double oz, double* __restrict__ part) {
    __shared__ double sums[OT_RED_WAVES][OT_CHROM_MAX_BANDS][WFF_M];
    __shared__ double stage[OT_RED_WAVES][WFF_M][FD_STAGE];
    const FdPiece P = batch.piece[blockIdx.y];
    const unsigned cell = K * WFF_M;
    double* part_field = part + (int64_t)(P.field & 0x7fffffffu) * list_len * cell;
    if (!fd_my_piece(P, list_len, cell, part_field)) return;  // (workgroup-uniform)
    const uint8_t* kp = key + (P.base - key_first);
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc[NC];
    fd_init_roles<WFF_M, NC>(acc);

    const uint32_t stride = P.blocks * OT_RED_THREADS;  // (at most 2^18 beyond n <= 2^28: no wrap)
    for (uint32_t r0 = blockIdx.x * OT_RED_THREADS + wave * 64; r0 < P.n; r0 += stride) {  // (wave-uniform)
        const uint32_t i = r0 + lane;
        unsigned kb = i < P.n ? kp[i] : FD_NO_BAND;
        if (kb >= K) kb = FD_NO_BAND;
        double v[WFF_M];
#pragma unroll
        for (int m = 0; m < WFF_M; m++) v[m] = 0.0;
        if (kb != FD_NO_BAND) {
            const int64_t r = P.base + i;
            const WfRay q = wf_section(R, r, k, wf_position(R, r, k));
            if (!q.used) {
                kb = FD_NO_BAND;
            } else {
                const double w = q.w, px = q.p.x - ox, py = q.p.y - oy, pz = q.p.z - oz;
                const V3 s = q.s;
                const double sp = s.x * px + s.y * py + s.z * pz;
                v[WFF_W] = w;
                v[WFF_COUNT] = 1.0;  // (exact up to 2^53 rays)
                v[WFF_P + 0] = w * px;
                v[WFF_P + 1] = w * py;
                v[WFF_P + 2] = w * pz;
                v[WFF_S + 0] = w * s.x;
                v[WFF_S + 1] = w * s.y;
                v[WFF_S + 2] = w * s.z;
                v[WFF_A + 0] = w * (1.0 - s.x * s.x);
                v[WFF_A + 1] = -(w * (s.x * s.y));
                v[WFF_A + 2] = -(w * (s.x * s.z));
                v[WFF_A + 3] = w * (1.0 - s.y * s.y);
                v[WFF_A + 4] = -(w * (s.y * s.z));
                v[WFF_A + 5] = w * (1.0 - s.z * s.z);
                v[WFF_B + 0] = w * (px - s.x * sp);
                v[WFF_B + 1] = w * (py - s.y * sp);
                v[WFF_B + 2] = w * (pz - s.z * sp);
            }
        }
        fd_add_rays<WFF_M, NC>(kb, v, stage[wave], acc);
    }
    fd_store_roles<WFF_M, NC>(acc, K, sums[wave]);
    fd_write_partial<WFF_M>(sums, K, part_field + (int64_t)(P.block0 + blockIdx.x) * cell);
}

// part[lists][list_len][cell] -> out[lists][cell], cell = K * slots: reduce_final_kernel (ot_block_reduce.hpp) for records whose
// slots repeat per band -- bit m % slots of maxmask: a maximum, of negmask: stored negated.  Wave wv takes the quantities wv,
// wv + 4, ..., lane l the partials l, l + 64, ... in that order, then the lanes fold.  One workgroup per list.
__global__ __launch_bounds__(OT_RED_THREADS) void wvf_final_kernel(const double* __restrict__ part, int list_len, int cell, int slots,
                                                                   unsigned maxmask, unsigned negmask, double* __restrict__ out) {
    part += (int64_t)list_len * cell * blockIdx.x;
    out += (int64_t)cell * blockIdx.x;
    const int lane = threadIdx.x & 63;
    for (int m = threadIdx.x >> 6; m < cell; m += OT_RED_WAVES) {  // (wave-uniform)
        const bool is_max = (maxmask >> (m % slots)) & 1u;
        double r = is_max ? -__builtin_inf() : 0.0;
        for (int b = lane; b < list_len; b += 64) {
            const double p = part[(int64_t)cell * b + m];
            r = is_max ? fmax(r, p) : r + p;
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double other = __shfl_down(r, o);
            r = is_max ? fmax(r, other) : r + other;
        }
        if (lane == 0) out[m] = ((negmask >> (m % slots)) & 1u) ? -r : r;
    }
}

// (c, R) of a cell: a sphere only where all four are finite and R is not 0
OT_DEV bool wvf_has_sphere(const double* c) {
    const double inf = __builtin_inf();
    return fabs(c[0]) < inf && fabs(c[1]) < inf && fabs(c[2]) < inf && fabs(c[3]) < inf && c[3] != 0.0;
}

// One thread per ray of a piece; grid (workgroups of the longest piece, pieces of the batch).  spheres[F][K][4]: (c, R) per
// cell, no number: no sphere.  The dense planes start at ray key_first, as the key does.  counts[F][K][2]: used rays of the
// cell whose line misses its sphere | used rays of a cell without a sphere (integer atomics: no order to depend on).
__global__ __launch_bounds__(OT_RED_THREADS) void wvf_paths_kernel(ot_rays R, const uint8_t* __restrict__ key, int64_t key_first, int k,
                                                                   FdBatch batch, unsigned K, const double* __restrict__ spheres,
                                                                   double* __restrict__ u, double* __restrict__ v,
                                                                   double* __restrict__ opl, float* __restrict__ w_out,
                                                                   unsigned long long* __restrict__ counts) {
    __shared__ double sph[OT_CHROM_MAX_BANDS][4];
    __shared__ unsigned cnt[OT_CHROM_MAX_BANDS][2];
    const FdPiece P = batch.piece[blockIdx.y];
    const unsigned f = P.field & 0x7fffffffu;
    if ((uint64_t)blockIdx.x * OT_RED_THREADS >= P.n) return;  // (workgroup-uniform)
    if (threadIdx.x < K * 4) sph[threadIdx.x / 4][threadIdx.x % 4] = spheres[((int64_t)f * K) * 4 + threadIdx.x];
    if (threadIdx.x < K * 2) cnt[threadIdx.x / 2][threadIdx.x % 2] = 0u;
    __syncthreads();
    const uint32_t i = blockIdx.x * OT_RED_THREADS + threadIdx.x;
    if (i < P.n) {
        const int64_t r = P.base + i, at = r - key_first;
        const unsigned kb = key[at];
        const double nan = __builtin_nan("");
        double ui = nan, vi = nan, li = nan;
        float wi = 0.f;
        if (kb < K) {
            if (wvf_has_sphere(sph[kb])) {
                if (wf_path(R, r, k, sph[kb][0], sph[kb][1], sph[kb][2], sph[kb][3], ui, vi, li, wi)) atomicAdd(&cnt[kb][0], 1u);
            } else if (wf_section(R, r, k, wf_position(R, r, k)).used) {
                atomicAdd(&cnt[kb][1], 1u);
            }
        }
        u[at] = ui;
        v[at] = vi;
        opl[at] = li;
        w_out[at] = wi;
    }
    __syncthreads();
    if (threadIdx.x < K * 2) {
        const unsigned c = cnt[threadIdx.x / 2][threadIdx.x % 2];
        if (c) atomicAdd(&counts[((int64_t)f * K) * 2 + threadIdx.x], (unsigned long long)c);
    }
}

// ---- moments of the planes ------------------------------------------------------------------------------------------
// An entry counts when its key is a band and w_out > 0 (a used ray that met the sphere of its cell).
// part[F][list_len][K][WVF_M1]: the first eight slots of the record, the minimum as the maximum of -opl
template <int NC>
__global__ __launch_bounds__(OT_RED_THREADS) void wvf_first_kernel(const double* __restrict__ u, const double* __restrict__ v,
                                                                   const double* __restrict__ opl, const float* __restrict__ w,
                                                                   const float* __restrict__ wl, const uint8_t* __restrict__ key,
                                                                   int64_t key_first, FdBatch batch, unsigned K, unsigned list_len,
                                                                   double* __restrict__ part) {
    __shared__ double sums[OT_RED_WAVES][OT_CHROM_MAX_BANDS][WVF_M1];
    __shared__ double stage[OT_RED_WAVES][WVF_M1][FD_STAGE];
    const FdPiece P = batch.piece[blockIdx.y];
    const unsigned cell = K * WVF_M1;
    double* part_field = part + (int64_t)(P.field & 0x7fffffffu) * list_len * cell;
    if (!fd_my_piece<WVF_M1, WVF_MAX1>(P, list_len, cell, part_field)) return;  // (workgroup-uniform)
    const int64_t at = P.base - key_first;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc[NC];
    fd_init_roles<WVF_M1, NC, WVF_MAX1>(acc);

    const uint32_t stride = P.blocks * OT_RED_THREADS;
    for (uint32_t r0 = blockIdx.x * OT_RED_THREADS + wave * 64; r0 < P.n; r0 += stride) {  // (wave-uniform)
        const uint32_t i = r0 + lane;
        unsigned kb = i < P.n ? key[at + i] : FD_NO_BAND;
        if (kb >= K) kb = FD_NO_BAND;
        double a[WVF_M1] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (kb != FD_NO_BAND) {
            const float wi = w[at + i];
            if (!(wi > 0.f)) {
                kb = FD_NO_BAND;
            } else {
                const double wd = (double)wi, l = opl[at + i];
                a[WVF_W] = wd;
                a[WVF_COUNT] = 1.0;
                a[WVF_WOPL] = wd * l;
                a[WVF_WU] = wd * u[at + i];
                a[WVF_WV] = wd * v[at + i];
                a[WVF_WWL] = wd * (double)wl[at + i];
                a[WVF_OPL_MIN] = -l;
                a[WVF_OPL_MAX] = l;
            }
        }
        fd_add_rays<WVF_M1, NC, WVF_MAX1>(kb, a, stage[wave], acc);
    }
    fd_store_roles<WVF_M1, NC>(acc, K, sums[wave]);
    fd_write_partial<WVF_M1, WVF_MAX1>(sums, K, part_field + (int64_t)(P.block0 + blockIdx.x) * cell);
}

// first[F][K][WVF_M1] -> pupil[F][0 .. 1]: the pupil centre of a field, common to its bands, (sum_b slot 3, sum_b slot 4) /
// sum_b slot 0 added in band order.  One thread per field.
__global__ void wvf_centre_kernel(int F, int K, const double* __restrict__ first, double* __restrict__ pupil) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double W = 0.0, su = 0.0, sv = 0.0;
    for (int b = 0; b < K; b++) {
        const double* m = first + ((int64_t)f * K + b) * WVF_M1;
        W += m[WVF_W];
        su += m[WVF_WU];
        sv += m[WVF_WV];
    }
    pupil[WVF_PUPIL_M * f + WVF_CU] = su / W;
    pupil[WVF_PUPIL_M * f + WVF_CV] = sv / W;
}

// part[F][list_len][K][2]: sum w opd^2 about the cell's mean | max (du^2 + dv^2) about the field's pupil centre
__global__ __launch_bounds__(OT_RED_THREADS) void wvf_central_kernel(const double* __restrict__ u, const double* __restrict__ v,
                                                                     const double* __restrict__ opl, const float* __restrict__ w,
                                                                     const uint8_t* __restrict__ key, int64_t key_first, FdBatch batch,
                                                                     unsigned K, unsigned list_len, const double* __restrict__ first,
                                                                     const double* __restrict__ pupil, double* __restrict__ part) {
    __shared__ double sums[OT_RED_WAVES][OT_CHROM_MAX_BANDS][WVF_M2];
    __shared__ double stage[OT_RED_WAVES][WVF_M2][FD_STAGE];
    __shared__ double mean[OT_CHROM_MAX_BANDS];
    const FdPiece P = batch.piece[blockIdx.y];
    const unsigned cell = K * WVF_M2, f = P.field & 0x7fffffffu;
    double* part_field = part + (int64_t)f * list_len * cell;
    if (!fd_my_piece<WVF_M2, WVF_MAX2>(P, list_len, cell, part_field)) return;  // (workgroup-uniform)
    const int64_t at = P.base - key_first;
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    double acc[1];  // (WVF_M2 = 2: a lane owns one slot of one band, 32 bands to a wave)
    fd_init_roles<WVF_M2, 1, WVF_MAX2>(acc);
    if (threadIdx.x < K) {
        // the means: the same IEEE quotients as the host forms from the record (no entry in the sums: NaN, and nothing reads it)
        const double* m = first + ((int64_t)f * K + threadIdx.x) * WVF_M1;
        mean[threadIdx.x] = m[WVF_WOPL] / m[WVF_W];
    }
    const double cu = pupil[WVF_PUPIL_M * f + WVF_CU], cv = pupil[WVF_PUPIL_M * f + WVF_CV];
    __syncthreads();

    const uint32_t stride = P.blocks * OT_RED_THREADS;
    for (uint32_t r0 = blockIdx.x * OT_RED_THREADS + wave * 64; r0 < P.n; r0 += stride) {  // (wave-uniform)
        const uint32_t i = r0 + lane;
        unsigned kb = i < P.n ? key[at + i] : FD_NO_BAND;
        if (kb >= K) kb = FD_NO_BAND;
        double a[WVF_M2] = {0.0, 0.0};
        if (kb != FD_NO_BAND) {
            const float wi = w[at + i];
            if (!(wi > 0.f)) {
                kb = FD_NO_BAND;
            } else {
                const double d = opl[at + i] - mean[kb], du = u[at + i] - cu, dv = v[at + i] - cv;
                a[0] = (double)wi * (d * d);
                a[1] = du * du + dv * dv;
            }
        }
        fd_add_rays<WVF_M2, 1, WVF_MAX2>(kb, a, stage[wave], acc);
    }
    fd_store_roles<WVF_M2, 1>(acc, K, sums[wave]);
    fd_write_partial<WVF_M2, WVF_MAX2>(sums, K, part_field + (int64_t)(P.block0 + blockIdx.x) * cell);
}

// first[F][K][8], central[F][K][2] -> moments[F][K][WVF_M], and the rest of pupil[F][4]: the largest squared distance of the
// field's counted entries from its centre and the root of it, the pupil radius the fit divides by when the caller gives none.  A
// cell without an entry: slots 0 .. 7 zero, slot 8 NaN (the policy of fd_finish_kernel).  One thread per field.
__global__ void wvf_finish_kernel(int F, int K, const double* __restrict__ first, const double* __restrict__ central,
                                  double* __restrict__ moments, double* __restrict__ pupil) {
    const int f = blockIdx.x * blockDim.x + threadIdx.x;
    if (f >= F) return;
    double r2 = 0.0;
    for (int b = 0; b < K; b++) {
        const int64_t c = (int64_t)f * K + b;
        double* m = moments + WVF_M * c;
        const bool none = first[WVF_M1 * c + WVF_COUNT] == 0.0;
        for (int s = 0; s < WVF_M1; s++) m[s] = none ? 0.0 : first[WVF_M1 * c + s];
        m[WVF_WOPD2] = none ? __builtin_nan("") : central[WVF_M2 * c];
        if (!none) r2 = fmax(r2, central[WVF_M2 * c + 1]);
    }
    pupil[WVF_PUPIL_M * f + WVF_R2MAX] = r2;
    pupil[WVF_PUPIL_M * f + WVF_PUPIL_R] = ot_sqrt(r2);
}

// ---- normal equations per cell --------------------------------------------------------------------------------------
// wf_zernike_kernel (ot_wavefront.hpp) per cell: grid (list_len, chunks, pieces of the batch * K); workgroup (bx, c, piece * K + b)
// walks its piece as workgroup bx of the piece's for chunk c and band b: it reads the key byte of every entry of its share and
// the planes of the entries of its own band.  The slots of a chunk and their additions are those of wf_zernike_kernel (which
// keeps its own text: through a shared function its register allocation moves), Z by the same wf_zernike_all at (x, y) about
// the field's pupil centre, opd against the cell's mean.  part[F][K][list_len][chunks][JT + 3]; a field's last piece zeroes the
// rest of its cells' lists.
template <int JT>
__global__ __launch_bounds__(OT_RED_THREADS) void wvf_zernike_kernel(const double* __restrict__ u, const double* __restrict__ v,
                                                                     const double* __restrict__ opl, const float* __restrict__ w,
                                                                     const uint8_t* __restrict__ key, int64_t key_first, FdBatch batch,
                                                                     unsigned K, unsigned list_len, const double* __restrict__ moments,
                                                                     const double* __restrict__ pupil, double pupil_radius,
                                                                     double* __restrict__ part) {
    constexpr int S = JT + 3;
    const FdPiece P = batch.piece[blockIdx.z / K];
    const unsigned b = blockIdx.z % K, f = P.field & 0x7fffffffu;
    const int c = blockIdx.y;
    double* list = part + ((int64_t)f * K + b) * list_len * gridDim.y * S;
    const unsigned place = P.block0 + blockIdx.x;
    double* mine = list + ((int64_t)place * gridDim.y + c) * S;
    if (blockIdx.x >= P.blocks) {  // (workgroup-uniform)
        if ((P.field >> 31) && place < list_len && threadIdx.x < S) mine[threadIdx.x] = 0.0;
        return;
    }
    const double* mom = moments + ((int64_t)f * K + b) * WVF_M;
    const double mean = mom[WVF_WOPL] / mom[WVF_W];
    const bool given = pupil_radius == pupil_radius;
    const WfPupil Pp = {pupil[WVF_PUPIL_M * f + WVF_CU], pupil[WVF_PUPIL_M * f + WVF_CV],
                        given ? pupil_radius : pupil[WVF_PUPIL_M * f + WVF_PUPIL_R], given};
    double acc[S];
#pragma unroll
    for (int s = 0; s < S; s++) acc[s] = 0.0;
    const int64_t at = P.base - key_first;
    const uint32_t stride = P.blocks * OT_RED_THREADS;
    for (uint32_t i = blockIdx.x * OT_RED_THREADS + threadIdx.x; i < P.n; i += stride) {
        if (key[at + i] != b) continue;
        const float wi = w[at + i];
        if (!(wi > 0.f)) continue;
        double x, y;
        if (!wf_unit_disc(Pp, u[at + i], v[at + i], &x, &y)) continue;
        double Z[JT];
        wf_zernike_all<JT>(x, y, Z);
        double za = Z[0], zb = Z[JT - 1];
#pragma unroll
        for (int s = 1; s < (JT + 1) / 2; s++) {  // (wave-uniform selects)
            za = s == c ? Z[s] : za;
            zb = s == c ? Z[JT - 1 - s] : zb;
        }
        const double wd = (double)wi, wa = wd * za, wb = wd * zb;
#pragma unroll
        for (int s = 0; s < JT; s++) acc[s] += s >= c ? wa * Z[s] : wb * Z[JT - 1 - s];
        acc[JT] += wb * zb;
        const double opd = opl[at + i] - mean;
        acc[JT + 1] += wa * opd;
        acc[JT + 2] += wb * opd;
    }
    block_reduce_fixed<S, red_max()>(acc, mine);
}

// part[cells][list_len][chunks][JT + 3] -> out[cells][J (J + 1) / 2 + J]: wf_zernike_final_kernel per cell, grid (threads over
// the slots of the chunks, cells).  One thread per slot of a chunk adds its partials in index order and stores the sum where its
// (i, j) belongs, if that lies within J.
__global__ __launch_bounds__(OT_RED_THREADS) void wvf_zernike_final_kernel(const double* __restrict__ part, int list_len, int JT, int J,
                                                                           double* __restrict__ out) {
    const int S = JT + 3, chunks = (JT + 1) / 2, tri = J * (J + 1) / 2;
    const int q = blockIdx.x * blockDim.x + threadIdx.x;
    if (q >= chunks * S) return;
    part += (int64_t)blockIdx.y * list_len * chunks * S;
    out += (int64_t)blockIdx.y * (tri + J);
    const int c = q / S, s = q % S, a = c, b = JT - 1 - c;
    int i, j;  // j = -1: an entry of g
    if (s < JT) {
        i = s >= c ? a : b;
        j = s >= c ? s : JT - 1 - s;
    } else if (s == JT) {
        i = j = b;
    } else {
        i = s == JT + 1 ? a : b;
        j = -1;
    }
    if (a == b && (s < c || s == JT || s == JT + 2)) return;  // the middle chunk's repeats
    if (i >= J || j >= J) return;
    double r = 0.0;
    for (int k = 0; k < list_len; k++) r += part[((int64_t)k * chunks + c) * S + s];
    out[j < 0 ? tri + i : i * J - i * (i - 1) / 2 + (j - i)] = r;
}
