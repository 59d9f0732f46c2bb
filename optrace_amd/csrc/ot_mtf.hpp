// Geometric MTF across field and focus (Raytracer.mtf_analysis): per field point, band of wavelengths, plane and spatial frequency
// the OTF sums of the ray lines of section k along the tangential direction t of the field and across it.  Definition: DESIGN.md
// "MTF analysis"; the layout of the sums: include/optrace_amd.h.  The rays, their test and their lines (a, m) are those of the field
// analysis (ot_field_ray.hpp); the means are the quotients of the first-pass slots of the `ot_field_sums` record of the cell.
// Shape: that of spot_otf_kernel, 32 sums per lane (36 for three bands).  A workgroup (x, piece, group of bands and tile) walks the rays of ONE piece of
// ONE field as workgroup x of the piece's.  A lane takes its ray when the ray's band is one of the KB bands of the group, forms
// the sine and cosine of a tile of about 8 / KB (plane, frequency) pairs, both directions, and adds them with the ray's weight to the
// sums of the ray's band and with the weight 0 to those of the other bands of the group: rays of different bands keep the lanes
// of one wave busy side by side, and which lane adds which ray where follows from the ray's place alone.  A wave none of whose 64
// rays is of the group goes on at once.  block_reduce_fixed folds the lanes, the last kernel adds a field's partials in their
// order: every addition's place follows from the field's count and (K, Z, Q).
// Included by ot_mtf_api.hip alone.
#pragma once
#include "ot_block_reduce.hpp"
#include "ot_device.hpp"
#include "ot_field_ray.hpp"

#define MT_PAIRS 8    // (plane, frequency) pairs a lane holds, over the bands of its group (9 for three bands)
#define MT_PIECES 32  // pieces a launch takes

// Bands a workgroup takes side by side, pairs of a tile and doubles of a partial [KB][re t | im t | re s | im s][TILE] for K bands
// in all: K itself up to 4, where every ray of a band finds its band in the one group; 4 beyond.  Three bands, the three lines of
// most lens data, take tiles of 3 pairs, 36 sums: the ray's loads and line terms are spread over one pair more.
constexpr int mt_group(int K) { return K < 4 ? K : 4; }
constexpr int mt_tile(int KB) { return KB == 3 ? 3 : MT_PAIRS / KB; }
constexpr int mt_cell(int KB) { return KB * 4 * mt_tile(KB); }

// A piece is a field's range, or 2^28 rays of it: 32-bit offsets from `base`.
struct MtPiece {
    int64_t base;     // first ray of the piece in the storage
    uint32_t n;       // its rays, at most 2^28
    uint32_t blocks;  // workgroups that walk it
    uint32_t block0;  // place of its first workgroup's partial in the field's list
    uint32_t field;
    double tx, ty;    // the field's tangential direction
};
struct MtBatch {
    MtPiece piece[MT_PIECES];
};
struct MtPlanes {
    double zeta[OT_MTF_MAX_PLANES];
};
struct MtLists {
    uint32_t blocks[OT_FIELD_MAX_FIELDS];  // partials every field's list holds
};

// part[F][list_len][groups][tiles][CELL]; grid (most workgroups of a piece of the batch, pieces of the batch, groups * tiles).
// records[F][K][OT_FIELD_M]: the records of ot_field_sums.  Four waves per SIMD (128 VGPRs): the sums take up to 64 of them.
template <int KB>
__global__ __launch_bounds__(OT_RED_THREADS, 4) void mt_sums_kernel(const double* __restrict__ p, const float* __restrict__ w,
                                                                    const uint8_t* __restrict__ key, int64_t key_first, int64_t N, int nt,
                                                                    int k, MtBatch batch, MtPlanes planes, unsigned K, unsigned Z,
                                                                    unsigned Q, unsigned tiles, unsigned list_len, double ox, double oy,
                                                                    double oz, const double* __restrict__ records,
                                                                    const double* __restrict__ freq, double* __restrict__ part) {
    constexpr int TILE = mt_tile(KB), CELL = mt_cell(KB);
    __shared__ double mean[OT_CHROM_MAX_BANDS][4];
    const MtPiece P = batch.piece[blockIdx.y];
    if (blockIdx.x >= P.blocks) return;  // (workgroup-uniform)
    const unsigned groups = (K + KB - 1) / KB, g = blockIdx.z / tiles, tile = blockIdx.z % tiles, b0 = g * KB;
    const double* rec = records + (int64_t)P.field * K * OT_FIELD_M;
    if (threadIdx.x < K * 4) {
        // the means: the same IEEE quotients as the central pass of the field analysis and the host form from the record (no ray
        // in the sums: NaN, and nothing reads it)
        const double* m = rec + (threadIdx.x / 4) * OT_FIELD_M;
        mean[threadIdx.x / 4][threadIdx.x % 4] = m[2 + threadIdx.x % 4] / m[0];
    }
    __syncthreads();
    double v[CELL];  // [KB][re t | im t | re s | im s][TILE]
#pragma unroll
    for (int j = 0; j < CELL; j++) v[j] = 0.0;
    const double tx = P.tx, ty = P.ty, sx = -ty, sy = tx;
    double zt[TILE], nu[TILE];
#pragma unroll
    for (int i = 0; i < TILE; i++) {  // (wave-uniform; the tail repeats the last pair)
        const unsigned at = tile * TILE + i < Z * Q ? tile * TILE + i : Z * Q - 1;
        zt[i] = planes.zeta[at / Q];
        nu[i] = freq[at % Q];
    }
    const FdSection S = fd_section(p + P.base, w + P.base, nullptr, key + (P.base - key_first), N, nt, k);
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t stride = P.blocks * OT_RED_THREADS;  // (at most 2^18 beyond n <= 2^28: no wrap)
    for (uint32_t r0 = blockIdx.x * OT_RED_THREADS + wave * 64; r0 < P.n; r0 += stride) {  // (wave-uniform)
        const uint32_t r = r0 + lane;
        const unsigned kb = r < P.n ? S.key[r] : FD_NO_BAND;
        const bool mine = kb >= b0 && kb < b0 + KB && kb < K;
        if (!__ballot(mine)) continue;  // (wave-uniform)
        FdRay q;
        if (!mine || !fd_ray(S, r, ox, oy, oz, q) || q.dz == 0.0) continue;
        const double dax = q.ax - mean[kb][0], day = q.ay - mean[kb][1], dmx = q.mx - mean[kb][2], dmy = q.my - mean[kb][3];
        const double al_t = tx * dax + ty * day, mu_t = tx * dmx + ty * dmy;
        const double al_s = sx * dax + sy * day, mu_s = sx * dmx + sy * dmy;
        double wb[KB];  // the ray's weight for its band, 0 for the others: w cs + 0 cs' adds up to the bits of w cs alone
#pragma unroll
        for (int j = 0; j < KB; j++) wb[j] = kb == b0 + j ? q.w : 0.0;
#pragma unroll
        for (int i = 0; i < TILE; i++) {
            double tt = nu[i] * (al_t + zt[i] * mu_t), ts = nu[i] * (al_s + zt[i] * mu_s), sn_t, cs_t, sn_s, cs_s;
            tt -= rint(tt);  // (in turns: sincospi_small sees |2 t| <= 1 whatever nu and e are)
            ts -= rint(ts);
            sincospi_small(2.0 * tt, &sn_t, &cs_t);
            sincospi_small(2.0 * ts, &sn_s, &cs_s);
#pragma unroll
            for (int j = 0; j < KB; j++) {
                v[(4 * j + 0) * TILE + i] += wb[j] * cs_t;
                v[(4 * j + 1) * TILE + i] -= wb[j] * sn_t;
                v[(4 * j + 2) * TILE + i] += wb[j] * cs_s;
                v[(4 * j + 3) * TILE + i] -= wb[j] * sn_s;
            }
        }
    }
    block_reduce_fixed<CELL, red_max()>(
        v, part + ((((int64_t)P.field * list_len + P.block0 + blockIdx.x) * groups + g) * tiles + tile) * CELL);
}

// part[F][list_len][groups][tiles][CELL] -> sums[F][K][Z][Q][4]: a thread per sum adds the partials of its field's list in index
// order.  KB, TILE: the group and the tile of the kernel that wrote the partials
__global__ __launch_bounds__(OT_RED_THREADS) void mt_final_kernel(const double* __restrict__ part, MtLists lists, int64_t total,
                                                                  unsigned K, unsigned Z, unsigned Q, unsigned KB, unsigned TILE,
                                                                  unsigned tiles, unsigned list_len, double* __restrict__ sums) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total) return;
    const unsigned c = (unsigned)(j % 4), pair = (unsigned)(j / 4 % (Z * Q)), cell = (unsigned)(j / 4 / (Z * Q)), f = cell / K, b = cell % K;
    const unsigned groups = (K + KB - 1) / KB, CELL = KB * 4 * TILE;
    const int64_t step = (int64_t)groups * tiles * CELL;
    const double* col = part + (int64_t)f * list_len * step + ((int64_t)(b / KB) * tiles + pair / TILE) * CELL +
                        (4 * (b % KB) + c) * TILE + pair % TILE;
    double r = 0.0;
    for (unsigned at = 0; at < lists.blocks[f]; at++) r += col[at * step];
    sums[j] = r;
}
