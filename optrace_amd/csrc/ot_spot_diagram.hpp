// Spot diagrams across field and focus (Raytracer.spot_diagram): per field point, band of wavelengths and plane where the ray lines
// of section k land about a centre, as a power map of n_px x n_px cells with its counts, and the largest and the power-weighted
// mean squared distance from the centre.  Definition: DESIGN.md "Spot diagrams"; include/optrace_amd.h, ot_spotdiag_*.  The rays,
// their test and their lines (a, m) are those of the field analysis (ot_field_ray.hpp).
//   extent  the frame of mt_sums_kernel: a workgroup (x, piece, group of bands and tile of planes) walks the rays of ONE piece of ONE
//           field; a lane holds, for the KB bands of its group and the planes of its tile, the largest |e|^2 and sum w |e|^2, its
//           ray adding to its own band alone.  block_reduce_fixed folds the lanes, the last kernel folds a field's partials in
//           index order: the same bits on every call, whatever the other fields are.
//   maps    a workgroup holds a chunk of whole (band, plane) tiles in LDS -- the f64 cells, the power and the count outside, the
//           tile's centre and zeta -- and walks the rays of one piece part: a lane forms its ray line once and walks the planes
//           of its band that lie in the chunk, binning with LDS atomics; the cells that are not zero and the counters are flushed
//           with one global atomic each.  Chunks go over gridDim.z.  When one tile alone exceeds the LDS budget the cells are
//           added to global memory directly, the counters of all tiles still in LDS, in one chunk.
// Included by ot_spot_diagram_api.hip alone.
#pragma once
#include "ot_block_reduce.hpp"
#include "ot_device.hpp"
#include "ot_field_ray.hpp"

#define SD_PAIRS 8         // (band, plane) pairs a lane of the extent pass holds (9 for three bands)
#define SD_PIECES 32       // pieces a launch takes
#define SD_MAP_THREADS 1024
#define SD_TILE_AUX 40     // bytes a tile takes in LDS beside its cells: outside power, centre (2), zeta, two 32-bit counters

// Bands a workgroup of the extent pass takes side by side, planes of its tile and doubles of a partial [KB][max | sum][TILE]:
// the grouping of the MTF pass
constexpr int sd_group(int K) { return K < 4 ? K : 4; }
constexpr int sd_tile(int KB) { return KB == 3 ? 3 : SD_PAIRS / KB; }
constexpr int sd_cell(int KB) { return KB * 2 * sd_tile(KB); }
constexpr red_mask sd_max_mask(int KB) {  // the rows [j][0][.] of the partial are maxima
    red_mask m = 0;
    for (int j = 0; j < KB; j++)
        for (int i = 0; i < sd_tile(KB); i++) m |= (red_mask)1 << (2 * j * sd_tile(KB) + i);
    return m;
}

// A piece is a field's range, or 2^28 rays of it: 32-bit offsets from `base`.
struct SdPiece {
    int64_t base;     // first ray of the piece in the storage
    uint32_t n;       // its rays, at most 2^28
    uint32_t blocks;  // workgroups that walk it
    uint32_t block0;  // extent pass: place of its first workgroup's partial in the field's list
    uint32_t field;
};
struct SdBatch {
    SdPiece piece[SD_PIECES];
};
struct SdPlanes {
    double zeta[OT_MTF_MAX_PLANES];
};
struct SdLists {
    uint32_t blocks[OT_FIELD_MAX_FIELDS];  // partials every field's list holds
};

// e = (a + zeta m) - centre, one f64 operation each (no fused product: -ffp-contract=off)
OT_DEV void sd_offset(const FdRay& q, double zeta, double cx, double cy, double& ex, double& ey) {
    const double x = q.ax + zeta * q.mx, y = q.ay + zeta * q.my;
    ex = x - cx;
    ey = y - cy;
}

// part[F][list_len][groups][tiles][CELL]; grid (most workgroups of a piece of the batch, pieces of the batch, groups * tiles).
// centre[F][K][Z][2], relative to the origin's xy.
template <int KB>
__global__ __launch_bounds__(OT_RED_THREADS) void sd_extent_kernel(const double* __restrict__ p, const float* __restrict__ w,
                                                                   const uint8_t* __restrict__ key, int64_t key_first, int64_t N, int nt,
                                                                   int k, SdBatch batch, SdPlanes planes, unsigned K, unsigned Z,
                                                                   unsigned tiles, unsigned list_len, double ox, double oy, double oz,
                                                                   const double* __restrict__ centre, double* __restrict__ part) {
    constexpr int TILE = sd_tile(KB), CELL = sd_cell(KB);
    __shared__ double cen[KB][TILE][2];
    const SdPiece P = batch.piece[blockIdx.y];
    if (blockIdx.x >= P.blocks) return;  // (workgroup-uniform)
    const unsigned groups = (K + KB - 1) / KB, g = blockIdx.z / tiles, tile = blockIdx.z % tiles, b0 = g * KB;
    if (threadIdx.x < KB * TILE * 2) {  // (the tail of the bands and of the planes repeats the last one: inside the array, and never stored)
        const unsigned c = threadIdx.x % 2, i = threadIdx.x / 2 % TILE, j = threadIdx.x / 2 / TILE;
        const unsigned b = b0 + j < K ? b0 + j : K - 1, z = tile * TILE + i < Z ? tile * TILE + i : Z - 1;
        cen[j][i][c] = centre[(((int64_t)P.field * K + b) * Z + z) * 2 + c];
    }
    __syncthreads();
    double v[CELL];  // [KB][max |e|^2 | sum w |e|^2][TILE]
#pragma unroll
    for (int j = 0; j < CELL; j++) v[j] = 0.0;
    double zt[TILE];
#pragma unroll
    for (int i = 0; i < TILE; i++) zt[i] = planes.zeta[tile * TILE + i < Z ? tile * TILE + i : Z - 1];  // (wave-uniform)
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
        const unsigned own = kb - b0;
#pragma unroll
        for (int i = 0; i < TILE; i++) {
            double ex, ey;
            sd_offset(q, zt[i], cen[own][i][0], cen[own][i][1], ex, ey);
            const double r2 = ex * ex + ey * ey, wr2 = q.w * r2;
#pragma unroll
            for (int j = 0; j < KB; j++) {  // (a select per band, no product with 0: a ray far away or of no number stays in its band)
                v[(2 * j + 0) * TILE + i] = fmax(v[(2 * j + 0) * TILE + i], own == (unsigned)j ? r2 : 0.0);
                v[(2 * j + 1) * TILE + i] += own == (unsigned)j ? wr2 : 0.0;
            }
        }
    }
    block_reduce_fixed<CELL, sd_max_mask(KB)>(
        v, part + ((((int64_t)P.field * list_len + P.block0 + blockIdx.x) * groups + g) * tiles + tile) * CELL);
}

// part[F][list_len][groups][tiles][CELL] -> ext[F][K][Z][2]: a thread per value folds the partials of its field's list in index
// order.  KB, TILE: the group and the tile of the kernel that wrote the partials
__global__ __launch_bounds__(OT_RED_THREADS) void sd_extent_final_kernel(const double* __restrict__ part, SdLists lists, int64_t total,
                                                                         unsigned K, unsigned Z, unsigned KB, unsigned TILE,
                                                                         unsigned tiles, unsigned list_len, double* __restrict__ ext) {
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= total) return;
    const unsigned c = (unsigned)(j % 2), z = (unsigned)(j / 2 % Z), cell = (unsigned)(j / 2 / Z), f = cell / K, b = cell % K;
    const unsigned groups = (K + KB - 1) / KB, CELL = KB * 2 * TILE;
    const int64_t step = (int64_t)groups * tiles * CELL;
    const double* col = part + (int64_t)f * list_len * step + ((int64_t)(b / KB) * tiles + z / TILE) * CELL +
                        (2 * (b % KB) + c) * TILE + z % TILE;
    double r = 0.0;
    if (c == 0)
        for (unsigned at = 0; at < lists.blocks[f]; at++) r = fmax(r, col[at * step]);
    else
        for (unsigned at = 0; at < lists.blocks[f]; at++) r += col[at * step];
    ext[j] = r;
}

// maps[F][K][Z][n_px][n_px] += w; counts[F][K][Z][2] += (binned, outside); outside_power[F][K][Z] += w of the rays outside.
// Grid (most workgroups of a piece of the batch, pieces of the batch, chunks); chunk c holds the tiles c T .. c T + T - 1 of the K Z
// (band, plane) tiles of the piece's field.  Dynamic LDS: [cells_lds ? T n_px^2 : 0] cells | [T] outside power | [T][2] centre |
// [T] zeta | [T] rays outside (32 bits: a workgroup walks 2^28 rays at the most).  cells_lds = 0: the cells are added to `maps` directly.
__global__ __launch_bounds__(SD_MAP_THREADS) void sd_map_kernel(const double* __restrict__ p, const float* __restrict__ w,
                                                                const uint8_t* __restrict__ key, int64_t key_first, int64_t N, int nt, int k,
                                                                SdBatch batch, SdPlanes planes, unsigned K, unsigned Z, unsigned T,
                                                                int n_px, int cells_lds, double ox, double oy, double oz,
                                                                const double* __restrict__ centre, double size, double* __restrict__ maps,
                                                                unsigned long long* __restrict__ counts, double* __restrict__ outside_power) {
    extern __shared__ double sd_sh[];
    __shared__ unsigned walked[OT_CHROM_MAX_BANDS];  // rays of a band this workgroup took: on every plane the binned and the outside ones
    const SdPiece P = batch.piece[blockIdx.y];
    if (blockIdx.x >= P.blocks) return;  // (workgroup-uniform)
    const unsigned cells = (unsigned)n_px * (unsigned)n_px, t0 = blockIdx.z * T, t1 = t0 + T < K * Z ? t0 + T : K * Z, nT = t1 - t0;
    const unsigned n_lds = cells_lds ? nT * cells : 0;  // (T n_px^2 within the LDS: below 2^15)
    double* cell_sh = sd_sh;
    double* out_sh = sd_sh + (cells_lds ? T * cells : 0);
    double* cen_sh = out_sh + T;
    double* zeta_sh = cen_sh + 2 * T;
    unsigned* gone_sh = (unsigned*)(zeta_sh + T);
    const int64_t tile0 = (int64_t)P.field * K * Z + t0;  // the chunk's first tile among all
    for (unsigned c = threadIdx.x; c < n_lds; c += SD_MAP_THREADS) cell_sh[c] = 0.0;
    for (unsigned i = threadIdx.x; i < nT; i += SD_MAP_THREADS) {
        out_sh[i] = 0.0;
        gone_sh[i] = 0u;
        cen_sh[2 * i] = centre[(tile0 + i) * 2];
        cen_sh[2 * i + 1] = centre[(tile0 + i) * 2 + 1];
        zeta_sh[i] = planes.zeta[(t0 + i) % Z];
    }
    if (threadIdx.x < OT_CHROM_MAX_BANDS) walked[threadIdx.x] = 0u;
    __syncthreads();
    const unsigned b_lo = t0 / Z, b_hi = (t1 - 1) / Z;  // the bands with a tile in the chunk
    const double fn = (double)n_px, scale = fn / size, half = 0.5 * fn;
    const FdSection S = fd_section(p + P.base, w + P.base, nullptr, key + (P.base - key_first), N, nt, k);
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t stride = P.blocks * SD_MAP_THREADS;  // (at most 2^20 beyond n <= 2^28: no wrap)
    for (uint32_t r0 = blockIdx.x * SD_MAP_THREADS + wave * 64; r0 < P.n; r0 += stride) {  // (wave-uniform)
        const uint32_t r = r0 + lane;
        const unsigned kb = r < P.n ? S.key[r] : FD_NO_BAND;
        const bool mine = kb >= b_lo && kb <= b_hi && kb < K;
        if (!__ballot(mine)) continue;  // (wave-uniform)
        FdRay q;
        if (!mine || !fd_ray(S, r, ox, oy, oz, q) || q.dz == 0.0) continue;
        atomicAdd(&walked[kb], 1u);
        const unsigned first = kb * Z > t0 ? kb * Z : t0, last = (kb + 1) * Z < t1 ? (kb + 1) * Z : t1;
        for (unsigned t = first; t < last; t++) {
            const unsigned i = t - t0;
            double ex, ey;
            sd_offset(q, zeta_sh[i], cen_sh[2 * i], cen_sh[2 * i + 1], ex, ey);
            const double col = floor(ex * scale + half), row = floor(ey * scale + half);
            if (col >= 0.0 && col < fn && row >= 0.0 && row < fn) {  // (no number: outside; nothing is clamped into the map)
                const unsigned at = (unsigned)row * (unsigned)n_px + (unsigned)col;
                if (cells_lds)
                    unsafeAtomicAdd(&cell_sh[i * cells + at], q.w);
                else
                    unsafeAtomicAdd(&maps[(tile0 + i) * (int64_t)cells + at], q.w);
            } else {
                atomicAdd(&gone_sh[i], 1u);
                unsafeAtomicAdd(&out_sh[i], q.w);
            }
        }
    }
    __syncthreads();
    double* map = maps + tile0 * (int64_t)cells;  // (the chunk's tiles follow each other in `maps` as in LDS)
    for (unsigned c = threadIdx.x; c < n_lds; c += SD_MAP_THREADS) {
        const double s = cell_sh[c];
        if (s != 0.0) unsafeAtomicAdd(&map[c], s);
    }
    for (unsigned i = threadIdx.x; i < nT; i += SD_MAP_THREADS) {
        const unsigned all = walked[(t0 + i) / Z], gone = gone_sh[i];
        if (all != gone) atomicAdd(&counts[(tile0 + i) * 2], (unsigned long long)(all - gone));
        if (gone) {
            atomicAdd(&counts[(tile0 + i) * 2 + 1], (unsigned long long)gone);
            unsafeAtomicAdd(&outside_power[tile0 + i], out_sh[i]);
        }
    }
}
