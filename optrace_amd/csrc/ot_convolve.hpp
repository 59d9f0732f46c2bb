// Field-dependent convolution (ot_convolve_field, DESIGN.md "Field-dependent convolution"): the direct sum
//   out[c][y][x] = sum_{b,a} sum_{dy,dx} P[b][a][dy][dx] W[b][a](y - dy, x - dx) I[c][y - dy][x - dx]
// in gather form.  One workgroup of 256 owns a tile of CF_TY x CF_TX = 16 x 128 outputs of one channel, lane (ly, lx) the 8
// neighbours x = 8 lx .. 8 lx + 7 of row ly, kept in registers.  The taps go in chunks of CF_KY x CF_KX = 16 x 32; per chunk and
// per node whose weight is not zero everywhere on the chunk's source window (31 x 159 pixels) that window is staged in LDS with W
// applied, the node's taps beside it, and every lane runs 16 rows x 4 blocks of 8 taps: one group of 8 window values and 8 taps
// from LDS, 64 fused multiply-adds.  The order of a pixel's terms is chunk (dy, then dx), node (b, then a), tap row, tap: a
// function of the shapes alone.
//
// LDS image of the window: column c sits at (c / 8) * 10 + c % 8 doubles of its row, rows CF_ROW = 224 doubles apart.  A lane
// reads aligned groups of 8 columns as four 16-byte reads; groups of neighbouring lanes are 80 bytes apart, so the 16 lanes that
// share an LDS cycle (two rows of a wave, a whole number of 256-byte bank rows apart) hit 16 different 16-byte slots.  59.8 KiB
// per workgroup: two workgroups share a CU's 160 KiB.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#define CF_THREADS 256
#define CF_TX 128
#define CF_TY 16
#define CF_KX 32
#define CF_KY 16
#define CF_WCOLS (CF_TX + CF_KX)      // window columns staged (the last one is never read)
#define CF_WROWS (CF_TY + CF_KY - 1)  // window rows
#define CF_GROUP 10                   // doubles per group of 8 columns
#define CF_ROW 224                    // doubles per window row: (CF_WCOLS / 8) * CF_GROUP = 200, up to a multiple of 32

struct ConvfArgs {
    const double* img;
    const double* psf;
    double* out;
    int32_t n_ch, ny, nx, y0, x0, ny_in, nx_in, gy, gx, py, px;
    int32_t oh, ow, tiles_x, tiles_y;
};

// t(j) = clamp((j - j0) / (n_in - 1), 0, 1) (G - 1), 0 when G = 1 or n_in = 1
__device__ __forceinline__ double convf_t(int j, int j0, int n_in, int G) {
    if (G == 1 || n_in == 1) return 0.0;
    double u = (double)(j - j0) / (double)(n_in - 1);
    u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    return u * (double)(G - 1);
}

__device__ __forceinline__ double convf_hat(double u) {
    const double h = 1.0 - fabs(u);
    return h > 0.0 ? h : 0.0;
}

// nodes b with hat(t - b) > 0 for some t in [tlo, thi]: floor(tlo) .. ceil(thi)
__device__ __forceinline__ void convf_nodes(double tlo, double thi, int G, int& lo, int& hi) {
    lo = (int)floor(tlo);
    hi = (int)ceil(thi);
    lo = lo < 0 ? 0 : lo;
    hi = hi > G - 1 ? G - 1 : hi;
}

__global__ __launch_bounds__(CF_THREADS) void convolve_field_kernel(const ConvfArgs A) {
    __shared__ __attribute__((aligned(16))) double win[CF_WROWS * CF_ROW];
    __shared__ __attribute__((aligned(16))) double taps[CF_KY * CF_KX];
    __shared__ double t_row[CF_WROWS];
    __shared__ double t_col[CF_WCOLS];

    const int tid = threadIdx.x;
    const int lx = tid & 15, ly = tid >> 4;
    unsigned tile = blockIdx.x;
    const int tx = (int)(tile % (unsigned)A.tiles_x);
    tile /= (unsigned)A.tiles_x;
    const int ty = (int)(tile % (unsigned)A.tiles_y);
    const int ch = (int)(tile / (unsigned)A.tiles_y);
    const int ox0 = tx * CF_TX, oy0 = ty * CF_TY;
    const double* __restrict__ img = A.img + (int64_t)ch * A.ny * A.nx;
    const int64_t psf_plane = (int64_t)A.py * A.px;

    double acc[8];
#pragma unroll
    for (int k = 0; k < 8; k++) acc[k] = 0.0;

    for (int dy0 = 0; dy0 < A.py; dy0 += CF_KY) {
        const int wy0 = oy0 - dy0 - (CF_KY - 1);  // source row of window row 0
        const int jlo = wy0 < 0 ? 0 : wy0, jhi = wy0 + CF_WROWS - 1 > A.ny - 1 ? A.ny - 1 : wy0 + CF_WROWS - 1;
        if (jlo > jhi) continue;  // (the same for every lane)
        const int rows = A.py - dy0 < CF_KY ? A.py - dy0 : CF_KY;
        int b_lo, b_hi;
        convf_nodes(convf_t(jlo, A.y0, A.ny_in, A.gy), convf_t(jhi, A.y0, A.ny_in, A.gy), A.gy, b_lo, b_hi);
        for (int dx0 = 0; dx0 < A.px; dx0 += CF_KX) {
            const int wx0 = ox0 - dx0 - (CF_KX - 1);
            const int ilo = wx0 < 0 ? 0 : wx0, ihi = wx0 + CF_WCOLS - 2 > A.nx - 1 ? A.nx - 1 : wx0 + CF_WCOLS - 2;
            if (ilo > ihi) continue;
            const int blocks = (A.px - dx0 < CF_KX ? A.px - dx0 + 7 : CF_KX) >> 3;
            int a_lo, a_hi;
            convf_nodes(convf_t(ilo, A.x0, A.nx_in, A.gx), convf_t(ihi, A.x0, A.nx_in, A.gx), A.gx, a_lo, a_hi);

            __syncthreads();  // the last chunk's reads of t_row, t_col are done
            if (tid < CF_WROWS) t_row[tid] = convf_t(wy0 + tid, A.y0, A.ny_in, A.gy);
            if (tid < CF_WCOLS) t_col[tid] = convf_t(wx0 + tid, A.x0, A.nx_in, A.gx);

            for (int b = b_lo; b <= b_hi; b++)
                for (int a = a_lo; a <= a_hi; a++) {
                    __syncthreads();  // t_row, t_col written; the last node's reads of win and taps are done
                    const double* __restrict__ P = A.psf + ((int64_t)b * A.gx + a) * psf_plane;
                    for (int e = tid; e < CF_KY * CF_KX; e += CF_THREADS) {
                        const int dy = dy0 + e / CF_KX, dx = dx0 + e % CF_KX;
                        taps[e] = dy < A.py && dx < A.px ? P[(int64_t)dy * A.px + dx] : 0.0;
                    }
                    // (a rolled loop: with all 20 loads of a lane issued ahead of their use the kernel took 256 VGPRs, one wave per
                    // SIMD, and 20 % longer; the second workgroup of the CU computes while this one waits here)
                    for (int e = tid; e < CF_WROWS * CF_WCOLS; e += CF_THREADS) {
                        const int r = e / CF_WCOLS, c = e % CF_WCOLS;
                        const int j = wy0 + r, i = wx0 + c;
                        double v = 0.0;
                        if (j >= 0 && j < A.ny && i >= 0 && i < A.nx)
                            v = convf_hat(t_row[r] - (double)b) * convf_hat(t_col[c] - (double)a) * img[(int64_t)j * A.nx + i];
                        win[r * CF_ROW + (c >> 3) * CF_GROUP + (c & 7)] = v;
                    }
                    __syncthreads();

                    // Output 8 lx + k and tap t of the chunk read window column 8 lx + k - t + CF_KX - 1.  In block q (taps 8 q .. 8 q + 7)
                    // that is column 8 m + (7 + k - j) with m = lx + CF_KX / 8 - 1 - q, j = t - 8 q: the groups m (lo) and m + 1 (hi).
                    for (int r = 0; r < rows; r++) {
                        const double* wrow = win + (ly - r + CF_KY - 1) * CF_ROW + (lx + CF_KX / 8) * CF_GROUP;
                        const double* trow = taps + r * CF_KX;
                        double hi[8], lo[8], p[8];
#pragma unroll
                        for (int h = 0; h < 4; h++) {
                            const double2 v = *(const double2*)(wrow + 2 * h);
                            hi[2 * h] = v.x;
                            hi[2 * h + 1] = v.y;
                        }
                        for (int q = 0; q < blocks; q++) {
                            wrow -= CF_GROUP;
#pragma unroll
                            for (int h = 0; h < 4; h++) {
                                const double2 v = *(const double2*)(wrow + 2 * h);
                                lo[2 * h] = v.x;
                                lo[2 * h + 1] = v.y;
                                const double2 t = *(const double2*)(trow + 8 * q + 2 * h);
                                p[2 * h] = t.x;
                                p[2 * h + 1] = t.y;
                            }
#pragma unroll
                            for (int j = 0; j < 8; j++)
#pragma unroll
                                for (int k = 0; k < 8; k++) {
                                    const int s = 7 + k - j;
                                    acc[k] = fma(p[j], s < 8 ? lo[s] : hi[s - 8], acc[k]);
                                }
#pragma unroll
                            for (int h = 0; h < 8; h++) hi[h] = lo[h];
                        }
                    }
                }
        }
    }

    const int y = oy0 + ly;
    if (y < A.oh) {
        double* __restrict__ o = A.out + ((int64_t)ch * A.oh + y) * A.ow;
#pragma unroll
        for (int k = 0; k < 8; k++) {
            const int x = ox0 + 8 * lx + k;
            if (x < A.ow) o[x] = acc[k];
        }
    }
}
