// C-ABI, beam footprints: records and power maps of every section of a stored trace (Raytracer.footprints).
#include "ot_footprint.hpp"
#include "ot_host.hpp"

// Workgroups per section over all launches of a pass: a launch per piece of for_ray_chunks, reduce_blocks of the piece's rays each
static int64_t fp_blocks_total(int64_t count) {
    int64_t total = 0;
    for_ray_chunks(0, count, [&](int64_t, uint32_t n) { total += reduce_blocks(n, OT_FP_BLOCKS); });
    return total;
}

static const char* fp_bad_storage(const ot_rays* rays, int64_t first, int64_t count) {
    if (!rays || !rays->p || !rays->w) return "null argument";
    if (rays->nt < 2) return "fewer than 2 sections";
    if (first < 0 || count < 0 || first + count > rays->N) return "ray range outside the storage";
    return nullptr;
}

extern "C" int64_t ot_footprint_workspace(int64_t count, int32_t nt) {
    if (count < 0 || nt < 2 || nt > OT_FP_MAX_SECTIONS) return 0;
    return fp_blocks_total(count) * nt * FP_M1;
}

extern "C" int ot_footprint_moments(const ot_rays* rays, int64_t first, int64_t count, const double* axis, double* workspace,
                                    double* records, void* stream) {
    if (!axis || !workspace || !records) return fail(OT_ERR_INVALID, "ot_footprint_moments: null argument");
    if (const char* bad = fp_bad_storage(rays, first, count)) return fail(OT_ERR_INVALID, std::string("ot_footprint_moments: ") + bad);
    if (rays->nt > OT_FP_MAX_SECTIONS) return fail(OT_ERR_UNSUPPORTED, "ot_footprint_moments: more than 65535 sections");
    if (count == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nt = rays->nt;
    const int64_t N = rays->N;
    const unsigned total = (unsigned)fp_blocks_total(count);
    const unsigned minima = (1u << FP_XMIN) | (1u << FP_YMIN) | (1u << FP_ZMIN);
    const unsigned extremes = minima | (1u << FP_XMAX) | (1u << FP_YMAX) | (1u << FP_ZMAX);

    unsigned block0 = 0;
    for_ray_chunks(first, count, [&](int64_t base, uint32_t n) {
        const unsigned blocks = reduce_blocks(n, OT_FP_BLOCKS);
        hipLaunchKernelGGL(fp_first_kernel, dim3(blocks, (unsigned)nt), dim3(OT_RED_THREADS), 0, st, rays->p + base, rays->w + base, N, nt, n,
                           block0, total, workspace);
        block0 += blocks;
    });
    hipLaunchKernelGGL(reduce_final_kernel, dim3((unsigned)nt), dim3(OT_RED_THREADS), 0, st, workspace, (int)total, (int)FP_M1, extremes,
                       minima, records, (int64_t)total * FP_M1, (int64_t)FP_M);
    block0 = 0;
    for_ray_chunks(first, count, [&](int64_t base, uint32_t n) {
        const unsigned blocks = reduce_blocks(n, OT_FP_BLOCKS);
        hipLaunchKernelGGL(fp_central_kernel, dim3(blocks, (unsigned)nt), dim3(OT_RED_THREADS), 0, st, rays->p + base, rays->w + base, N, nt, n,
                           block0, total, axis, records, workspace);
        block0 += blocks;
    });
    hipLaunchKernelGGL(reduce_final_kernel, dim3((unsigned)nt), dim3(OT_RED_THREADS), 0, st, workspace, (int)total, (int)FP_M2,
                       1u << (FP_R2MAX - FP_M1), 0u, records + FP_M1, (int64_t)total * FP_M2, (int64_t)FP_M);
    hipLaunchKernelGGL(fp_finish_kernel, grid_for(nt), dim3(256), 0, st, nt, records);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_footprint_maps(const ot_rays* rays, int64_t first, int64_t count, const double* axis, const double* records,
                                 int32_t n_px, double* maps, void* stream) {
    if (!axis || !records || !maps) return fail(OT_ERR_INVALID, "ot_footprint_maps: null argument");
    if (const char* bad = fp_bad_storage(rays, first, count)) return fail(OT_ERR_INVALID, std::string("ot_footprint_maps: ") + bad);
    if (rays->nt > OT_FP_MAX_SECTIONS) return fail(OT_ERR_UNSUPPORTED, "ot_footprint_maps: more than 65535 sections");
    if (n_px < 1 || n_px > OT_FP_MAX_PX) return fail(OT_ERR_UNSUPPORTED, "ot_footprint_maps: n_px outside 1 .. 1024");
    if (count == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    const int nt = rays->nt, cells = n_px * n_px;
    for_ray_chunks(first, count, [&](int64_t base, uint32_t n) {
        const HistShape hs = hist_shape(n, (size_t)cells * sizeof(double));
        hipLaunchKernelGGL(fp_map_kernel, dim3(hs.grid.x, (unsigned)nt), hs.block, hs.lds, (hipStream_t)stream, rays->p + base, rays->w + base,
                           rays->N, nt, n, axis, records, (int)n_px, hs.lds ? cells : 0, maps);
    });
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
