// C-ABI, ray fans: transverse aberration per ray, band records and the binned pupil cuts of a stored trace (Raytracer.ray_fans).
#include "ot_fans.hpp"
#include "ot_host.hpp"

// Workgroups per band over all launches of a pass: a launch per piece of for_ray_chunks, reduce_blocks of the piece's rays each
static int64_t fan_blocks_total(int64_t count) {
    int64_t total = 0;
    for_ray_chunks(0, count, [&](int64_t, uint32_t n) { total += reduce_blocks(n, OT_CHROM_BLOCKS); });
    return total;
}

static bool fan_bands_ok(int32_t n_bands) { return n_bands >= 1 && n_bands <= OT_CHROM_MAX_BANDS; }
static std::string fan_bad_bands(const char* who) { return std::string(who) + ": n_bands outside 1 .. " + std::to_string(OT_CHROM_MAX_BANDS); }

extern "C" int64_t ot_fans_workspace(int64_t count, int32_t n_bands) {
    if (count < 0 || !fan_bands_ok(n_bands)) return 0;
    return fan_blocks_total(count) * n_bands * FAN_M1;
}

extern "C" int ot_fans_transverse(const ot_rays* rays, int64_t first, int64_t count, int32_t section, const double* focus, float* w,
                                  double* ex, double* ey, int64_t* n_parallel, void* stream) {
    if (!focus || !w || !ex || !ey || !n_parallel) return fail(OT_ERR_INVALID, "ot_fans_transverse: null argument");
    if (const char* bad = bad_section_sphere(rays, first, count, section, false, nullptr, 0.0))
        return fail(OT_ERR_INVALID, std::string("ot_fans_transverse: ") + bad);
    if (!std::isfinite(focus[0]) || !std::isfinite(focus[1]) || !std::isfinite(focus[2]))
        return fail(OT_ERR_INVALID, "ot_fans_transverse: focus not finite");
    if (count == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(n_parallel, 0, sizeof(int64_t), st));
    for_ray_chunks(first, count, [&](int64_t base, uint32_t n) {
        const int64_t at = base - first;
        hipLaunchKernelGGL(fan_transverse_kernel, grid_for(n), dim3(OT_RED_THREADS), 0, st, rays->p + base, rays->N, (int)rays->nt,
                           (int)section, n, focus[0], focus[1], focus[2], w + at, ex + at, ey + at, (unsigned long long*)n_parallel);
    });
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_fans_bands(int64_t count, const double* opl, const double* ex, const double* ey, const float* w, const float* wl,
                             const uint8_t* key, int32_t n_bands, double* workspace, double* records, void* stream) {
    if (count < 0 || !opl || !ex || !ey || !w || !wl || !key || !workspace || !records)
        return fail(OT_ERR_INVALID, "ot_fans_bands: null argument or count below 0");
    if (!fan_bands_ok(n_bands)) return fail(OT_ERR_UNSUPPORTED, fan_bad_bands("ot_fans_bands"));
    if (count == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned total = (unsigned)fan_blocks_total(count), K = (unsigned)n_bands;
    auto planes = [&](int64_t at) { return FanPlanes{key + at, w + at, wl + at, opl + at, ex + at, ey + at}; };

    unsigned block0 = 0;
    for_ray_chunks(0, count, [&](int64_t base, uint32_t n) {
        const unsigned blocks = reduce_blocks(n, OT_CHROM_BLOCKS);
        hipLaunchKernelGGL(fan_first_kernel, dim3(blocks, K), dim3(OT_RED_THREADS), 0, st, planes(base), n, block0, total, workspace);
        block0 += blocks;
    });
    hipLaunchKernelGGL(reduce_final_kernel, dim3(K), dim3(OT_RED_THREADS), 0, st, workspace, (int)total, (int)FAN_M1,
                       (1u << FAN_OPL_MIN) | (1u << FAN_OPL_MAX), 1u << FAN_OPL_MIN, records, (int64_t)total * FAN_M1, (int64_t)FAN_M);
    block0 = 0;
    for_ray_chunks(0, count, [&](int64_t base, uint32_t n) {
        const unsigned blocks = reduce_blocks(n, OT_CHROM_BLOCKS);
        hipLaunchKernelGGL(fan_central_kernel, dim3(blocks, K), dim3(OT_RED_THREADS), 0, st, planes(base), n, block0, total, records,
                           workspace);
        block0 += blocks;
    });
    hipLaunchKernelGGL(reduce_final_kernel, dim3(K), dim3(OT_RED_THREADS), 0, st, workspace, (int)total, (int)FAN_M2,
                       1u << (FAN_R2MAX - FAN_M1), 0u, records + FAN_M1, (int64_t)total * FAN_M2, (int64_t)FAN_M);
    hipLaunchKernelGGL(fan_finish_kernel, grid_for(n_bands), dim3(256), 0, st, (int)n_bands, records);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_fans_bins(int64_t count, const double* u, const double* v, const double* opl, const double* ex, const double* ey,
                            const float* w, const uint8_t* key, const double* moments, double pupil_radius, const double* records,
                            int32_t n_bands, int32_t n_bins, double slab, double* out, void* stream) {
    if (count < 0 || !u || !v || !opl || !ex || !ey || !w || !key || !moments || !records || !out)
        return fail(OT_ERR_INVALID, "ot_fans_bins: null argument or count below 0");
    if (!fan_bands_ok(n_bands)) return fail(OT_ERR_UNSUPPORTED, fan_bad_bands("ot_fans_bins"));
    if (n_bins < 1 || n_bins > OT_FAN_MAX_BINS)
        return fail(OT_ERR_UNSUPPORTED, "ot_fans_bins: n_bins outside 1 .. " + std::to_string(OT_FAN_MAX_BINS));
    if (!(slab > 0.0 && slab <= 1.0)) return fail(OT_ERR_INVALID, "ot_fans_bins: slab not in (0, 1]");
    if (!std::isnan(pupil_radius) && !(std::isfinite(pupil_radius) && pupil_radius > 0.0))
        return fail(OT_ERR_INVALID, "ot_fans_bins: pupil radius neither NaN nor above zero");
    if (count == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    const int cells = n_bands * 2 * n_bins * FB_M;
    const HistShape hs = hist_shape(count, (size_t)cells * sizeof(double));
    hipLaunchKernelGGL(fan_bins_kernel, hs.grid, hs.block, hs.lds, (hipStream_t)stream, count, u, v, opl, ex, ey, w, key, moments,
                       pupil_radius, records, (int)n_bands, (int)n_bins, slab, hs.lds ? cells : 0, out);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
