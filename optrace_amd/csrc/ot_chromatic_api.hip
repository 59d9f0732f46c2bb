// C-ABI, chromatic analysis: focus sums and plane records per band of wavelengths of a stored trace (Raytracer.chromatic_analysis).
#include "ot_chromatic.hpp"
#include "ot_host.hpp"

// Workgroups per band over all launches of a pass: a launch per piece of for_ray_chunks, reduce_blocks of the piece's rays each
static int64_t ch_blocks_total(int64_t count) {
    int64_t total = 0;
    for_ray_chunks(0, count, [&](int64_t, uint32_t n) { total += reduce_blocks(n, OT_CHROM_BLOCKS); });
    return total;
}

static bool ch_bands_ok(int32_t n_bands) { return n_bands >= 1 && n_bands <= OT_CHROM_MAX_BANDS; }
static std::string ch_bad_bands(const char* who) { return std::string(who) + ": n_bands outside 1 .. " + std::to_string(OT_CHROM_MAX_BANDS); }

extern "C" int64_t ot_chromatic_workspace(int64_t count, int32_t n_bands) {
    if (count < 0 || !ch_bands_ok(n_bands)) return 0;
    return ch_blocks_total(count) * n_bands * WFF_M;
}

extern "C" int ot_chromatic_focus(const ot_rays* rays, int64_t first, int64_t count, int32_t section, const uint8_t* key, int32_t n_bands,
                                  const double* origin, double* workspace, double* sums, void* stream) {
    if (!key || !origin || !workspace || !sums) return fail(OT_ERR_INVALID, "ot_chromatic_focus: null argument");
    if (const char* bad = bad_section_sphere(rays, first, count, section, false, nullptr, 0.0))
        return fail(OT_ERR_INVALID, std::string("ot_chromatic_focus: ") + bad);
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
        return fail(OT_ERR_INVALID, "ot_chromatic_focus: origin not finite");
    if (!ch_bands_ok(n_bands)) return fail(OT_ERR_UNSUPPORTED, ch_bad_bands("ot_chromatic_focus"));
    if (count == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned total = (unsigned)ch_blocks_total(count);
    unsigned block0 = 0;
    for_ray_chunks(first, count, [&](int64_t base, uint32_t n) {
        const unsigned blocks = reduce_blocks(n, OT_CHROM_BLOCKS);
        hipLaunchKernelGGL(ch_focus_kernel, dim3(blocks, (unsigned)n_bands), dim3(OT_RED_THREADS), 0, st, rays->p + base, rays->w + base,
                           key + (base - first), rays->N, (int)rays->nt, (int)section, n, block0, total, origin[0], origin[1], origin[2],
                           workspace);
        block0 += blocks;
    });
    hipLaunchKernelGGL(reduce_final_kernel, dim3((unsigned)n_bands), dim3(OT_RED_THREADS), 0, st, workspace, (int)total, (int)WFF_M, 0u, 0u,
                       sums, (int64_t)total * WFF_M, (int64_t)WFF_M);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_chromatic_plane(const ot_rays* rays, int64_t first, int64_t count, int32_t section, const uint8_t* key, int32_t n_bands,
                                  double z, double* workspace, double* records, void* stream) {
    if (!key || !workspace || !records || (rays && !rays->wl)) return fail(OT_ERR_INVALID, "ot_chromatic_plane: null argument");
    if (const char* bad = bad_section_sphere(rays, first, count, section, false, nullptr, 0.0))
        return fail(OT_ERR_INVALID, std::string("ot_chromatic_plane: ") + bad);
    if (!std::isfinite(z)) return fail(OT_ERR_INVALID, "ot_chromatic_plane: z not finite");
    if (!ch_bands_ok(n_bands)) return fail(OT_ERR_UNSUPPORTED, ch_bad_bands("ot_chromatic_plane"));
    if (count == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nt = rays->nt, k = section;
    const int64_t N = rays->N;
    const unsigned total = (unsigned)ch_blocks_total(count), K = (unsigned)n_bands;

    unsigned block0 = 0;
    for_ray_chunks(first, count, [&](int64_t base, uint32_t n) {
        const unsigned blocks = reduce_blocks(n, OT_CHROM_BLOCKS);
        hipLaunchKernelGGL(ch_first_kernel, dim3(blocks, K), dim3(OT_RED_THREADS), 0, st, rays->p + base, rays->w + base, rays->wl + base,
                           key + (base - first), N, nt, k, n, block0, total, z, workspace);
        block0 += blocks;
    });
    hipLaunchKernelGGL(reduce_final_kernel, dim3(K), dim3(OT_RED_THREADS), 0, st, workspace, (int)total, (int)CH_M1, 0u, 0u, records,
                       (int64_t)total * CH_M1, (int64_t)CH_M);
    block0 = 0;
    for_ray_chunks(first, count, [&](int64_t base, uint32_t n) {
        const unsigned blocks = reduce_blocks(n, OT_CHROM_BLOCKS);
        hipLaunchKernelGGL(ch_central_kernel, dim3(blocks, K), dim3(OT_RED_THREADS), 0, st, rays->p + base, rays->w + base,
                           key + (base - first), N, nt, k, n, block0, total, z, records, workspace);
        block0 += blocks;
    });
    hipLaunchKernelGGL(reduce_final_kernel, dim3(K), dim3(OT_RED_THREADS), 0, st, workspace, (int)total, (int)CH_M2,
                       1u << (CH_R2MAX - CH_M1), 0u, records + CH_M1, (int64_t)total * CH_M2, (int64_t)CH_M);
    hipLaunchKernelGGL(ch_finish_kernel, grid_for(n_bands), dim3(256), 0, st, (int)n_bands, records);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
