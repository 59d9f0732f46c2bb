// C-ABI, Huygens point spread function: ray records from the storage and the wavefront planes, and their coherent sum over an
// image plane (Raytracer.huygens_psf).
#include "ot_host.hpp"
#include "ot_psf.hpp"

extern "C" int64_t ot_psf_workspace(int64_t n, int32_t n_px) {
    if (n < 0 || n_px < 1 || n_px > OT_PSF_MAX_PX) return 0;
    const PsfShape s = psf_shape(n, n_px);
    return s.chunks * s.stride;
}

extern "C" int ot_psf_rays(const ot_rays* rays, int64_t first, int64_t count, int32_t section, const double* focus, double radius,
                           const double* opl, const double* moments, double* rec, void* stream) {
    if ((rays && !rays->wl) || !focus || !opl || !moments || !rec) return fail(OT_ERR_INVALID, "ot_psf_rays: null argument");
    if (const char* bad = bad_section_sphere(rays, first, count, section, true, focus, radius))
        return fail(OT_ERR_INVALID, std::string("ot_psf_rays: ") + bad);
    if (count == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(psf_rays_kernel, grid_for(count), dim3(OT_PSF_THREADS), 0, (hipStream_t)stream, *rays, first, count, (int)section,
                       focus[0], focus[1], focus[2], radius, opl, moments, rec);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

// The launches that ot_psf_sum and ot_psf_stack share.  Band b gets ceil(n_b / chunk_len) chunks: for the one band of ot_psf_sum
// the chunks of psf_shape that hold a ray.
static int psf_launch(int64_t n, const double* rec, int n_bands, const int64_t* starts, double radius, int n_px, double size, int n_planes,
                      const double* dz, const PsfShape& s, double* workspace, double* field, double* sums, bool kappa,
                      hipStream_t st) {
    PsfStack S;
    S.n_bands = n_bands;
    S.chunk_len = s.chunk_len;
    S.chunk0[0] = 0;
    for (int b = 0; b <= OT_PSF_MAX_BANDS; b++) {
        const int e = b < n_bands ? b : n_bands;  // (the entries behind the last band repeat it: no index reads past what was set)
        S.start[b] = starts[e];
        if (b > 0) S.chunk0[b] = S.chunk0[b - 1] + (b <= n_bands ? (int32_t)((starts[b] - starts[b - 1] + s.chunk_len - 1) / s.chunk_len) : 0);
    }
    for (int z = 0; z < OT_PSF_MAX_PLANES; z++) S.dz[z] = z < n_planes ? dz[z] : 0.0;
    const int64_t chunks = S.chunk0[n_bands];
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(psf_sum_kernel, dim3((unsigned)s.tiles, (unsigned)chunks, (unsigned)n_planes), dim3(OT_PSF_THREADS), 0, st, n, rec,
                       std::fabs(radius), radius > 0.0 ? 1.0 : -1.0, n_px, size, S, workspace);
    hipLaunchKernelGGL(psf_final_kernel, dim3(grid_for(s.stride).x, (unsigned)n_bands, (unsigned)n_planes), dim3(OT_PSF_THREADS), 0, st,
                       workspace, chunks, s.P, S, field, sums);
    if (kappa) hipLaunchKernelGGL(psf_band_kappa_kernel, dim3((unsigned)n_bands), dim3(OT_PSF_THREADS), 0, st, n, rec, S, n_planes, sums);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_psf_sum(int64_t n, const double* rec, double radius, int32_t n_px, double size, double dz, double* workspace,
                          double* field, double* centre, void* stream) {
    if (n < 0 || !rec || !workspace || !field || !centre) return fail(OT_ERR_INVALID, "ot_psf_sum: null argument");
    if (n_px < 1) return fail(OT_ERR_INVALID, "ot_psf_sum: n_px below 1");
    if (n_px > OT_PSF_MAX_PX) return fail(OT_ERR_UNSUPPORTED, "ot_psf_sum: n_px above 1024");
    if (!std::isfinite(size) || !(size > 0.0)) return fail(OT_ERR_INVALID, "ot_psf_sum: size not finite or not above zero");
    if (!std::isfinite(dz)) return fail(OT_ERR_INVALID, "ot_psf_sum: dz not finite");
    if (!std::isfinite(radius) || radius == 0.0) return fail(OT_ERR_INVALID, "ot_psf_sum: radius not finite, or zero");
    if (n == 0) return OT_OK;
    const int64_t starts[2] = {0, n};
    const PsfShape s = psf_shape(n, n_px);
    return psf_launch(n, rec, 1, starts, radius, n_px, size, 1, &dz, s, workspace, field, centre, false, (hipStream_t)stream);
}

// ---- the stack: bands of the rays x image planes (Raytracer.huygens_stack) -----------------------------------------------------------
static_assert(OT_PSF_MAX_BANDS == OT_PSF_MAX_BANDS_ && OT_PSF_MAX_PLANES == OT_PSF_MAX_PLANES_, "limits of the header and the kernels");

// chunks of the workspace: a bound that needs no starts.  Band b has ceil(n_b / chunk_len) chunks, all bands together less than
// n / chunk_len + n_bands, so at most ceil(n / chunk_len) + n_bands - 1 <= chunks + n_bands - 1.
static int64_t psf_stack_chunks(const PsfShape& s, int n_bands) { return s.chunks + n_bands - 1; }

extern "C" int64_t ot_psf_stack_workspace(int64_t n, int32_t n_bands, int32_t n_px, int32_t n_planes) {
    if (n < 0 || n_px < 1 || n_px > OT_PSF_MAX_PX || n_bands < 1 || n_bands > OT_PSF_MAX_BANDS || n_planes < 1 || n_planes > OT_PSF_MAX_PLANES)
        return 0;
    const PsfShape s = psf_stack_shape(n, n_px, n_planes);
    return (int64_t)n_planes * psf_stack_chunks(s, n_bands) * s.stride;
}

static int bad_stack_counts(const char* name, int32_t n_bands, int32_t n_px, int32_t n_planes) {
    const std::string at = std::string(name) + ": ";
    if (n_px < 1) return fail(OT_ERR_INVALID, at + "n_px below 1");
    if (n_px > OT_PSF_MAX_PX) return fail(OT_ERR_UNSUPPORTED, at + "n_px above 1024");
    if (n_bands < 1) return fail(OT_ERR_INVALID, at + "n_bands below 1");
    if (n_bands > OT_PSF_MAX_BANDS) return fail(OT_ERR_UNSUPPORTED, at + "n_bands above 32");
    if (n_planes < 1) return fail(OT_ERR_INVALID, at + "n_planes below 1");
    if (n_planes > OT_PSF_MAX_PLANES) return fail(OT_ERR_UNSUPPORTED, at + "n_planes above 64");
    return OT_OK;
}

extern "C" int ot_psf_stack(int64_t n, const double* rec, int32_t n_bands, const int64_t* starts, double radius, int32_t n_px, double size,
                            int32_t n_planes, const double* dz, double* workspace, double* field, double* sums, void* stream) {
    if (n < 0 || !rec || !starts || !dz || !workspace || !field || !sums) return fail(OT_ERR_INVALID, "ot_psf_stack: null argument");
    if (int rc = bad_stack_counts("ot_psf_stack", n_bands, n_px, n_planes)) return rc;
    if (starts[0] != 0 || starts[n_bands] != n) return fail(OT_ERR_INVALID, "ot_psf_stack: starts do not run from 0 to n");
    for (int b = 0; b < n_bands; b++)
        if (starts[b] > starts[b + 1]) return fail(OT_ERR_INVALID, "ot_psf_stack: starts not ascending");
    if (!std::isfinite(size) || !(size > 0.0)) return fail(OT_ERR_INVALID, "ot_psf_stack: size not finite or not above zero");
    for (int z = 0; z < n_planes; z++)
        if (!std::isfinite(dz[z])) return fail(OT_ERR_INVALID, "ot_psf_stack: dz not finite");
    if (!std::isfinite(radius) || radius == 0.0) return fail(OT_ERR_INVALID, "ot_psf_stack: radius not finite, or zero");
    const PsfShape s = psf_stack_shape(n, n_px, n_planes);
    const int64_t px = (int64_t)n_px * n_px;
    if ((int64_t)n_planes * psf_stack_chunks(s, n_bands) * s.stride + (int64_t)n_planes * n_bands * 2 * px > OT_PSF_STACK_CAP)
        return fail(OT_ERR_UNSUPPORTED, "ot_psf_stack: workspace and field above 2^28 doubles: fewer planes, bands or image points per call");
    if (n == 0) return OT_OK;
    return psf_launch(n, rec, n_bands, starts, radius, n_px, size, n_planes, dz, s, workspace, field, sums, true, (hipStream_t)stream);
}

extern "C" int ot_psf_combine(int32_t n_bands, int32_t n_planes, int32_t n_px, const double* field, const double* sums, double* intensity,
                              double* band_strehl, double* strehl, double* g, double* noise_floor, void* stream) {
    if (!field || !sums || !intensity || !band_strehl || !strehl || !g || !noise_floor)
        return fail(OT_ERR_INVALID, "ot_psf_combine: null argument");
    if (int rc = bad_stack_counts("ot_psf_combine", n_bands, n_px, n_planes)) return rc;
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(psf_combine_kernel, dim3(grid_for((int64_t)n_px * n_px + 1).x, (unsigned)n_planes), dim3(OT_PSF_THREADS), 0,
                       (hipStream_t)stream, (int)n_bands, (int)n_px, field, sums, intensity, band_strehl, strehl, g, noise_floor);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
