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

extern "C" int ot_psf_sum(int64_t n, const double* rec, double radius, int32_t n_px, double size, double dz, double* workspace,
                          double* field, double* centre, void* stream) {
    if (n < 0 || !rec || !workspace || !field || !centre) return fail(OT_ERR_INVALID, "ot_psf_sum: null argument");
    if (n_px < 1) return fail(OT_ERR_INVALID, "ot_psf_sum: n_px below 1");
    if (n_px > OT_PSF_MAX_PX) return fail(OT_ERR_UNSUPPORTED, "ot_psf_sum: n_px above 1024");
    if (!std::isfinite(size) || !(size > 0.0)) return fail(OT_ERR_INVALID, "ot_psf_sum: size not finite or not above zero");
    if (!std::isfinite(dz)) return fail(OT_ERR_INVALID, "ot_psf_sum: dz not finite");
    if (!std::isfinite(radius) || radius == 0.0) return fail(OT_ERR_INVALID, "ot_psf_sum: radius not finite, or zero");
    if (n == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const PsfShape s = psf_shape(n, n_px);
    hipLaunchKernelGGL(psf_sum_kernel, dim3((unsigned)s.tiles, (unsigned)s.chunks), dim3(OT_PSF_THREADS), 0, st, n, rec, std::fabs(radius),
                       radius > 0.0 ? 1.0 : -1.0, (int)n_px, size, dz, s.chunk_len, workspace);
    hipLaunchKernelGGL(psf_final_kernel, grid_for(s.stride), dim3(OT_PSF_THREADS), 0, st, workspace, s.chunks, s.P, field, centre);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
