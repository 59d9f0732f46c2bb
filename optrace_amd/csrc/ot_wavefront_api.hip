// C-ABI, wavefront analysis: optical path to a reference sphere, its moments, pupil map and Zernike normal equations
// (Raytracer.wavefront_analysis).
#include "ot_host.hpp"
#include "ot_wavefront.hpp"

extern "C" int ot_wavefront_focus(const ot_rays* rays, int64_t first, int64_t count, int32_t section, const double* origin,
                                  double* workspace, double* sums, void* stream) {
    if (!origin || !workspace || !sums) return fail(OT_ERR_INVALID, "ot_wavefront_focus: null argument");
    if (const char* bad = bad_section_sphere(rays, first, count, section, false, nullptr, 0.0))
        return fail(OT_ERR_INVALID, std::string("ot_wavefront_focus: ") + bad);
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
        return fail(OT_ERR_INVALID, "ot_wavefront_focus: origin not finite");
    if (count == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = reduce_blocks(count, OT_WF_BLOCKS);
    hipLaunchKernelGGL(wf_focus_kernel, dim3(blocks), dim3(OT_RED_THREADS), 0, st, *rays, first, count, (int)section, origin[0], origin[1],
                       origin[2], workspace);
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(OT_RED_THREADS), 0, st, workspace, (int)blocks, (int)WFF_M, 0u, 0u, sums, 0, 0);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_wavefront_paths(const ot_rays* rays, int64_t first, int64_t count, int32_t section, const double* focus, double radius,
                                  double* u, double* v, double* opl, float* w_out, int64_t* missed, void* stream) {
    if (!focus || !u || !v || !opl || !w_out || !missed) return fail(OT_ERR_INVALID, "ot_wavefront_paths: null argument");
    if (const char* bad = bad_section_sphere(rays, first, count, section, true, focus, radius))
        return fail(OT_ERR_INVALID, std::string("ot_wavefront_paths: ") + bad);
    if (count == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemsetAsync(missed, 0, sizeof(int64_t), st));
    hipLaunchKernelGGL(wf_paths_kernel, grid_for(count), dim3(OT_RED_THREADS), 0, st, *rays, first, count, (int)section, focus[0], focus[1],
                       focus[2], radius, u, v, opl, w_out, (unsigned long long*)missed);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_wavefront_moments(int64_t n, const double* u, const double* v, const double* opl, const float* w, const float* wl,
                                    double* workspace, double* moments, void* stream) {
    if (n < 0 || !u || !v || !opl || !w || !workspace || !moments) return fail(OT_ERR_INVALID, "ot_wavefront_moments: null argument");
    if (n == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = reduce_blocks(n, OT_WF_BLOCKS);
    const unsigned maxima = (1u << WF_OPL_MIN) | (1u << WF_OPL_MAX);
    hipLaunchKernelGGL(wf_first_kernel, dim3(blocks), dim3(OT_RED_THREADS), 0, st, n, u, v, opl, w, wl, workspace);
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(OT_RED_THREADS), 0, st, workspace, (int)blocks, 8, maxima, 1u << WF_OPL_MIN, moments, 0, 0);
    hipLaunchKernelGGL(wf_central_kernel, dim3(blocks), dim3(OT_RED_THREADS), 0, st, n, u, v, opl, w, moments, workspace);
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(OT_RED_THREADS), 0, st, workspace, (int)blocks, 2, 2u, 0u, moments + WF_WOPD2, 0, 0);
    hipLaunchKernelGGL(wf_pupil_radius_kernel, dim3(1), dim3(1), 0, st, moments);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

// pupil_radius: NaN (take the moments') or finite and above zero
static bool wf_bad_pupil(double pupil_radius) { return !std::isnan(pupil_radius) && !(std::isfinite(pupil_radius) && pupil_radius > 0.0); }

extern "C" int ot_wavefront_map(int64_t n, const double* u, const double* v, const double* opl, const float* w, const double* moments,
                                double pupil_radius, int32_t n_grid, double* map, void* stream) {
    if (n < 0 || !u || !v || !opl || !w || !moments || !map) return fail(OT_ERR_INVALID, "ot_wavefront_map: null argument");
    if (n_grid < 1) return fail(OT_ERR_INVALID, "ot_wavefront_map: n_grid below 1");
    if (n_grid > OT_WF_MAX_GRID) return fail(OT_ERR_UNSUPPORTED, "ot_wavefront_map: n_grid above 1024");
    if (wf_bad_pupil(pupil_radius)) return fail(OT_ERR_INVALID, "ot_wavefront_map: pupil radius neither NaN nor above zero");
    if (n == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    const int cells2 = 2 * n_grid * n_grid;
    const HistShape hs = hist_shape(n, (size_t)cells2 * sizeof(double));
    hipLaunchKernelGGL(wf_map_kernel, hs.grid, hs.block, hs.lds, (hipStream_t)stream, n, u, v, opl, w, moments, pupil_radius, (int)n_grid,
                       hs.lds ? cells2 : 0, map);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

template <int JT>
static void wf_zernike_launch(int64_t n, const double* u, const double* v, const double* opl, const float* w, const double* moments,
                              double pupil_radius, int J, double* workspace, double* out, hipStream_t st) {
    // about OT_WF_BLOCKS workgroups in all, at least 64 walkers per chunk: OT_WF_WS holds their partials
    constexpr int chunks = (JT + 1) / 2, per_chunk = OT_WF_BLOCKS / chunks;
    static_assert((int64_t)(per_chunk < 64 ? 64 : per_chunk) * chunks * (JT + 3) <= OT_WF_WS, "workspace");
    const unsigned bx = reduce_blocks(n, per_chunk < 64 ? 64 : per_chunk);
    hipLaunchKernelGGL(wf_zernike_kernel<JT>, dim3(bx, (unsigned)chunks), dim3(OT_RED_THREADS), 0, st, n, u, v, opl, w, moments, pupil_radius,
                       workspace);
    hipLaunchKernelGGL(wf_zernike_final_kernel, grid_for(chunks * (JT + 3)), dim3(OT_RED_THREADS), 0, st, workspace, (int)bx, JT, J, out);
}

extern "C" int ot_wavefront_zernike(int64_t n, const double* u, const double* v, const double* opl, const float* w, const double* moments,
                                    double pupil_radius, int32_t J, double* workspace, double* out, void* stream) {
    if (n < 0 || !u || !v || !opl || !w || !moments || !workspace || !out) return fail(OT_ERR_INVALID, "ot_wavefront_zernike: null argument");
    if (J < 1) return fail(OT_ERR_INVALID, "ot_wavefront_zernike: no polynomials");
    if (J > OT_WF_MAX_J) return fail(OT_ERR_UNSUPPORTED, "ot_wavefront_zernike: more than 36 polynomials");
    if (wf_bad_pupil(pupil_radius)) return fail(OT_ERR_INVALID, "ot_wavefront_zernike: pupil radius neither NaN nor above zero");
    if (n == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    // (two table sizes: the fourth radial order, which is the default of the Python side, and everything)
    if (J <= 15)
        wf_zernike_launch<15>(n, u, v, opl, w, moments, pupil_radius, J, workspace, out, st);
    else
        wf_zernike_launch<OT_WF_MAX_J>(n, u, v, opl, w, moments, pupil_radius, J, workspace, out, st);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
