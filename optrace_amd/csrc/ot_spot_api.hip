// C-ABI, spot analysis: moments, radial histogram and geometric OTF of a hit list (Raytracer.spot_analysis).
#include "ot_host.hpp"
#include "ot_spot.hpp"

extern "C" int ot_spot_moments(int64_t n, const uint32_t* fill, const double* x, const double* y, const float* w, double* workspace,
                               double* moments, void* stream) {
    if (n < 0 || !x || !y || !w || !workspace || !moments) return fail(OT_ERR_INVALID, "ot_spot_moments: null argument");
    if (n == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned blocks = reduce_blocks(n, OT_SPOT_BLOCKS);
    hipLaunchKernelGGL(spot_first_kernel, dim3(blocks), dim3(OT_RED_THREADS), 0, st, n, x, y, w, fill, workspace);
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(OT_RED_THREADS), 0, st, workspace, (int)blocks, 4, 0u, 0u, moments, 0, 0);
    hipLaunchKernelGGL(spot_central_kernel, dim3(blocks), dim3(OT_RED_THREADS), 0, st, n, x, y, w, fill, moments, workspace);
    hipLaunchKernelGGL(reduce_final_kernel, dim3(1), dim3(OT_RED_THREADS), 0, st, workspace, (int)blocks, 4, 1u << 3, 0u, moments + 4, 0, 0);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_spot_radial(int64_t n, const uint32_t* fill, const double* x, const double* y, const float* w, const double* moments,
                              int32_t n_radii, double* hist, void* stream) {
    if (n < 0 || !x || !y || !w || !moments || !hist) return fail(OT_ERR_INVALID, "ot_spot_radial: null argument");
    if (n_radii < 1) return fail(OT_ERR_INVALID, "ot_spot_radial: n_radii below 1");
    if (n_radii > OT_SPOT_MAX_RADII) return fail(OT_ERR_UNSUPPORTED, "ot_spot_radial: more than 65536 radial bins");
    if (n == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    const HistShape hs = hist_shape(n, (size_t)n_radii * sizeof(double));
    hipLaunchKernelGGL(spot_radial_kernel, hs.grid, hs.block, hs.lds, (hipStream_t)stream, n, x, y, w, fill, moments, n_radii,
                       hs.lds ? n_radii : 0, hist);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_spot_otf(int64_t n, const uint32_t* fill, const double* x, const double* y, const float* w, const double* moments,
                           const double* freq, int32_t K, double* workspace, double* otf, void* stream) {
    if (n < 0 || !x || !y || !w || !moments || !freq || !workspace || !otf) return fail(OT_ERR_INVALID, "ot_spot_otf: null argument");
    if (K < 1) return fail(OT_ERR_INVALID, "ot_spot_otf: no frequencies");
    if (K > OT_SPOT_MAX_FREQ) return fail(OT_ERR_UNSUPPORTED, "ot_spot_otf: more than 4096 frequencies");
    if (n == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    // about OT_SPOT_BLOCKS workgroups in all, at least 64 walkers per chunk: OT_SPOT_WS(K) holds their partials
    const int chunks = (K + OT_SPOT_CHUNK - 1) / OT_SPOT_CHUNK;
    const int per_chunk = OT_SPOT_BLOCKS / chunks;
    const unsigned bx = reduce_blocks(n, per_chunk < 64 ? 64 : per_chunk);
    hipLaunchKernelGGL(spot_otf_kernel, dim3(bx, (unsigned)chunks), dim3(OT_RED_THREADS), 0, st, n, x, y, w, fill, moments, freq, K, workspace);
    hipLaunchKernelGGL(spot_otf_final_kernel, grid_for(4 * (int64_t)K), dim3(OT_RED_THREADS), 0, st, workspace, (int)bx, K, otf);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
