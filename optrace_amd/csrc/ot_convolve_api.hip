// C-ABI, field-dependent convolution: an image spread by a grid of point spread functions, blended bilinearly over the field
// (ot.convolve_field).
#include "ot_host.hpp"
#include "ot_convolve.hpp"

extern "C" int ot_convolve_field(const double* img, int32_t n_ch, int32_t ny, int32_t nx, int32_t y0, int32_t x0, int32_t ny_in,
                                 int32_t nx_in, const double* psf, int32_t gy, int32_t gx, int32_t py, int32_t px, double* out,
                                 void* stream) {
    if (!img || !psf || !out) return fail(OT_ERR_INVALID, "ot_convolve_field: null argument");
    if (n_ch < 1 || n_ch > 3) return fail(OT_ERR_INVALID, "ot_convolve_field: n_ch outside 1..3");
    if (ny < 1 || nx < 1 || ny_in < 1 || nx_in < 1 || gy < 1 || gx < 1 || py < 1 || px < 1)
        return fail(OT_ERR_INVALID, "ot_convolve_field: size below 1");
    if (y0 < 0 || x0 < 0 || (int64_t)y0 + ny_in > ny || (int64_t)x0 + nx_in > nx)
        return fail(OT_ERR_INVALID, "ot_convolve_field: interior outside the plane");
    if (py > OT_CONVF_MAX_PSF || px > OT_CONVF_MAX_PSF) return fail(OT_ERR_UNSUPPORTED, "ot_convolve_field: py or px above 512");
    if (gy > OT_CONVF_MAX_GRID || gx > OT_CONVF_MAX_GRID) return fail(OT_ERR_UNSUPPORTED, "ot_convolve_field: gy or gx above 64");
    const int64_t oh = (int64_t)ny + py - 1, ow = (int64_t)nx + px - 1;
    if (oh * ow > INT32_MAX) return fail(OT_ERR_UNSUPPORTED, "ot_convolve_field: output plane above 2^31 - 1 elements");
    const int64_t tiles_x = (ow + CF_TX - 1) / CF_TX, tiles_y = (oh + CF_TY - 1) / CF_TY;
    if (tiles_x * tiles_y * n_ch > INT32_MAX) return fail(OT_ERR_UNSUPPORTED, "ot_convolve_field: more than 2^31 - 1 output tiles");
    if (int rc = require_device()) return rc;
    ConvfArgs A;
    A.img = img, A.psf = psf, A.out = out;
    A.n_ch = n_ch, A.ny = ny, A.nx = nx, A.y0 = y0, A.x0 = x0, A.ny_in = ny_in, A.nx_in = nx_in;
    A.gy = gy, A.gx = gx, A.py = py, A.px = px;
    A.oh = (int32_t)oh, A.ow = (int32_t)ow, A.tiles_x = (int32_t)tiles_x, A.tiles_y = (int32_t)tiles_y;
    hipLaunchKernelGGL(convolve_field_kernel, dim3((unsigned)(tiles_x * tiles_y * n_ch)), dim3(CF_THREADS), 0, (hipStream_t)stream, A);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
