// C-ABI, sampler stage: the stratified samplers, the start positions of the source shapes, inverse transform sampling and the
// wavelengths of sRGB colours as entry points of their own (kernels: ot_sample.hpp).  Arguments are checked before a device is
// looked for; the tables come from the builders the source stage uses (ot_host.hpp).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ot_host.hpp"
#include "ot_sample.hpp"

extern "C" int ot_sample_stratified(int32_t kind, int32_t flag, const double* bounds, const ot_source_range* ranges,
                                    int32_t n_ranges, uint64_t seed, int64_t n, double* out0, double* out1, void* stream) {
    if (kind < OT_SAMPLE_INTERVAL || kind > OT_SAMPLE_RING) return fail(OT_ERR_INVALID, "ot_sample_stratified: unknown kind");
    if (!bounds || !out0 || (kind != OT_SAMPLE_INTERVAL && !out1)) return fail(OT_ERR_INVALID, "ot_sample_stratified: null pointer");
    if (n < 0) return fail(OT_ERR_INVALID, "ot_sample_stratified: negative count");
    StratArgs A = {kind, flag, bounds[0], bounds[1], 0.0, 0.0};
    if (kind == OT_SAMPLE_RING) {
        if (!(bounds[0] >= 0.0) || !(bounds[1] > bounds[0])) return fail(OT_ERR_INVALID, "ot_sample_stratified: ring needs 0 <= ri < r");
    } else if (!(bounds[1] >= bounds[0])) {
        return fail(OT_ERR_INVALID, "ot_sample_stratified: upper bound below the lower one");
    }
    if (kind == OT_SAMPLE_RECTANGLE) {
        A.c = bounds[2];
        A.d = bounds[3];
        if (!(A.d >= A.c)) return fail(OT_ERR_INVALID, "ot_sample_stratified: upper bound below the lower one");
    }
    if (n == 0) return OT_OK;
    RangeArgs rg;
    if (int rc = sampler_ranges("ot_sample_stratified", ranges, n_ranges, n, &rg)) return rc;
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(sample_stratified_kernel, grid_for(n), dim3(256), 0, (hipStream_t)stream, A, rg, seed, n, out0, out1);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_sample_positions(const ot_source* shape, const ot_source_range* ranges, int32_t n_ranges, uint64_t seed,
                                   int64_t n, double* p, void* stream) {
    if (!shape || !p) return fail(OT_ERR_INVALID, "ot_sample_positions: null pointer");
    if (n < 0) return fail(OT_ERR_INVALID, "ot_sample_positions: negative count");
    if (shape->shape == OT_SRC_IMAGE_RGB || shape->shape == OT_SRC_IMAGE_GRAY)
        return fail(OT_ERR_UNSUPPORTED, "ot_sample_positions: image sources have no positions of their own");
    if (shape->shape < OT_SRC_POINT || shape->shape > OT_SRC_RECT) return fail(OT_ERR_INVALID, "ot_sample_positions: unknown shape");
    if (shape->shape == OT_SRC_RING && !(shape->r > shape->ri)) return fail(OT_ERR_INVALID, "ot_sample_positions: ring needs ri < r");
    if (n == 0) return OT_OK;
    RangeArgs rg;
    if (int rc = sampler_ranges("ot_sample_positions", ranges, n_ranges, n, &rg)) return rc;
    if (int rc = require_device()) return rc;
    ShapeArgs S;
    std::memset(&S, 0, sizeof(S));
    S.shape = shape->shape;
    std::memcpy(S.pos, shape->pos, sizeof(S.pos));
    S.r = shape->r; S.ri = shape->ri; S.dim[0] = shape->dim[0]; S.dim[1] = shape->dim[1];
    S.ca = (shape->angle != 0.0) ? std::cos(shape->angle) : 1.0;  // as SourceDev::ca, sa (ot_sources_create)
    S.sa = (shape->angle != 0.0) ? std::sin(shape->angle) : 0.0;
    hipLaunchKernelGGL(sample_positions_kernel, grid_for(n), dim3(256), 0, (hipStream_t)stream, S, rg, seed, n, p);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_sample_inverse(int32_t kind, const double* x, const double* f, int64_t m, const double* S, int64_t n,
                                 const ot_source_range* ranges, int32_t n_ranges, uint64_t seed, double* out, void* stream) {
    if (kind != OT_SAMPLE_DISCRETE && kind != OT_SAMPLE_CONTINUOUS) return fail(OT_ERR_INVALID, "ot_sample_inverse: unknown kind");
    if (!x || !f || !out) return fail(OT_ERR_INVALID, "ot_sample_inverse: null pointer");
    if (m < 1 || m > 0x7fffffffll) return fail(OT_ERR_INVALID, "ot_sample_inverse: the pdf needs between 1 and 2^31 - 1 values");
    if (n < 0) return fail(OT_ERR_INVALID, "ot_sample_inverse: negative count");
    // the tables: random.py:136-157
    std::vector<double> tab, F;
    if (kind == OT_SAMPLE_DISCRETE) {  // x[m'] | F[m']: entries with f > 0, running sum
        std::vector<double> xs;
        double acc = 0.0;
        for (int64_t j = 0; j < m; j++) {
            if (f[j] < 0) return fail(OT_ERR_INVALID, "ot_sample_inverse: negative value in the pdf");
            if (f[j] > 0) {
                acc += f[j];
                xs.push_back(x[j]);
                F.push_back(acc);
            }
        }
        tab = xs;
        tab.insert(tab.end(), F.begin(), F.end());
    } else {  // (F_j, x_j) pairs of the cumulative trapezoid
        F.resize((size_t)m);
        for (int64_t j = 0; j < m; j++) {
            if (f[j] < 0) return fail(OT_ERR_INVALID, "ot_sample_inverse: negative value in the pdf");
            F[j] = (j == 0) ? 0.0 : F[j - 1] + (f[j] + f[j - 1]) / 2;
            tab.push_back(F[j]);
            tab.push_back(x[j]);
        }
    }
    if (F.empty() || !(F.back() > 0.0)) return fail(OT_ERR_INVALID, "ot_sample_inverse: cumulated probability is zero");
    if (n == 0) return OT_OK;
    RangeArgs rg;
    if (S) {
        rg.n = 0;
        rg.ext = nullptr;
    } else if (int rc = sampler_ranges("ot_sample_inverse", ranges, n_ranges, n, &rg)) {
        return rc;
    }
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    CdfGuide G;
    std::vector<int32_t> guides;
    build_cdf_guide(F.data(), F.size(), 0.0, &G, guides);
    const size_t o_guide = align_up(sizeof(double) * tab.size());
    const size_t total = o_guide + sizeof(int32_t) * guides.size();
    const ot_scratch::Lease lease = workspace(OT_WS_SAMPLE, total, st);
    if (!lease) return fail(OT_ERR_HIP, "ot_sample_inverse: out of device memory");
    std::vector<char> host(total, 0);
    std::memcpy(host.data(), tab.data(), sizeof(double) * tab.size());
    std::memcpy(host.data() + o_guide, guides.data(), sizeof(int32_t) * guides.size());
    // in stream order behind the previous user of the block; the host copy is gone when this function returns
    HIP_TRY(hipMemcpyAsync(lease.p(), host.data(), total, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    G.g = (const int32_t*)(lease.p() + o_guide);
    hipLaunchKernelGGL(sample_inverse_kernel, grid_for(n), dim3(256), 0, st, (const double*)lease.p(), (int)F.size(), (int)kind, G,
                       F.back(), S, rg, seed, n, out);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_sample_srgb_wavelengths(const double* rgb, int64_t n, const ot_source_range* ranges, int32_t n_ranges,
                                          uint64_t seed, double* wl, void* stream) {
    if (!rgb || !wl) return fail(OT_ERR_INVALID, "ot_sample_srgb_wavelengths: null pointer");
    if (n < 0) return fail(OT_ERR_INVALID, "ot_sample_srgb_wavelengths: negative count");
    if (n == 0) return OT_OK;
    RangeArgs rg;
    if (int rc = sampler_ranges("ot_sample_srgb_wavelengths", ranges, n_ranges, n, &rg)) return rc;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const std::vector<double>& inv = srgb_primary_inverse_tables();  // (lives as long as the process: no wait for the copy)
    const ot_scratch::Lease lease = workspace(OT_WS_SAMPLE, sizeof(double) * inv.size(), st);
    if (!lease) return fail(OT_ERR_HIP, "ot_sample_srgb_wavelengths: out of device memory");
    HIP_TRY(hipMemcpyAsync(lease.p(), inv.data(), sizeof(double) * inv.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(sample_srgb_kernel, grid_for(n), dim3(256), 0, st, rgb, (const double*)lease.p(), rg, seed, n, wl);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
