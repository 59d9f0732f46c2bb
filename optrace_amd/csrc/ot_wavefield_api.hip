// C-ABI, wavefront across the field: per field point and band of wavelengths the sums for the reference sphere, the optical paths
// to the sphere of every ray's cell, their moments and the normal equations of a Zernike fit (Raytracer.wavefront_field).
#include "ot_host.hpp"
#include "ot_wavefield.hpp"

// bands a lane owns at the most: enough for OT_CHROM_MAX_BANDS
enum { WVF_NCF = (OT_CHROM_MAX_BANDS + FdRoles<WFF_M>::J - 1) / FdRoles<WFF_M>::J, WVF_NC1 = (OT_CHROM_MAX_BANDS + FdRoles<WVF_M1>::J - 1) / FdRoles<WVF_M1>::J };
static_assert(FdRoles<WVF_M2>::J >= OT_CHROM_MAX_BANDS, "the second pass of the moments: one band per lane");

static bool wvf_shape_ok(int32_t n_fields, int32_t n_bands) {
    return n_fields >= 1 && n_fields <= OT_FIELD_MAX_FIELDS && n_bands >= 1 && n_bands <= OT_CHROM_MAX_BANDS;
}
static std::string wvf_shape_text() {
    return "n_fields outside 1 .. " + std::to_string(OT_FIELD_MAX_FIELDS) + " or n_bands outside 1 .. " + std::to_string(OT_CHROM_MAX_BANDS);
}

// Workgroups of a field over all its pieces, `cap` at the most per piece: from the field's count alone, so what a field's sums
// are does not depend on the other fields of the call.
static int64_t wvf_field_blocks(int64_t count, int64_t cap) {
    int64_t total = 0;
    for_ray_chunks(0, count, [&](int64_t, uint32_t n) { total += reduce_blocks(n, cap); });
    return total;
}
// The longest list of partials of a field: every field's list is padded to it
static int64_t wvf_list_len(const int64_t* fields, int32_t n_fields, int64_t cap) {
    int64_t len = 1;
    for (int32_t f = 0; f < n_fields; f++) len = std::max(len, wvf_field_blocks(fields[2 * f + 1], cap));
    return len;
}
// the table size of the fit and the walkers of a piece it takes at the most (two sizes, as in ot_wavefront_zernike)
static int wvf_table(int J) { return J <= 15 ? 15 : OT_WF_MAX_J; }
static int64_t wvf_zernike_cell(int JT) { return (int64_t)((JT + 1) / 2) * (JT + 3); }

// The pieces of the fields, from the counts alone: `cap` workgroups at the most per piece (0: one per 256 rays); a field without
// rays has one piece without workgroups, which pads its list.
static std::vector<FdPiece> wvf_pieces(const int64_t* fields, unsigned F, int64_t cap) {
    std::vector<FdPiece> pieces;
    for (unsigned f = 0; f < F; f++) {
        uint32_t block0 = 0;
        for_ray_chunks(fields[2 * f], fields[2 * f + 1], [&](int64_t base, uint32_t n) {
            const uint32_t blocks = cap ? reduce_blocks(n, cap) : (n + OT_RED_THREADS - 1) / OT_RED_THREADS;
            pieces.push_back({base, n, blocks, block0, f});
            block0 += blocks;
        });
        if (!block0) pieces.push_back({fields[2 * f], 0u, 0u, 0u, f});
        pieces.back().field |= 0x80000000u;
    }
    return pieces;
}
template <class Launch>
static void wvf_for_batches(const std::vector<FdPiece>& pieces, Launch&& launch) {
    for (size_t at = 0; at < pieces.size(); at += FD_PIECES) {
        const unsigned n = (unsigned)std::min<size_t>(FD_PIECES, pieces.size() - at);
        FdBatch batch = {};
        std::copy(pieces.begin() + at, pieces.begin() + at + n, batch.piece);
        launch(batch, n);
    }
}

// fields[n_fields][2]: every range within [key_first, key_first + ...) and within N rays (N < 0: no storage to hold them to).
// -> what is wrong, or nullptr; *total: the rays of all fields
static const char* wvf_bad_fields(const int64_t* fields, int32_t n_fields, int64_t key_first, int64_t N, int64_t* total) {
    *total = 0;
    for (int32_t f = 0; f < n_fields; f++) {
        const int64_t first = fields[2 * f], count = fields[2 * f + 1];
        if (first < 0 || count < 0 || (N >= 0 && first + count > N)) return "ray range outside the storage";
        if (count > 0 && first < key_first) return "a field starts before key_first";
        *total += count;
    }
    return nullptr;
}

extern "C" int64_t ot_wavefield_workspace(const int64_t* fields, int32_t n_fields, int32_t n_bands, int32_t J) {
    if (!fields || !wvf_shape_ok(n_fields, n_bands) || J < 1 || J > OT_WF_MAX_J) return 0;
    for (int32_t f = 0; f < n_fields; f++)
        if (fields[2 * f + 1] < 0) return 0;
    // the partials of the sums, [F][list][K][17] for the largest | the sums of the two passes of the moments; or the partials of the fit
    const int64_t sums = (int64_t)n_fields * n_bands * (wvf_list_len(fields, n_fields, OT_FIELD_BLOCKS) * WFF_M + WVF_M1 + WVF_M2);
    const int64_t fit = (int64_t)n_fields * n_bands * wvf_list_len(fields, n_fields, OT_WFF_FIT_BLOCKS) * wvf_zernike_cell(wvf_table(J));
    return std::max(sums, fit);
}

extern "C" int ot_wavefield_focus(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key,
                                  int64_t key_first, int32_t n_bands, const double* origin, double* workspace, double* sums,
                                  void* stream) {
    if (!fields || !key || !origin || !workspace || !sums) return fail(OT_ERR_INVALID, "ot_wavefield_focus: null argument");
    if (!wvf_shape_ok(n_fields, n_bands)) return fail(OT_ERR_UNSUPPORTED, "ot_wavefield_focus: " + wvf_shape_text());
    if (const char* bad = bad_section_sphere(rays, 0, 0, section, false, nullptr, 0.0))
        return fail(OT_ERR_INVALID, std::string("ot_wavefield_focus: ") + bad);
    int64_t rays_total;
    if (const char* bad = wvf_bad_fields(fields, n_fields, key_first, rays->N, &rays_total))
        return fail(OT_ERR_INVALID, std::string("ot_wavefield_focus: ") + bad);
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
        return fail(OT_ERR_INVALID, "ot_wavefield_focus: origin not finite");
    if (rays_total == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned K = (unsigned)n_bands, F = (unsigned)n_fields, list_len = (unsigned)wvf_list_len(fields, n_fields, OT_FIELD_BLOCKS);
    wvf_for_batches(wvf_pieces(fields, F, OT_FIELD_BLOCKS), [&](const FdBatch& batch, unsigned n) {
        // (the bands a lane owns: one where that covers K, else as many as cover OT_CHROM_MAX_BANDS)
        hipLaunchKernelGGL(K <= FdRoles<WFF_M>::J ? wvf_focus_kernel<1> : wvf_focus_kernel<WVF_NCF>, dim3(list_len, n), dim3(OT_RED_THREADS),
                           0, st, *rays, key, key_first, (int)section, batch, K, list_len, origin[0], origin[1], origin[2], workspace);
    });
    hipLaunchKernelGGL(wvf_final_kernel, dim3(F), dim3(OT_RED_THREADS), 0, st, (const double*)workspace, (int)list_len, (int)(K * WFF_M),
                       (int)WFF_M, 0u, 0u, sums);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_wavefield_paths(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key,
                                  int64_t key_first, int32_t n_bands, const double* spheres, double* u, double* v, double* opl,
                                  float* w_out, int64_t* counts, void* stream) {
    if (!fields || !key || !spheres || !u || !v || !opl || !w_out || !counts) return fail(OT_ERR_INVALID, "ot_wavefield_paths: null argument");
    if (!wvf_shape_ok(n_fields, n_bands)) return fail(OT_ERR_UNSUPPORTED, "ot_wavefield_paths: " + wvf_shape_text());
    if (const char* bad = bad_section_sphere(rays, 0, 0, section, true, nullptr, 0.0))
        return fail(OT_ERR_INVALID, std::string("ot_wavefield_paths: ") + bad);
    int64_t rays_total;
    if (const char* bad = wvf_bad_fields(fields, n_fields, key_first, rays->N, &rays_total))
        return fail(OT_ERR_INVALID, std::string("ot_wavefield_paths: ") + bad);
    if (rays_total == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned K = (unsigned)n_bands, F = (unsigned)n_fields;
    HIP_TRY(hipMemsetAsync(counts, 0, sizeof(int64_t) * 2 * F * K, st));
    wvf_for_batches(wvf_pieces(fields, F, 0), [&](const FdBatch& batch, unsigned n) {
        uint32_t blocks = 1;
        for (unsigned i = 0; i < n; i++) blocks = std::max(blocks, batch.piece[i].blocks);
        hipLaunchKernelGGL(wvf_paths_kernel, dim3(blocks, n), dim3(OT_RED_THREADS), 0, st, *rays, key, key_first, (int)section, batch, K,
                           spheres, u, v, opl, w_out, (unsigned long long*)counts);
    });
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_wavefield_moments(const int64_t* fields, int32_t n_fields, const double* u, const double* v, const double* opl,
                                    const float* w, const float* wl, const uint8_t* key, int64_t key_first, int32_t n_bands,
                                    double* workspace, double* moments, double* pupil, void* stream) {
    if (!fields || !u || !v || !opl || !w || !wl || !key || !workspace || !moments || !pupil)
        return fail(OT_ERR_INVALID, "ot_wavefield_moments: null argument");
    if (!wvf_shape_ok(n_fields, n_bands)) return fail(OT_ERR_UNSUPPORTED, "ot_wavefield_moments: " + wvf_shape_text());
    int64_t total;
    if (const char* bad = wvf_bad_fields(fields, n_fields, key_first, -1, &total))
        return fail(OT_ERR_INVALID, std::string("ot_wavefield_moments: ") + bad);
    if (total == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned K = (unsigned)n_bands, F = (unsigned)n_fields, list_len = (unsigned)wvf_list_len(fields, n_fields, OT_FIELD_BLOCKS);
    const std::vector<FdPiece> pieces = wvf_pieces(fields, F, OT_FIELD_BLOCKS);
    double *part = workspace, *first = workspace + (int64_t)F * K * list_len * WFF_M, *central = first + (int64_t)F * K * WVF_M1;
    wvf_for_batches(pieces, [&](const FdBatch& batch, unsigned n) {
        hipLaunchKernelGGL(K <= FdRoles<WVF_M1>::J ? wvf_first_kernel<1> : wvf_first_kernel<WVF_NC1>, dim3(list_len, n), dim3(OT_RED_THREADS),
                           0, st, u, v, opl, w, wl, key, key_first, batch, K, list_len, part);
    });
    hipLaunchKernelGGL(wvf_final_kernel, dim3(F), dim3(OT_RED_THREADS), 0, st, (const double*)part, (int)list_len, (int)(K * WVF_M1),
                       (int)WVF_M1, (unsigned)WVF_MAX1, 1u << WVF_OPL_MIN, first);
    hipLaunchKernelGGL(wvf_centre_kernel, grid_for(F), dim3(256), 0, st, (int)F, (int)K, (const double*)first, pupil);
    wvf_for_batches(pieces, [&](const FdBatch& batch, unsigned n) {
        hipLaunchKernelGGL(wvf_central_kernel, dim3(list_len, n), dim3(OT_RED_THREADS), 0, st, u, v, opl, w, key, key_first, batch, K,
                           list_len, (const double*)first, (const double*)pupil, part);
    });
    hipLaunchKernelGGL(wvf_final_kernel, dim3(F), dim3(OT_RED_THREADS), 0, st, (const double*)part, (int)list_len, (int)(K * WVF_M2),
                       (int)WVF_M2, (unsigned)WVF_MAX2, 0u, central);
    hipLaunchKernelGGL(wvf_finish_kernel, grid_for(F), dim3(256), 0, st, (int)F, (int)K, (const double*)first, (const double*)central,
                       moments, pupil);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

template <int JT>
static void wvf_zernike_launch(const std::vector<FdPiece>& pieces, const double* u, const double* v, const double* opl, const float* w,
                               const uint8_t* key, int64_t key_first, unsigned F, unsigned K, unsigned list_len, const double* moments,
                               const double* pupil, double pupil_radius, int J, double* workspace, double* out, hipStream_t st) {
    constexpr int chunks = (JT + 1) / 2;
    wvf_for_batches(pieces, [&](const FdBatch& batch, unsigned n) {
        hipLaunchKernelGGL(wvf_zernike_kernel<JT>, dim3(list_len, (unsigned)chunks, n * K), dim3(OT_RED_THREADS), 0, st, u, v, opl, w, key,
                           key_first, batch, K, list_len, moments, pupil, pupil_radius, workspace);
    });
    hipLaunchKernelGGL(wvf_zernike_final_kernel, dim3(grid_for(chunks * (JT + 3)).x, F * K), dim3(OT_RED_THREADS), 0, st,
                       (const double*)workspace, (int)list_len, JT, J, out);
}

extern "C" int ot_wavefield_zernike(const int64_t* fields, int32_t n_fields, const double* u, const double* v, const double* opl,
                                    const float* w, const uint8_t* key, int64_t key_first, int32_t n_bands, const double* moments,
                                    const double* pupil, double pupil_radius, int32_t J, double* workspace, double* out, void* stream) {
    if (!fields || !u || !v || !opl || !w || !key || !moments || !pupil || !workspace || !out)
        return fail(OT_ERR_INVALID, "ot_wavefield_zernike: null argument");
    if (J < 1) return fail(OT_ERR_INVALID, "ot_wavefield_zernike: no polynomials");
    if (!wvf_shape_ok(n_fields, n_bands) || J > OT_WF_MAX_J)
        return fail(OT_ERR_UNSUPPORTED, "ot_wavefield_zernike: " + wvf_shape_text() + " or more than 36 polynomials");
    int64_t total;
    if (const char* bad = wvf_bad_fields(fields, n_fields, key_first, -1, &total))
        return fail(OT_ERR_INVALID, std::string("ot_wavefield_zernike: ") + bad);
    if (!std::isnan(pupil_radius) && !(std::isfinite(pupil_radius) && pupil_radius > 0.0))
        return fail(OT_ERR_INVALID, "ot_wavefield_zernike: pupil radius neither NaN nor above zero");
    if (total == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned K = (unsigned)n_bands, F = (unsigned)n_fields, list_len = (unsigned)wvf_list_len(fields, n_fields, OT_WFF_FIT_BLOCKS);
    const std::vector<FdPiece> pieces = wvf_pieces(fields, F, OT_WFF_FIT_BLOCKS);
    if (J <= 15)
        wvf_zernike_launch<15>(pieces, u, v, opl, w, key, key_first, F, K, list_len, moments, pupil, pupil_radius, J, workspace, out, st);
    else
        wvf_zernike_launch<OT_WF_MAX_J>(pieces, u, v, opl, w, key, key_first, F, K, list_len, moments, pupil, pupil_radius, J, workspace, out, st);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
