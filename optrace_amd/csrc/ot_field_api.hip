// C-ABI, field analysis: per field point and band of wavelengths the moments of the ray lines of a stored trace
// (Raytracer.field_analysis).
#include "ot_field.hpp"
#include "ot_host.hpp"

// bands a lane owns at the most: enough for OT_CHROM_MAX_BANDS
enum { FD_NC1 = (OT_CHROM_MAX_BANDS + FdRoles<FD_M1>::J - 1) / FdRoles<FD_M1>::J, FD_NC2 = (OT_CHROM_MAX_BANDS + FdRoles<FD_M2>::J - 1) / FdRoles<FD_M2>::J };

static bool fd_shape_ok(int32_t n_fields, int32_t n_bands) {
    return n_fields >= 1 && n_fields <= OT_FIELD_MAX_FIELDS && n_bands >= 1 && n_bands <= OT_CHROM_MAX_BANDS;
}

// Workgroups of a field over all its pieces: a piece per chunk of for_ray_chunks, reduce_blocks of the piece's rays each.  From
// the field's count alone: what a field's sums are does not depend on the other fields of the call.
static int64_t fd_field_blocks(int64_t count) {
    int64_t total = 0;
    for_ray_chunks(0, count, [&](int64_t, uint32_t n) { total += reduce_blocks(n, OT_FIELD_BLOCKS); });
    return total;
}

// The longest list of partials of a field: every field's list is padded to it with zeros, one batched last kernel folds them all
static int64_t fd_list_len(const int64_t* fields, int32_t n_fields) {
    int64_t len = 1;
    for (int32_t f = 0; f < n_fields; f++) len = std::max(len, fd_field_blocks(fields[2 * f + 1]));
    return len;
}

extern "C" int64_t ot_field_workspace(const int64_t* fields, int32_t n_fields, int32_t n_bands) {
    if (!fields || !fd_shape_ok(n_fields, n_bands)) return 0;
    for (int32_t f = 0; f < n_fields; f++)
        if (fields[2 * f + 1] < 0) return 0;
    // the partials of a pass, [F][list][K][FD_M2] for the larger one | the sums of pass 1 | the sums of pass 2
    return ((int64_t)n_fields * fd_list_len(fields, n_fields) * FD_M2 + (int64_t)n_fields * FD_M) * n_bands;
}

extern "C" int ot_field_sums(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key,
                             int64_t key_first, int32_t n_bands, const double* origin, double* workspace, double* records,
                             void* stream) {
    if (!fields || !key || !origin || !workspace || !records || (rays && !rays->wl))
        return fail(OT_ERR_INVALID, "ot_field_sums: null argument");
    if (!fd_shape_ok(n_fields, n_bands))
        return fail(OT_ERR_UNSUPPORTED, "ot_field_sums: n_fields outside 1 .. " + std::to_string(OT_FIELD_MAX_FIELDS) +
                                            " or n_bands outside 1 .. " + std::to_string(OT_CHROM_MAX_BANDS));
    int64_t rays_total = 0;
    for (int32_t f = 0; f < n_fields; f++) {
        if (const char* bad = bad_section_sphere(rays, fields[2 * f], fields[2 * f + 1], section, false, nullptr, 0.0))
            return fail(OT_ERR_INVALID, std::string("ot_field_sums: ") + bad);
        if (fields[2 * f + 1] > 0 && fields[2 * f] < key_first) return fail(OT_ERR_INVALID, "ot_field_sums: a field starts before key_first");
        rays_total += fields[2 * f + 1];
    }
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
        return fail(OT_ERR_INVALID, "ot_field_sums: origin not finite");
    if (rays_total == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int nt = rays->nt, k = section;
    const int64_t N = rays->N;
    const unsigned K = (unsigned)n_bands, F = (unsigned)n_fields, list_len = (unsigned)fd_list_len(fields, n_fields);

    // the pieces, from the counts alone; a field without rays has one piece without workgroups, which zeroes its list
    std::vector<FdPiece> pieces;
    for (unsigned f = 0; f < F; f++) {
        uint32_t block0 = 0;
        for_ray_chunks(fields[2 * f], fields[2 * f + 1], [&](int64_t base, uint32_t n) {
            const uint32_t blocks = reduce_blocks(n, OT_FIELD_BLOCKS);
            pieces.push_back({base, n, blocks, block0, f});
            block0 += blocks;
        });
        if (!block0) pieces.push_back({fields[2 * f], 0u, 0u, 0u, f});
        pieces.back().field |= 0x80000000u;
    }
    double *part = workspace, *first = workspace + (int64_t)F * list_len * FD_M2 * K, *central = first + (int64_t)F * FD_M1 * K;

    auto pass = [&](bool second) {
        for (size_t at = 0; at < pieces.size(); at += FD_PIECES) {
            const unsigned n = (unsigned)std::min<size_t>(FD_PIECES, pieces.size() - at);
            FdBatch batch = {};
            std::copy(pieces.begin() + at, pieces.begin() + at + n, batch.piece);
            // (the bands a lane owns: one where that covers K, else as many as cover OT_CHROM_MAX_BANDS)
            if (!second)
                hipLaunchKernelGGL(K <= FdRoles<FD_M1>::J ? fd_first_kernel<1> : fd_first_kernel<FD_NC1>, dim3(list_len, n),
                                   dim3(OT_RED_THREADS), 0, st, rays->p, rays->w, rays->wl, key, key_first, N, nt, k, batch, K, list_len,
                                   origin[0], origin[1], origin[2], part);
            else
                hipLaunchKernelGGL(K <= FdRoles<FD_M2>::J ? fd_central_kernel<1> : fd_central_kernel<FD_NC2>, dim3(list_len, n),
                                   dim3(OT_RED_THREADS), 0, st, rays->p, rays->w, key, key_first, N, nt, k, batch, K, list_len, origin[0],
                                   origin[1], origin[2], (const double*)first, part);
        }
        const int M = (int)(K * (second ? FD_M2 : FD_M1));
        hipLaunchKernelGGL(reduce_final_kernel, dim3(F), dim3(OT_RED_THREADS), 0, st, part, (int)list_len, M, 0u, 0u,
                           second ? central : first, (int64_t)list_len * M, (int64_t)M);
    };
    pass(false);
    pass(true);
    hipLaunchKernelGGL(fd_finish_kernel, grid_for((int64_t)F * K), dim3(256), 0, st, (int)(F * K), (const double*)first,
                       (const double*)central, records);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
