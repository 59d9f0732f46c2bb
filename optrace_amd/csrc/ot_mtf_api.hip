// C-ABI, MTF analysis: per field point, band of wavelengths, plane and spatial frequency the geometric OTF sums of the ray lines of
// a stored trace, tangential and sagittal (Raytracer.mtf_analysis).
#include "ot_host.hpp"
#include "ot_mtf.hpp"

static bool mt_shape_ok(int32_t n_fields, int32_t n_bands, int32_t n_planes, int32_t n_freq) {
    return n_fields >= 1 && n_fields <= OT_FIELD_MAX_FIELDS && n_bands >= 1 && n_bands <= OT_CHROM_MAX_BANDS && n_planes >= 1 &&
           n_planes <= OT_MTF_MAX_PLANES && n_freq >= 1 && n_freq <= OT_MTF_MAX_FREQ;
}

static int64_t mt_groups(int32_t n_bands) { return (n_bands + mt_group(n_bands) - 1) / mt_group(n_bands); }
static int64_t mt_tiles(int32_t n_bands, int32_t n_planes, int32_t n_freq) {
    const int tile = mt_tile(mt_group(n_bands));
    return ((int64_t)n_planes * n_freq + tile - 1) / tile;
}

// Most workgroups per piece: about OT_MTF_BLOCKS over the groups of bands and the tiles of the grid, OT_MTF_MIN_BLOCKS at the
// least -- the work of a ray grows with groups * tiles, the workgroups that share a field's rays need not.
static int64_t mt_block_cap(int64_t groups, int64_t tiles) {
    return std::max<int64_t>(OT_MTF_MIN_BLOCKS, OT_MTF_BLOCKS / (groups * tiles));
}

// Workgroups of a field over all its pieces, from the field's count and (K, Z, Q) alone
static int64_t mt_field_blocks(int64_t count, int64_t cap) {
    int64_t total = 0;
    for_ray_chunks(0, count, [&](int64_t, uint32_t n) { total += reduce_blocks(n, cap); });
    return total;
}

static int64_t mt_list_len(const int64_t* fields, int32_t n_fields, int64_t cap) {
    int64_t len = 1;
    for (int32_t f = 0; f < n_fields; f++) len = std::max(len, mt_field_blocks(fields[2 * f + 1], cap));
    return len;
}

extern "C" int64_t ot_mtf_workspace(const int64_t* fields, int32_t n_fields, int32_t n_bands, int32_t n_planes, int32_t n_freq) {
    if (!fields || !mt_shape_ok(n_fields, n_bands, n_planes, n_freq)) return 0;
    for (int32_t f = 0; f < n_fields; f++)
        if (fields[2 * f + 1] < 0) return 0;
    // the partials [F][list][groups][tiles][cell]
    const int64_t groups = mt_groups(n_bands), tiles = mt_tiles(n_bands, n_planes, n_freq);
    return (int64_t)n_fields * mt_list_len(fields, n_fields, mt_block_cap(groups, tiles)) * groups * tiles * mt_cell(mt_group(n_bands));
}

extern "C" int ot_mtf_sums(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key,
                           int64_t key_first, int32_t n_bands, const double* origin, const double* records, const double* t,
                           const double* zeta, int32_t n_planes, const double* freq, int32_t n_freq, double* workspace, double* sums,
                           void* stream) {
    if (!fields || !key || !origin || !records || !t || !zeta || !freq || !workspace || !sums)
        return fail(OT_ERR_INVALID, "ot_mtf_sums: null argument");
    if (!mt_shape_ok(n_fields, n_bands, n_planes, n_freq))
        return fail(OT_ERR_UNSUPPORTED, "ot_mtf_sums: n_fields outside 1 .. " + std::to_string(OT_FIELD_MAX_FIELDS) +
                                            ", n_bands outside 1 .. " + std::to_string(OT_CHROM_MAX_BANDS) + ", n_planes outside 1 .. " +
                                            std::to_string(OT_MTF_MAX_PLANES) + " or n_freq outside 1 .. " +
                                            std::to_string(OT_MTF_MAX_FREQ));
    int64_t rays_total = 0;
    for (int32_t f = 0; f < n_fields; f++) {
        if (const char* bad = bad_section_sphere(rays, fields[2 * f], fields[2 * f + 1], section, false, nullptr, 0.0))
            return fail(OT_ERR_INVALID, std::string("ot_mtf_sums: ") + bad);
        if (fields[2 * f + 1] > 0 && fields[2 * f] < key_first) return fail(OT_ERR_INVALID, "ot_mtf_sums: a field starts before key_first");
        rays_total += fields[2 * f + 1];
    }
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
        return fail(OT_ERR_INVALID, "ot_mtf_sums: origin not finite");
    for (int32_t i = 0; i < 2 * n_fields; i++)
        if (!std::isfinite(t[i])) return fail(OT_ERR_INVALID, "ot_mtf_sums: t not finite");
    for (int32_t j = 0; j < n_planes; j++)
        if (!std::isfinite(zeta[j])) return fail(OT_ERR_INVALID, "ot_mtf_sums: zeta not finite");
    if (rays_total == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned K = (unsigned)n_bands, F = (unsigned)n_fields, Z = (unsigned)n_planes, Q = (unsigned)n_freq;
    const unsigned KB = (unsigned)mt_group(n_bands), groups = (unsigned)mt_groups(n_bands);
    const unsigned tiles = (unsigned)mt_tiles(n_bands, n_planes, n_freq);
    const int64_t cap = mt_block_cap(groups, tiles);
    const unsigned list_len = (unsigned)mt_list_len(fields, n_fields, cap);

    // the pieces and the length of every field's list, from the counts alone
    std::vector<MtPiece> pieces;
    MtLists lists = {};
    for (unsigned f = 0; f < F; f++) {
        uint32_t block0 = 0;
        for_ray_chunks(fields[2 * f], fields[2 * f + 1], [&](int64_t base, uint32_t n) {
            const uint32_t blocks = reduce_blocks(n, cap);
            pieces.push_back({base, n, blocks, block0, f, t[2 * f], t[2 * f + 1]});
            block0 += blocks;
        });
        lists.blocks[f] = block0;
    }
    MtPlanes planes = {};
    std::copy(zeta, zeta + n_planes, planes.zeta);

    for (size_t at = 0; at < pieces.size(); at += MT_PIECES) {
        const unsigned n = (unsigned)std::min<size_t>(MT_PIECES, pieces.size() - at);
        MtBatch batch = {};
        std::copy(pieces.begin() + at, pieces.begin() + at + n, batch.piece);
        unsigned most = 1;
        for (unsigned i = 0; i < n; i++) most = std::max(most, batch.piece[i].blocks);
        auto kernel = KB == 1 ? mt_sums_kernel<1> : KB == 2 ? mt_sums_kernel<2> : KB == 3 ? mt_sums_kernel<3> : mt_sums_kernel<4>;
        hipLaunchKernelGGL(kernel, dim3(most, n, groups * tiles), dim3(OT_RED_THREADS), 0, st, rays->p, rays->w, key, key_first,
                           rays->N, rays->nt, section, batch, planes, K, Z, Q, tiles, list_len, origin[0], origin[1], origin[2], records,
                           freq, workspace);
    }
    const int64_t total = (int64_t)F * K * Z * Q * 4;
    hipLaunchKernelGGL(mt_final_kernel, grid_for(total), dim3(OT_RED_THREADS), 0, st, (const double*)workspace, lists, total, K, Z, Q,
                       KB, (unsigned)mt_tile((int)KB), tiles, list_len, sums);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
