// C-ABI, spot diagrams: per field point, band of wavelengths and plane the power map of where the ray lines of a stored trace land
// about a centre, its counts, and the largest and the mean squared distance from the centre (Raytracer.spot_diagram).
#include "ot_host.hpp"
#include "ot_spot_diagram.hpp"

static bool sd_shape_ok(int32_t n_fields, int32_t n_bands, int32_t n_planes) {
    return n_fields >= 1 && n_fields <= OT_FIELD_MAX_FIELDS && n_bands >= 1 && n_bands <= OT_CHROM_MAX_BANDS && n_planes >= 1 &&
           n_planes <= OT_MTF_MAX_PLANES;
}

static int64_t sd_groups(int32_t n_bands) { return (n_bands + sd_group(n_bands) - 1) / sd_group(n_bands); }
static int64_t sd_tiles(int32_t n_bands, int32_t n_planes) {
    const int tile = sd_tile(sd_group(n_bands));
    return ((int64_t)n_planes + tile - 1) / tile;
}

// Most workgroups per piece of the extent pass: about OT_SD_BLOCKS over the groups of bands and the tiles of planes
static int64_t sd_block_cap(int64_t groups, int64_t tiles) { return std::max<int64_t>(OT_SD_MIN_BLOCKS, OT_SD_BLOCKS / (groups * tiles)); }

static int64_t sd_field_blocks(int64_t count, int64_t cap) {
    int64_t total = 0;
    for_ray_chunks(0, count, [&](int64_t, uint32_t n) { total += reduce_blocks(n, cap); });
    return total;
}

static int64_t sd_list_len(const int64_t* fields, int32_t n_fields, int64_t cap) {
    int64_t len = 1;
    for (int32_t f = 0; f < n_fields; f++) len = std::max(len, sd_field_blocks(fields[2 * f + 1], cap));
    return len;
}

// (band, plane) tiles a workgroup of the map pass holds in LDS; 0: one tile alone exceeds the budget
static int64_t sd_chunk_tiles(int32_t n_bands, int32_t n_planes, int32_t n_px) {
    const int64_t per_tile = (int64_t)n_px * n_px * 8 + SD_TILE_AUX;
    return std::min<int64_t>(OT_SD_LDS_BYTES / per_tile, (int64_t)n_bands * n_planes);
}

extern "C" int64_t ot_spotdiag_workspace(const int64_t* fields, int32_t n_fields, int32_t n_bands, int32_t n_planes) {
    if (!fields || !sd_shape_ok(n_fields, n_bands, n_planes)) return 0;
    for (int32_t f = 0; f < n_fields; f++)
        if (fields[2 * f + 1] < 0) return 0;
    // the partials [F][list][groups][tiles][cell]
    const int64_t groups = sd_groups(n_bands), tiles = sd_tiles(n_bands, n_planes);
    return (int64_t)n_fields * sd_list_len(fields, n_fields, sd_block_cap(groups, tiles)) * groups * tiles * sd_cell(sd_group(n_bands));
}

extern "C" int32_t ot_spotdiag_chunks(int32_t n_bands, int32_t n_planes, int32_t n_px) {
    if (!sd_shape_ok(1, n_bands, n_planes) || n_px < 1 || n_px > OT_SD_MAX_PX) return 0;
    const int64_t T = sd_chunk_tiles(n_bands, n_planes, n_px);
    return T ? (int32_t)(((int64_t)n_bands * n_planes + T - 1) / T) : 1;
}

// The checks the two passes share, answered before a device is looked for.  -> OT_OK and the rays of all fields
static int sd_check(const char* who, const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key,
                    int64_t key_first, int32_t n_bands, const double* origin, const double* centre, const double* zeta, int32_t n_planes,
                    int64_t* rays_total) {
    const std::string name = std::string(who) + ": ";
    if (!fields || !key || !origin || !centre || !zeta) return fail(OT_ERR_INVALID, name + "null argument");
    if (!sd_shape_ok(n_fields, n_bands, n_planes))
        return fail(OT_ERR_UNSUPPORTED, name + "n_fields outside 1 .. " + std::to_string(OT_FIELD_MAX_FIELDS) + ", n_bands outside 1 .. " +
                                            std::to_string(OT_CHROM_MAX_BANDS) + " or n_planes outside 1 .. " +
                                            std::to_string(OT_MTF_MAX_PLANES));
    *rays_total = 0;
    for (int32_t f = 0; f < n_fields; f++) {
        if (const char* bad = bad_section_sphere(rays, fields[2 * f], fields[2 * f + 1], section, false, nullptr, 0.0))
            return fail(OT_ERR_INVALID, name + bad);
        if (fields[2 * f + 1] > 0 && fields[2 * f] < key_first) return fail(OT_ERR_INVALID, name + "a field starts before key_first");
        *rays_total += fields[2 * f + 1];
    }
    if (!std::isfinite(origin[0]) || !std::isfinite(origin[1]) || !std::isfinite(origin[2]))
        return fail(OT_ERR_INVALID, name + "origin not finite");
    for (int32_t j = 0; j < n_planes; j++)
        if (!std::isfinite(zeta[j])) return fail(OT_ERR_INVALID, name + "zeta not finite");
    return OT_OK;
}

// The pieces of every field, `cap` workgroups of `threads` per piece at the most; lists (optional): the workgroups of every field
static std::vector<SdPiece> sd_pieces(const int64_t* fields, unsigned F, int64_t threads, int64_t cap, SdLists* lists) {
    std::vector<SdPiece> pieces;
    for (unsigned f = 0; f < F; f++) {
        uint32_t block0 = 0;
        for_ray_chunks(fields[2 * f], fields[2 * f + 1], [&](int64_t base, uint32_t n) {
            const uint32_t blocks = (uint32_t)std::max<int64_t>(1, std::min<int64_t>((n + threads - 1) / threads, cap));
            pieces.push_back({base, n, blocks, block0, f});
            block0 += blocks;
        });
        if (lists) lists->blocks[f] = block0;
    }
    return pieces;
}

extern "C" int ot_spotdiag_extent(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key,
                                  int64_t key_first, int32_t n_bands, const double* origin, const double* centre, const double* zeta,
                                  int32_t n_planes, double* workspace, double* ext, void* stream) {
    if (!workspace || !ext) return fail(OT_ERR_INVALID, "ot_spotdiag_extent: null argument");
    int64_t rays_total = 0;
    if (int rc = sd_check("ot_spotdiag_extent", rays, fields, n_fields, section, key, key_first, n_bands, origin, centre, zeta, n_planes,
                          &rays_total))
        return rc;
    if (rays_total == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned K = (unsigned)n_bands, F = (unsigned)n_fields, Z = (unsigned)n_planes;
    const unsigned KB = (unsigned)sd_group(n_bands), groups = (unsigned)sd_groups(n_bands), tiles = (unsigned)sd_tiles(n_bands, n_planes);
    const int64_t cap = sd_block_cap(groups, tiles);
    const unsigned list_len = (unsigned)sd_list_len(fields, n_fields, cap);
    SdLists lists = {};
    const std::vector<SdPiece> pieces = sd_pieces(fields, F, OT_RED_THREADS, cap, &lists);
    SdPlanes planes = {};
    std::copy(zeta, zeta + n_planes, planes.zeta);

    for (size_t at = 0; at < pieces.size(); at += SD_PIECES) {
        const unsigned n = (unsigned)std::min<size_t>(SD_PIECES, pieces.size() - at);
        SdBatch batch = {};
        std::copy(pieces.begin() + at, pieces.begin() + at + n, batch.piece);
        unsigned most = 1;
        for (unsigned i = 0; i < n; i++) most = std::max(most, batch.piece[i].blocks);
        auto kernel = KB == 1 ? sd_extent_kernel<1> : KB == 2 ? sd_extent_kernel<2> : KB == 3 ? sd_extent_kernel<3> : sd_extent_kernel<4>;
        hipLaunchKernelGGL(kernel, dim3(most, n, groups * tiles), dim3(OT_RED_THREADS), 0, st, rays->p, rays->w, key, key_first, rays->N,
                           rays->nt, section, batch, planes, K, Z, tiles, list_len, origin[0], origin[1], origin[2], centre, workspace);
    }
    const int64_t total = (int64_t)F * K * Z * 2;
    hipLaunchKernelGGL(sd_extent_final_kernel, grid_for(total), dim3(OT_RED_THREADS), 0, st, (const double*)workspace, lists, total, K, Z,
                       KB, (unsigned)sd_tile((int)KB), tiles, list_len, ext);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

// The map kernel's dynamic LDS goes beyond the 64 KiB a kernel gets unasked: raised once per device (hipFuncSetAttribute sets a
// property of the function on the current device).
static int sd_map_setup() {
    static bool done[64] = {};
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    if (dev < 0 || dev >= 64) return fail(OT_ERR_UNSUPPORTED, "ot_spotdiag_maps: device index beyond 63");
    if (!done[dev]) {
        HIP_TRY(hipFuncSetAttribute((const void*)sd_map_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, OT_SD_LDS_BYTES));
        done[dev] = true;
    }
    return OT_OK;
}

extern "C" int ot_spotdiag_maps(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key,
                                int64_t key_first, int32_t n_bands, const double* origin, const double* centre, const double* zeta,
                                int32_t n_planes, int32_t n_px, double size, double* maps, uint64_t* counts, double* outside_power,
                                void* stream) {
    if (!maps || !counts || !outside_power) return fail(OT_ERR_INVALID, "ot_spotdiag_maps: null argument");
    int64_t rays_total = 0;
    if (int rc = sd_check("ot_spotdiag_maps", rays, fields, n_fields, section, key, key_first, n_bands, origin, centre, zeta, n_planes,
                          &rays_total))
        return rc;
    if (n_px < 1 || n_px > OT_SD_MAX_PX)
        return fail(OT_ERR_UNSUPPORTED, "ot_spotdiag_maps: n_px outside 1 .. " + std::to_string(OT_SD_MAX_PX));
    if ((int64_t)n_fields * n_bands * n_planes * n_px * n_px > OT_SD_MAX_CELLS)
        return fail(OT_ERR_UNSUPPORTED, "ot_spotdiag_maps: more than " + std::to_string(OT_SD_MAX_CELLS) + " cells in all");
    if (!std::isfinite(size) || !(size > 0.0)) return fail(OT_ERR_INVALID, "ot_spotdiag_maps: size not finite or not above 0");
    if (rays_total == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    if (int rc = sd_map_setup()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const unsigned K = (unsigned)n_bands, F = (unsigned)n_fields, Z = (unsigned)n_planes;
    const int64_t fit = sd_chunk_tiles(n_bands, n_planes, n_px);
    const unsigned T = fit ? (unsigned)fit : K * Z, chunks = (K * Z + T - 1) / T;
    const size_t lds = (fit ? (size_t)T * n_px * n_px * 8 : 0) + (size_t)T * SD_TILE_AUX;  // (all K Z <= 2080 tiles' counters: 83 KB)
    // a workgroup per 1024 rays, about OT_SD_MAP_BLOCKS per piece over the chunks: each zeroes and flushes its chunk once
    const std::vector<SdPiece> pieces = sd_pieces(fields, F, SD_MAP_THREADS, std::max<int64_t>(OT_SD_MAP_MIN_BLOCKS, OT_SD_MAP_BLOCKS / chunks), nullptr);
    SdPlanes planes = {};
    std::copy(zeta, zeta + n_planes, planes.zeta);
    for (size_t at = 0; at < pieces.size(); at += SD_PIECES) {
        const unsigned n = (unsigned)std::min<size_t>(SD_PIECES, pieces.size() - at);
        SdBatch batch = {};
        std::copy(pieces.begin() + at, pieces.begin() + at + n, batch.piece);
        unsigned most = 1;
        for (unsigned i = 0; i < n; i++) most = std::max(most, batch.piece[i].blocks);
        hipLaunchKernelGGL(sd_map_kernel, dim3(most, n, chunks), dim3(SD_MAP_THREADS), lds, st, rays->p, rays->w, key, key_first, rays->N,
                           rays->nt, section, batch, planes, K, Z, T, n_px, fit ? 1 : 0, origin[0], origin[1], origin[2], centre, size, maps,
                           (unsigned long long*)counts, outside_power);
    }
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
