// C-ABI, Huygens PSF across the field: ray records against the sphere of every ray's cell, their coherent sum per (field, band)
// and plane in one launch, the combine step per field and the transfer function along each field's tangential and sagittal
// direction (Raytracer.huygens_field).
#include <cstring>

#include "ot_host.hpp"
// The lanes' arithmetic of the sum (psf_lane_points, psf_ray_points, psf_store) and the chunk rule (psf_stack_shape) are those of
// ot_psf.hpp; its kernels are defined in ot_psf_api.hip alone.
#define OT_PSF_NO_KERNELS
#include "ot_psf.hpp"
#include "ot_psf_field.hpp"

static_assert(OT_PSF_MAX_BANDS == OT_PSF_MAX_BANDS_ && OT_PSF_MAX_PLANES == OT_PSF_MAX_PLANES_ && OT_CHROM_MAX_BANDS == OT_PSF_MAX_BANDS,
              "limits of the header and the kernels");

static int bad_field_counts(const char* name, int32_t n_fields, int32_t n_bands, int32_t n_px, int32_t n_planes) {
    const std::string at = std::string(name) + ": ";
    if (n_fields < 1) return fail(OT_ERR_INVALID, at + "n_fields below 1");
    if (n_fields > OT_FIELD_MAX_FIELDS) return fail(OT_ERR_UNSUPPORTED, at + "n_fields above 64");
    if (n_bands < 1) return fail(OT_ERR_INVALID, at + "n_bands below 1");
    if (n_bands > OT_PSF_MAX_BANDS) return fail(OT_ERR_UNSUPPORTED, at + "n_bands above 32");
    if (n_px < 1) return fail(OT_ERR_INVALID, at + "n_px below 1");
    if (n_px > OT_PSF_MAX_PX) return fail(OT_ERR_UNSUPPORTED, at + "n_px above 1024");
    if (n_planes < 1) return fail(OT_ERR_INVALID, at + "n_planes below 1");
    if (n_planes > OT_PSF_MAX_PLANES) return fail(OT_ERR_UNSUPPORTED, at + "n_planes above 64");
    return OT_OK;
}

// The chunk rule: psf_stack_shape for a field of mean size, ceil(n / live) records, live the fields that hold a record -- every
// such field is aimed at the workgroups of a stack of its own, so that a chunk is as long as in a call per field and the launch
// has `live` times the rounds of one; a field without a record changes no bit of the others.  (With the chunk length of all n
// records in one stack the launch was slower than a loop over the fields: DESIGN.md section 7.)  With one field it is the stack's.
static PsfShape psf_field_shape(int64_t n, int live, int n_px, int n_planes) {
    if (live < 1) live = 1;
    return psf_stack_shape((n + live - 1) / live, n_px, n_planes);
}
static int psf_live_fields(const int64_t* starts, int n_fields, int n_bands) {
    int live = 0;
    for (int f = 0; f < n_fields; f++) live += starts[(f + 1) * n_bands] > starts[f * n_bands];
    return live;
}
// chunks of the workspace: a bound that needs no starts.  Cell c has ceil(n_c / chunk_len) chunks, all cells together less than
// n / chunk_len + cells; with g live fields n / chunk_len <= g * chunks of their shape: the largest over g <= n_fields, + cells - 1.
static int64_t psf_field_chunks(int64_t n, int n_fields, int n_bands, int n_px, int n_planes) {
    int64_t most = 0;
    for (int g = 1; g <= n_fields; g++) most = std::max(most, g * psf_field_shape(n, g, n_px, n_planes).chunks);
    return most + (int64_t)n_fields * n_bands - 1;
}
#define OT_PSFF_MAX_CHUNKS 65535  // the grid's second dimension

extern "C" int64_t ot_psf_field_workspace(int64_t n, int32_t n_fields, int32_t n_bands, int32_t n_px, int32_t n_planes) {
    if (n < 0 || n_fields < 1 || n_fields > OT_FIELD_MAX_FIELDS || n_bands < 1 || n_bands > OT_PSF_MAX_BANDS || n_px < 1 ||
        n_px > OT_PSF_MAX_PX || n_planes < 1 || n_planes > OT_PSF_MAX_PLANES)
        return 0;
    return (int64_t)n_planes * psf_field_chunks(n, n_fields, n_bands, n_px, n_planes) * psf_shape(n, n_px).stride;
}

extern "C" int ot_psf_field_rays(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key,
                                 int64_t key_first, int64_t span, int32_t n_bands, const double* spheres, const double* opl,
                                 const double* moments, double* rec, void* stream) {
    if ((rays && !rays->wl) || !fields || !key || !spheres || !opl || !moments || !rec)
        return fail(OT_ERR_INVALID, "ot_psf_field_rays: null argument");
    if (n_fields < 1 || n_bands < 1) return fail(OT_ERR_INVALID, "ot_psf_field_rays: n_fields or n_bands below 1");
    if (n_fields > OT_FIELD_MAX_FIELDS || n_bands > OT_PSF_MAX_BANDS)
        return fail(OT_ERR_UNSUPPORTED, "ot_psf_field_rays: n_fields above 64 or n_bands above 32");
    if (const char* bad = bad_section_sphere(rays, key_first, span, section, true, nullptr, 0.0))
        return fail(OT_ERR_INVALID, std::string("ot_psf_field_rays: ") + bad);
    PsfFieldRanges G = {};
    for (int32_t f = 0; f < n_fields; f++) {
        const int64_t first = fields[2 * f], count = fields[2 * f + 1];
        if (first < 0 || count < 0 || first + count > rays->N) return fail(OT_ERR_INVALID, "ot_psf_field_rays: ray range outside the storage");
        if (count > 0 && (first < key_first || first + count > key_first + span))
            return fail(OT_ERR_INVALID, "ot_psf_field_rays: a field outside the span");
        G.first[f] = first;
        G.count[f] = count;
    }
    if (span == 0) return OT_OK;
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(psf_field_rays_kernel, grid_for(span), dim3(OT_PSF_THREADS), 0, (hipStream_t)stream, *rays, G, (int)n_fields,
                       (int)section, key, key_first, span, (int)n_bands, spheres, opl, moments, rec);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_psf_field_sum(int64_t n, const double* rec, int32_t n_fields, int32_t n_bands, const int64_t* starts,
                                const double* radius, int32_t n_px, double size, int32_t n_planes, const double* dz, int64_t* table,
                                double* workspace, double* field, double* sums, void* stream) {
    if (n < 0 || !rec || !starts || !radius || !dz || !table || !workspace || !field || !sums)
        return fail(OT_ERR_INVALID, "ot_psf_field_sum: null argument");
    if (int rc = bad_field_counts("ot_psf_field_sum", n_fields, n_bands, n_px, n_planes)) return rc;
    const int cells = n_fields * n_bands;
    if (starts[0] != 0 || starts[cells] != n) return fail(OT_ERR_INVALID, "ot_psf_field_sum: starts do not run from 0 to n");
    for (int c = 0; c < cells; c++)
        if (starts[c] > starts[c + 1]) return fail(OT_ERR_INVALID, "ot_psf_field_sum: starts not ascending");
    if (!std::isfinite(size) || !(size > 0.0)) return fail(OT_ERR_INVALID, "ot_psf_field_sum: size not finite or not above zero");
    for (int z = 0; z < n_planes; z++)
        if (!std::isfinite(dz[z])) return fail(OT_ERR_INVALID, "ot_psf_field_sum: dz not finite");
    for (int f = 0; f < n_fields; f++)
        if (!std::isfinite(radius[f]) || radius[f] == 0.0) return fail(OT_ERR_INVALID, "ot_psf_field_sum: radius not finite, or zero");
    const PsfShape s = psf_field_shape(n, psf_live_fields(starts, n_fields, n_bands), n_px, n_planes);
    const int64_t px = (int64_t)n_px * n_px, most = psf_field_chunks(n, n_fields, n_bands, n_px, n_planes);
    if ((int64_t)n_planes * most * s.stride + (int64_t)n_fields * n_planes * n_bands * 2 * px > OT_PSF_STACK_CAP)
        return fail(OT_ERR_UNSUPPORTED,
                    "ot_psf_field_sum: workspace and field above 2^28 doubles: fewer fields, planes, bands or image points per call");
    if (most > OT_PSFF_MAX_CHUNKS)
        return fail(OT_ERR_UNSUPPORTED, "ot_psf_field_sum: more than 65535 chunks of records: fewer fields or records per call");
    if (n == 0) return OT_OK;
    // the cell table: start | chunk0 | |R| | sign R
    std::vector<int64_t> tab(OT_PSF_FIELD_TABLE(cells));
    int64_t chunk0 = 0;
    for (int c = 0; c <= cells; c++) {
        tab[c] = starts[c];
        if (c > 0) chunk0 += (starts[c] - starts[c - 1] + s.chunk_len - 1) / s.chunk_len;
        tab[cells + 1 + c] = chunk0;
    }
    for (int c = 0; c < cells; c++) {
        const double ax = std::fabs(radius[c / n_bands]), sg = radius[c / n_bands] > 0.0 ? 1.0 : -1.0;
        std::memcpy(&tab[2 * cells + 2 + c], &ax, sizeof(double));
        std::memcpy(&tab[3 * cells + 2 + c], &sg, sizeof(double));
    }
    const int64_t chunks = chunk0;
    PsfFieldPlanes Z;
    for (int z = 0; z < OT_PSF_MAX_PLANES; z++) Z.dz[z] = z < n_planes ? dz[z] : 0.0;
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    HIP_TRY(hipMemcpyAsync(table, tab.data(), sizeof(int64_t) * tab.size(), hipMemcpyHostToDevice, st));
    hipLaunchKernelGGL(psf_field_sum_kernel, dim3((unsigned)s.tiles, (unsigned)chunks, (unsigned)n_planes), dim3(OT_PSF_THREADS), 0, st, n,
                       rec, (const int64_t*)table, cells, s.chunk_len, (int)n_px, size, Z, workspace);
    hipLaunchKernelGGL(psf_field_final_kernel, dim3(grid_for(s.stride).x, (unsigned)cells, (unsigned)n_planes), dim3(OT_PSF_THREADS), 0, st,
                       (const double*)workspace, chunks, s.P, (const int64_t*)table, cells, (int)n_bands, field, sums);
    hipLaunchKernelGGL(psf_field_kappa_kernel, dim3((unsigned)cells), dim3(OT_PSF_THREADS), 0, st, n, rec, (const int64_t*)table, cells,
                       (int)n_bands, (int)n_planes, sums);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_psf_field_combine(int32_t n_fields, int32_t n_bands, int32_t n_planes, int32_t n_px, const double* field,
                                    const double* sums, double* intensity, double* band_strehl, double* strehl, double* g,
                                    double* noise_floor, void* stream) {
    if (!field || !sums || !intensity || !band_strehl || !strehl || !g || !noise_floor)
        return fail(OT_ERR_INVALID, "ot_psf_field_combine: null argument");
    if (int rc = bad_field_counts("ot_psf_field_combine", n_fields, n_bands, n_px, n_planes)) return rc;
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(psf_field_combine_kernel, dim3(grid_for((int64_t)n_px * n_px + 1).x, (unsigned)n_planes, (unsigned)n_fields),
                       dim3(OT_PSF_THREADS), 0, (hipStream_t)stream, (int)n_bands, (int)n_px, field, sums, intensity, band_strehl, strehl, g,
                       noise_floor);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_psf_field_otf(int32_t n_fields, int32_t n_planes, int32_t n_px, double size, const double* intensity,
                                const double* noise_floor, const double* t, int32_t n_freq, const double* frequencies, double* out,
                                void* stream) {
    if (!intensity || !noise_floor || !t || !frequencies || !out) return fail(OT_ERR_INVALID, "ot_psf_field_otf: null argument");
    if (int rc = bad_field_counts("ot_psf_field_otf", n_fields, 1, n_px, n_planes)) return rc;
    if (n_freq < 1) return fail(OT_ERR_INVALID, "ot_psf_field_otf: n_freq below 1");
    if (n_freq > OT_PSFF_MAX_FREQ) return fail(OT_ERR_UNSUPPORTED, "ot_psf_field_otf: n_freq above 64");
    if (!std::isfinite(size) || !(size > 0.0)) return fail(OT_ERR_INVALID, "ot_psf_field_otf: size not finite or not above zero");
    PsfFieldOtf D = {};
    for (int f = 0; f < n_fields; f++) {
        if (!std::isfinite(t[2 * f]) || !std::isfinite(t[2 * f + 1])) return fail(OT_ERR_INVALID, "ot_psf_field_otf: direction not finite");
        D.t[f][0] = t[2 * f];
        D.t[f][1] = t[2 * f + 1];
    }
    const double limit = (double)n_px / (2.0 * size);
    for (int m = 0; m < n_freq; m++) {
        if (!std::isfinite(frequencies[m]) || frequencies[m] < 0.0)
            return fail(OT_ERR_INVALID, "ot_psf_field_otf: frequency not finite or below zero");
        if (frequencies[m] > limit) return fail(OT_ERR_INVALID, "ot_psf_field_otf: frequency above the sampling limit n_px / (2 size)");
        D.nu[m] = frequencies[m];
    }
    if (int rc = require_device()) return rc;
    hipLaunchKernelGGL(psf_field_otf_kernel,
                       dim3((unsigned)((n_freq + OT_PSFF_FREQ_BLOCK - 1) / OT_PSFF_FREQ_BLOCK), (unsigned)n_planes, (unsigned)n_fields),
                       dim3(OT_RED_THREADS), 0, (hipStream_t)stream, (int)n_px, size, (int)n_freq, D, intensity, noise_floor, out);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}
