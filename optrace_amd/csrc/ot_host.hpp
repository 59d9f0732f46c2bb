// Host plumbing shared by the translation units of the C-ABI (ot_api.hip and ot_*_api.hip, one per stage): error reporting,
// launch shapes, the checks of a ray section, the scratch pool's front door, surface compilation and the source ranges.
// Functions are declared here and defined once, in the unit named beside them.  All of them are internal to the library:
// hidden visibility, so that the dynamic symbol table holds the C-ABI and the kernels' host stubs.
#pragma once
#include <stdint.h>

// ---- ray chunks -----------------------------------------------------------------------------------------------------
// Kernels with one ray per lane address their ray with 32-bit byte offsets from base pointers the host advances: a launch
// covers at most 2^28 rays.  fn(base, n) is called for consecutive pieces of [first, first + count), n <= OT_RAY_CHUNK.
// (Plain C++ ahead of the HIP includes: tests/cpp/ray_chunks_test.cpp compiles it with OT_HOST_CHUNKS_ONLY and no HIP.)
#define OT_RAY_CHUNK ((int64_t)1 << 28)
template <class F>
static inline void for_ray_chunks(int64_t first, int64_t count, F&& fn) {
    for (int64_t base = first; base < first + count; base += OT_RAY_CHUNK) {
        const int64_t left = first + count - base;
        fn(base, (uint32_t)(left < OT_RAY_CHUNK ? left : OT_RAY_CHUNK));
    }
}

#ifndef OT_HOST_CHUNKS_ONLY
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "ot_scene.hpp"
#include "ot_scratch.hpp"

#define OT_INTERNAL __attribute__((visibility("hidden")))

// ---- errors (ot_api.hip: the one thread-local message behind ot_last_error) -----------------------------------------
OT_INTERNAL int fail(int code, const std::string& msg);

#define HIP_TRY(expr)                                                                                   \
    do {                                                                                                \
        hipError_t e_ = (expr);                                                                         \
        if (e_ != hipSuccess)                                                                           \
            return fail(OT_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));                 \
    } while (0)

OT_INTERNAL int require_device();  // ot_api.hip

// ---- launch shapes and scratch layout -------------------------------------------------------------------------------
static inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + 255) / 256)); }
static inline size_t align_up(size_t v) { return (v + 255) & ~(size_t)255; }

// scratch layout: consecutive arrays, each on a 256-byte boundary
struct Carver {
    size_t off;
    size_t operator()(size_t bytes) {
        const size_t o = off;
        off = align_up(off + bytes);
        return o;
    }
};

OT_INTERNAL int cu_count();  // ot_api.hip

// Workgroups (of 256: OT_RED_THREADS) of a fixed-order reduction over n entries (ot_block_reduce.hpp), `cap` at the most: numbers
// that follow from n alone, not from the device's CU count, so that the order of the sums -- and with it their bits -- is the
// same on every device
static inline unsigned reduce_blocks(int64_t n, int64_t cap) {
    return (unsigned)std::max<int64_t>(1, std::min((n + 255) / 256, cap));
}

// Launch shape of an LDS-privatised f64 histogram over n >= 1 entries (spectrum, radial bins of the spot, pupil map): 1024
// threads, a workgroup per 1024 entries up to one per CU, and `lds_wanted` bytes of sums per workgroup if they fit into 64 KiB,
// which keeps two workgroups of LDS per CU free for other work; lds = 0 otherwise, and the kernel adds to global memory.
struct HistShape {
    dim3 grid, block;
    size_t lds;
};
static inline HistShape hist_shape(int64_t n, size_t lds_wanted) {
    const int64_t blocks = std::min<int64_t>((n + 1023) / 1024, cu_count());
    return {dim3((unsigned)blocks), dim3(1024), lds_wanted <= 64 * 1024 ? lds_wanted : 0};
}

// ---- a section of the ray storage and a sphere behind it (ot_wavefront_*, ot_psf_rays) ------------------------------------
// -> what is wrong, to follow the entry point's name in its message, or nullptr.  need_index: the index plane is read; c, radius:
// the sphere, c = nullptr where the entry point takes none.
static inline const char* bad_section_sphere(const ot_rays* rays, int64_t first, int64_t count, int32_t section, bool need_index,
                                             const double* c, double radius) {
    if (!rays || !rays->p || !rays->w || (need_index && !rays->n)) return "null argument";
    if (first < 0 || count < 0 || first + count > rays->N) return "ray range outside the storage";
    if (section < 0 || section > rays->nt - 2) return "section out of range";
    if (c && !(std::isfinite(c[0]) && std::isfinite(c[1]) && std::isfinite(c[2]) && std::isfinite(radius) && radius != 0.0))
        return "focus or radius not finite, or radius zero";
    return nullptr;
}

// ---- scratch pool (ot_api.hip, ot_scratch.hpp) ----------------------------------------------------------------------
enum { OT_WS_RENDER = 0, OT_WS_FUSED = 1, OT_WS_FUSED_HITS = 2, OT_WS_AUTO = 3, OT_WS_DET = 4, OT_WS_COLOR = 5, OT_WS_SAMPLE = 6 };

// -> lease on a block of at least `bytes` for this device, stream and purpose; empty when out of memory (the callers fall
// back to paths without scratch)
OT_INTERNAL ot_scratch::Lease workspace(int purpose, size_t bytes, hipStream_t st);

// ---- surface compilation (ot_scene_api.hip) -------------------------------------------------------------------------
OT_INTERNAL int compile_surface(const ot_surface& s, SurfDev& d);

// What goes into the device table of a compiled surface (d.tab != nullptr): the caller's spline tables as they are; for
// an asphere with more than OT_MAX_ASPH coefficients the layout of ot_device.hpp::asph_poly_long, built here:
// a[npad] | d[npad], d_j = a_j (2j + 2) as in SurfDev::dcoeff, zeros behind the last coefficient.
struct OT_INTERNAL DeviceTable {
    std::vector<double> own;
    const double* src = nullptr;
    size_t len = 0;
    DeviceTable(const ot_surface& s, const SurfDev& d);
};

// A compiled surface for the leaf entry points: its table (if any) is uploaded for the duration of the call.
struct OT_INTERNAL LeafSurface {
    SurfDev d;
    double* dev_tab = nullptr;
    hipStream_t st = nullptr;
    int init(const ot_surface* surf, hipStream_t stream);
    ~LeafSurface();
};

// ---- source ranges (ot_sources_api.hip) -----------------------------------------------------------------------------
struct RangeArgs;  // ot_trace_kernel.hpp

OT_INTERNAL void drop_range_cache(ot_sources* s);

// Fills the kernel argument block; with more than OT_MAX_RANGES ranges the records go to device memory (kept in
// the source table's cache until a different list arrives).
OT_INTERNAL int make_ranges(const ot_source_range* ranges, int32_t n_ranges, const ot_sources* src_c, int64_t N,
                            const RangeArgs** out);

// The argument block of a sampler kernel (ot_sample_api.hip): the same per-range constants, for ranges that belong to no
// source table -- at most OT_MAX_RANGES of them, in order and gap-free over [0, N); nothing goes to device memory.  `who`
// names the entry point in the messages.
OT_INTERNAL int sampler_ranges(const char* who, const ot_source_range* ranges, int32_t n_ranges, int64_t N, RangeArgs* out);

// ---- inverse-CDF tables (ot_sources_api.hip) ------------------------------------------------------------------------
// Start hints (CdfGuide, ot_scene.hpp) for the cumulative table F[n] searched over [x0, F[n - 1]]: fills dst->K, x0 and
// scale and appends the K bucket entries to `guides`; -> their offset in `guides` (dst->g is the caller's to set once the
// entries have an address on the device).
OT_INTERNAL size_t build_cdf_guide(const double* F, size_t n, double x0, CdfGuide* dst, std::vector<int32_t>& guides);

// The inverse cumulative spectra of the three sRGB primaries, 3 x (OT_PRIM_M + 1) nodes (SourceDev::prim_inv).
OT_INTERNAL const std::vector<double>& srgb_primary_inverse_tables();
#endif  // OT_HOST_CHUNKS_ONLY
