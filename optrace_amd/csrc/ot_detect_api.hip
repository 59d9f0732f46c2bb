// C-ABI, detector stage: hit search on detectors, sphere projection, the direct and tile binning paths, the fused detector
// images, the automatic-extent image and the detector spectrum.  detector_setup, the once-per-device record of the whole
// process, takes the address of kernels from every header below: they belong to this unit alone.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "ot_detector.hpp"
#include "ot_detector_fused.hpp"
#include "ot_host.hpp"
#include "ot_render_tiles.hpp"
#include "ot_spectrum.hpp"

// ---- detector + render -------------------------------------------------------------------------------------
// The one routing rule of the detector stage (detector.py uses the same, _capi.fused_ok): the fused kernels of
// ot_detector_images serve detectors with a closed-form hit (flat or conic) and no sphere projection with transcendentals;
// every other request takes the chain ot_detector_hits_multi + render_accumulate.
static bool numeric_hit(const ot_surface& s) { return !(s.kind == OT_SURF_CONIC || s.z_min == s.z_max); }
static bool fused_ok(const ot_surface& s, int32_t projection) {
    return !numeric_hit(s) && (projection == OT_PROJ_NONE || projection == OT_PROJ_ORTHOGRAPHIC);
}

extern "C" int ot_detector_hits_multi(const ot_rays* rays, int64_t first, int64_t count, const ot_detector_req* reqs,
                                      int32_t n_reqs, void* stream) {
    if (!rays || !reqs || n_reqs < 1) return fail(OT_ERR_INVALID, "ot_detector_hits: null argument");
    if (n_reqs > OT_DET_MAX) return fail(OT_ERR_INVALID, "ot_detector_hits_multi: at most 8 detectors per call");
    if (!rays->p || !rays->w) return fail(OT_ERR_INVALID, "ot_detector_hits: ray storage has null buffers");
    if (first < 0 || count < 0 || first + count > rays->N) return fail(OT_ERR_INVALID, "ot_detector_hits: range outside the storage");
    for (int k = 0; k < n_reqs; k++) {
        const ot_detector_req& q = reqs[k];
        if (!q.detector || !q.ill_count) return fail(OT_ERR_INVALID, "ot_detector_hits: null argument");
        // ph and hw both NULL: extent-only request (no hit list is written)
        // compact lists may go without positions (weights and wavelengths: the detector spectrum)
        if (q.fill && (!q.hw || !q.wl_out || !q.xy_only || !rays->wl))
            return fail(OT_ERR_INVALID, "ot_detector_hits: a compact hit list needs hw, wl_out and xy_only");
        if (!q.fill && (!q.ph || !q.hw) && (q.ph || q.hw || !q.extent4))
            return fail(OT_ERR_INVALID, "ot_detector_hits: ph and hw may only be NULL together, and only with extent4");
        if (q.projection < OT_PROJ_NONE || q.projection > OT_PROJ_STEREOGRAPHIC) return fail(OT_ERR_INVALID, "unknown projection");
    }
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::vector<LeafSurface> ls(n_reqs);
    std::vector<DetOne> host(n_reqs);
    bool numeric = false;
    int n_ext = 0;
    for (int k = 0; k < n_reqs; k++) {
        if (int rc = ls[k].init(reqs[k].detector, st)) return rc;
        n_ext += reqs[k].extent4 != nullptr;
    }
    if (count == 0) return OT_OK;
    // scratch: the detector records, then the extent slot tables -- a few KB from the kept pool (it used to come from the
    // stream-ordered pool; that cost 0.2 ms per call, and 7-58 ms whenever the driver was still busy with memory a large free
    // had returned to it, profiles/r3/readback_after_free.txt)
    const size_t o_slots = align_up(sizeof(DetOne) * OT_DET_MAX);
    const size_t total = o_slots + sizeof(unsigned long long) * 4 * OT_EXT_SLOTS * (size_t)OT_DET_MAX;
    const ot_scratch::Lease lease = workspace(OT_WS_DET, total, st);
    if (!lease) return fail(OT_ERR_HIP, "ot_detector_hits: no scratch memory");
    char* scratch = lease.p();
    unsigned long long* slots = (unsigned long long*)(scratch + o_slots);
    int e = 0;
    for (int k = 0; k < n_reqs; k++) {
        DetOne& d = host[k];
        std::memset(&d, 0, sizeof(d));
        d.det = ls[k].d;
        d.Rcurv = reqs[k].detector->R;
        if (reqs[k].crop4) d.crop = {reqs[k].crop4[0], reqs[k].crop4[1], reqs[k].crop4[2], reqs[k].crop4[3], 1};
        d.ph = reqs[k].ph;
        d.hw = reqs[k].hw;
        d.ill = (unsigned long long*)reqs[k].ill_count;
        d.projection = reqs[k].projection;
        d.xy_only = reqs[k].xy_only != 0;
        d.wl_out = reqs[k].wl_out;
        d.fill = reqs[k].fill;
        d.piece_shift = hit_piece_shift(count);
        if (reqs[k].extent4) d.ext_slots = slots + (size_t)4 * OT_EXT_SLOTS * e++;
        numeric = numeric || numeric_hit(*reqs[k].detector);
    }
    hipError_t err = hipSuccess;
    if (n_reqs > 1) err = hipMemcpyAsync(scratch, host.data(), sizeof(DetOne) * n_reqs, hipMemcpyHostToDevice, st);
    if (err == hipSuccess) {
        if (n_ext) hipLaunchKernelGGL(extent_init_kernel, dim3(n_ext), dim3(4 * OT_EXT_SLOTS), 0, st, slots);
        if (n_reqs == 1) {  // the record travels in the kernel arguments (scalar registers)
            if (numeric)
                hipLaunchKernelGGL(detector_kernel<true>, grid_for(count), dim3(256), 0, st, *rays, first, count, host[0]);
            else
                hipLaunchKernelGGL(detector_kernel<false>, grid_for(count), dim3(256), 0, st, *rays, first, count, host[0]);
        } else {
            const dim3 g = grid_for(count), b(256);
            const DetOne* dd = (const DetOne*)scratch;
#define OT_LAUNCH_DET(NUM, ND) hipLaunchKernelGGL((detector_multi_kernel<NUM, ND>), g, b, 0, st, *rays, first, count, dd, n_reqs)
            if (numeric) {
                OT_LAUNCH_DET(true, 8);
            } else {
                if (n_reqs <= 2) OT_LAUNCH_DET(false, 2);
                else if (n_reqs <= 4) OT_LAUNCH_DET(false, 4);
                else OT_LAUNCH_DET(false, 8);
            }
#undef OT_LAUNCH_DET
        }
        e = 0;
        for (int k = 0; k < n_reqs; k++)
            if (reqs[k].extent4)
                hipLaunchKernelGGL(extent_final_kernel, dim3(1), dim3(64), 0, st, slots + (size_t)4 * OT_EXT_SLOTS * e++, reqs[k].extent4);
        err = hipGetLastError();
    }
    HIP_TRY(err);
    return OT_OK;
}

extern "C" int64_t ot_hit_piece_len(int64_t count) { return hit_piece_len(count); }

extern "C" int ot_detector_hits(const ot_rays* rays, int64_t first, int64_t count, const ot_surface* detector,
                                int32_t projection, const double* crop4, double* ph, float* hw, double* extent4,
                                int64_t* ill_count, void* stream) {
    ot_detector_req q;
    q.wl_out = nullptr;
    q.fill = nullptr;
    q.detector = detector;
    q.projection = projection;
    q.xy_only = 0;
    q.crop4 = crop4;
    q.ph = ph;
    q.hw = hw;
    q.extent4 = extent4;
    q.ill_count = ill_count;
    return ot_detector_hits_multi(rays, first, count, &q, 1, stream);
}

extern "C" int ot_sphere_projection(const ot_surface* surf, int32_t projection, int64_t n, const double* p, double* out,
                                    void* stream) {
    if (!surf || n < 0 || (n && (!p || !out))) return fail(OT_ERR_INVALID, "ot_sphere_projection: bad argument");
    if (surf->kind != OT_SURF_CONIC || surf->k != 0.0) return fail(OT_ERR_INVALID, "sphere projection needs a spherical surface");
    if (projection < OT_PROJ_NONE || projection > OT_PROJ_STEREOGRAPHIC) return fail(OT_ERR_INVALID, "unknown projection");
    if (int rc = require_device()) return rc;
    if (n == 0) return OT_OK;
    hipLaunchKernelGGL(projection_kernel, grid_for(n), dim3(256), 0, (hipStream_t)stream, surf->pos[0], surf->pos[1],
                       surf->pos[2], surf->R, projection, n, p, out);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

#define OT_TILE_MIN_HITS (1ll << 21)  // shorter lists: the direct kernel alone

// ---- shared set-up of the binning paths ----------------------------------------------------------------------
#define OT_PROBE_LDS (OT_TILE_PROBE_SET * (int)sizeof(int))
#define OT_ACCUM_LDS ((OT_TILE_PX * 4 + OT_OBS_N * 6) * (int)sizeof(double))  // tile + (value, difference) observer table

// One-time set-up per device, for the whole process: the dynamic-LDS limits of the binning kernels (hipFuncSetAttribute sets
// a property of the function on the current device, not one of the calling thread) and the CIE observer table.  Marked done
// only when every step has succeeded, so that a failure is reported again by the next call.
static int detector_setup(const double** table) {
    struct PerDevice {
        bool done = false;
        double* table = nullptr;
    };
    static std::mutex mu;
    static PerDevice devs[64];
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return fail(OT_ERR_HIP, "could not upload the CIE observer table");
    std::lock_guard<std::mutex> lock(mu);
    PerDevice& d = devs[dev];
    if (!d.done) {
        if (!d.table) {
            // the 471 x 3 table, and behind it the same as (value, difference to the next row) pairs: 471 x 6 (observer_xyz_at6)
            std::vector<double> both((size_t)OT_OBS_N * 9);
            const double* src = (const double*)ot_observer_xyz;
            for (int i = 0; i < OT_OBS_N * 3; i++) both[i] = src[i];
            double* pairs = both.data() + (size_t)OT_OBS_N * 3;
            for (int j = 0; j < OT_OBS_N; j++)
                for (int c = 0; c < 3; c++) {
                    pairs[6 * j + 2 * c] = src[3 * j + c];
                    pairs[6 * j + 2 * c + 1] = (j + 1 < OT_OBS_N) ? (src[3 * (j + 1) + c] - src[3 * j + c]) / 1.0 : 0.0;  // observers.py:14-41
                }
            double* t = nullptr;
            if (hipMalloc((void**)&t, sizeof(double) * both.size()) != hipSuccess) return fail(OT_ERR_HIP, "could not upload the CIE observer table");
            if (hipMemcpy(t, both.data(), sizeof(double) * both.size(), hipMemcpyHostToDevice) != hipSuccess) {
                (void)hipFree(t);
                return fail(OT_ERR_HIP, "could not upload the CIE observer table");
            }
            d.table = t;
        }
        // the one-detector tile kernels stage their records in LDS: with many tiles more than the 64 KB a kernel gets unasked
        const int most = 96 * 1024, lb = (int)fuse_lb_lds(OT_LB_MAXK);
        const struct {
            const void* kernel;
            int bytes;
        } dynamic_lds[] = {
            {(const void*)tile_probe_kernel, OT_PROBE_LDS},
            {(const void*)tile_accum_kernel, OT_ACCUM_LDS},
            {(const void*)fuse_accum_multi_kernel, OT_ACCUM_LDS},
            {(const void*)spec_accum_kernel, OT_ACCUM_LDS},
            {(const void*)fuse_tiles_kernel<1, 1, false>, most},
            {(const void*)fuse_tiles_kernel<1, 2, false>, most},
            {(const void*)fuse_tiles_kernel<1, 1, true>, most},
            {(const void*)fuse_tiles_kernel<1, 2, true>, most},
            {(const void*)fuse_tiles_lb_kernel<false>, lb},
            {(const void*)fuse_tiles_lb_kernel<true>, lb},
        };
        for (const auto& k : dynamic_lds) HIP_TRY(hipFuncSetAttribute(k.kernel, hipFuncAttributeMaxDynamicSharedMemorySize, k.bytes));
        d.done = true;
    }
    *table = d.table;
    return OT_OK;
}

// OT_RENDER_PATH = direct | tiles pins the binning path (tests, profiling); unset: by hit count and probe
struct RenderPath {
    bool direct, tiles;
};
static RenderPath render_path() {
    const char* pin = std::getenv("OT_RENDER_PATH");
    return {pin && !std::strcmp(pin, "direct"), pin && !std::strcmp(pin, "tiles")};
}

static RenderArgs render_args(const double extent[4], int32_t Nx, int32_t Ny, double ws) {
    RenderArgs a;
    a.x0 = extent[0];
    a.x1 = extent[1];
    a.y0 = extent[2];
    a.y1 = extent[3];
    a.fx = (double)Nx / (extent[1] - extent[0]);  // Nx / s[0]  misc.py:75
    a.fy = (double)Ny / (extent[3] - extent[2]);
    a.Nx = Nx;
    a.Ny = Ny;
    a.ws = ws;
    return a;
}

static int render_accumulate(int64_t n, const unsigned int* fill, const double* px, const double* py, const float* w,
                             const float* wl, const double extent[4], int32_t Nx, int32_t Ny, double* hist, void* stream,
                             double weight_scale = 1.0) {
    if (n < 0 || !extent || !hist || Nx < 1 || Ny < 1 || (n && (!px || !py || !w || !wl)))
        return fail(OT_ERR_INVALID, "ot_render_accumulate: bad argument");
    if (int rc = require_device()) return rc;
    if (n == 0) return OT_OK;
    const RenderArgs a = render_args(extent, Nx, Ny, weight_scale);
    const double* table = nullptr;
    if (int rc = detector_setup(&table)) return rc;
    // one 1024-thread workgroup per CU (grid-stride): LDS-privatised histogram, see render_kernel
    const int64_t blocks = std::min<int64_t>((n + 1023) / 1024, cu_count());
    hipStream_t st = (hipStream_t)stream;
    // spread: device flag of the probe (the kernel returns at once where it says tiles), or none: bin everything
    const auto direct = [&](const int* spread) {
        hipLaunchKernelGGL(render_kernel, dim3((unsigned)blocks), dim3(1024), 0, st, n, px, py, w, wl, a, table, hist, spread, fill);
    };
    // long lists: a probe decides on the device whether the direct kernel or the tile path bins them
    // (ot_render_tiles.hpp); both are enqueued, the one that is not needed returns at once
    const RenderPath pin = render_path();
    TileArgs t;
    t.a = a;
    t.tx = (Nx + OT_TILE_W - 1) / OT_TILE_W;
    t.ty = (Ny + OT_TILE_W - 1) / OT_TILE_W;
    t.K = t.tx * t.ty;
    t.n = n;
    t.piece = fill ? hit_piece_len(n) : ((n + OT_TILE_PIECES - 1) / OT_TILE_PIECES + 1023) / 1024 * 1024;
    t.chunk = ((n + 1023) / 1024 + 1023) / 1024 * 1024;
    if (t.chunk < 16384) t.chunk = 16384;
    t.max_chunks = (int32_t)(n / t.chunk + t.K + 1);
    Carver carve{0};
    const size_t o_spread = carve(sizeof(int));
    const size_t o_counts = carve(sizeof(unsigned int) * OT_TILE_PIECES * (size_t)t.K);
    const size_t o_tot = carve(sizeof(unsigned long long) * t.K);
    const size_t o_starts = carve(sizeof(unsigned long long) * (t.K + 1));
    const size_t o_cstart = carve(sizeof(int) * (t.K + 1));
    const size_t o_rec = carve(sizeof(TileRec) * (size_t)n);
    const size_t o_slabs = carve(sizeof(double) * OT_TILE_PX * 4 * (size_t)t.max_chunks);
    // The direct kernel alone: pinned, a short list, more tiles than any image of RenderImage has, or no room for the hit
    // records (12 B per hit; the direct kernel needs no scratch)
    ot_scratch::Lease lease;
    if (!pin.direct && (pin.tiles || n >= OT_TILE_MIN_HITS) && t.K <= OT_TILE_MAX) lease = workspace(OT_WS_RENDER, carve.off, st);
    char* ws = lease.p();
    if (!ws) {
        direct(nullptr);
        HIP_TRY(hipGetLastError());
        return OT_OK;
    }
    TileWork wk;
    wk.fill = fill;
    wk.spread = (int*)(ws + o_spread);
    wk.counts = (unsigned int*)(ws + o_counts);
    wk.tot = (unsigned long long*)(ws + o_tot);
    wk.starts = (unsigned long long*)(ws + o_starts);
    wk.chunk_start = (int*)(ws + o_cstart);
    wk.rec = (TileRec*)(ws + o_rec);
    wk.slabs = (double*)(ws + o_slabs);
    if (pin.tiles)
        HIP_TRY(hipMemsetAsync(wk.spread, 1, sizeof(int), st));
    else
        hipLaunchKernelGGL(tile_probe_kernel, dim3(1), dim3(1024), OT_PROBE_LDS, st, t, px, py, w, wk.spread, fill);
    direct(wk.spread);
    hipLaunchKernelGGL(tile_count_kernel, dim3(OT_TILE_PIECES), dim3(1024), 0, st, t, px, py, w, wk);
    hipLaunchKernelGGL(tile_cursor_kernel, dim3((unsigned)((t.K + 3) / 4)), dim3(256), 0, st, t, wk, wk.tot);
    hipLaunchKernelGGL(tile_scan_kernel, dim3(1), dim3(1024), 0, st, t, wk, (const unsigned long long*)wk.tot);
    hipLaunchKernelGGL(tile_scatter_kernel, dim3(OT_TILE_PIECES), dim3(1024), 0, st, t, px, py, w, wl, wk);
    hipLaunchKernelGGL(tile_accum_kernel, dim3((unsigned)t.max_chunks), dim3(1024), OT_ACCUM_LDS, st, t, table, wk);
    hipLaunchKernelGGL(tile_reduce_kernel, dim3(OT_TILE_PX / 256, (unsigned)t.K), dim3(256), 0, st, t, wk, hist);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_render_accumulate(int64_t n, const double* px, const double* py, const float* w, const float* wl,
                                    const double extent[4], int32_t Nx, int32_t Ny, double* hist, void* stream) {
    return render_accumulate(n, nullptr, px, py, w, wl, extent, Nx, Ny, hist, stream);
}

extern "C" int ot_render_accumulate_compact(int64_t n, const uint32_t* fill, const double* px, const double* py,
                                            const float* w, const float* wl, const double extent[4], int32_t Nx,
                                            int32_t Ny, double* hist, void* stream) {
    if (!fill) return fail(OT_ERR_INVALID, "ot_render_accumulate_compact: fill counts missing");
    return render_accumulate(n, fill, px, py, w, wl, extent, Nx, Ny, hist, stream);
}

// ---- detector image in one pass (ot_detector_fused.hpp) ------------------------------------------------------
// a small record to device memory through the kernel arguments (no staging copy, nothing for the host to wait for)
template <class T>
__global__ void put_kernel(T v, T* dst) {
    if (threadIdx.x == 0) *dst = v;
}

struct FuseIndexAll {
    FuseIndex v[OT_DET_MAX];
};

// one detector, an image of few tiles: the tile kernel with line buffers (OT_TILE_LINEBUF=0 in the environment: the plain one)
static bool fuse_use_linebuf(int K) {
    const char* v = std::getenv("OT_TILE_LINEBUF");
    return K <= OT_LB_MAXK && !(v && v[0] == '0');
}

static int tile_count(int32_t Nx, int32_t Ny) { return ((Nx + OT_TILE_W - 1) / OT_TILE_W) * ((Ny + OT_TILE_W - 1) / OT_TILE_W); }

// the rays from `first` on as a storage of their own: the tile kernels address their rays with 32 bits from its start
static ot_rays rays_from(const ot_rays& rays, int64_t first) {
    ot_rays part = rays;
    part.p += first;
    part.w += first;
    part.wl += first;
    return part;
}

// Shape of the tile kernel's launch: n_wg persistent workgroups of `piece` rays.  A workgroup hands out chunks of its own
// part of a detector's pool (per_wg chunks); every (workgroup, tile) pair leaves at most one chunk partly filled.
// small_k: two rays per thread and sub-block (images of at most 1024 tiles: 10-bit tile numbers); linebuf: the line-buffer
// kernel, one 1024-thread workgroup per CU.
struct TilePool {
    bool linebuf, small_k;
    unsigned n_wg;
    int64_t piece;
    TilePool(int64_t count, bool linebuf_, bool small_k_, int cus) : linebuf(linebuf_), small_k(small_k_) {
        const int64_t brt = linebuf ? OT_LB_BR * OT_LB_RPT : OT_FUSE_BR * (small_k ? 2 : 1);
        n_wg = (unsigned)std::min<int64_t>((linebuf ? 1 : OT_FUSE_WG_PER_CU) * (int64_t)cus, (count + brt - 1) / brt);
        piece = ((count + n_wg - 1) / n_wg + brt - 1) / brt * brt;
    }
    void size(FuseOne& f) const {  // (f.K set)
        f.per_wg = (uint32_t)((piece + OT_FUSE_CH - 1) / OT_FUSE_CH + f.K + 2);
        f.cap = (uint32_t)std::min<int64_t>((int64_t)f.per_wg * n_wg, 0xffffffffll / OT_FUSE_CH - 1);  // record numbers: 32 bits
    }
};

// Scratch of the second tile pass for n detectors of at most K tiles and cap chunks each: chunks grouped by tile (FuseIndex),
// and one slab per accumulation workgroup -- a tile with c chunks takes ceil(c / OT_FUSE_CPW) of them
struct IndexLayout {
    size_t o_tn, o_ts, o_list, o_ws, o_slabs;
    int K;
    uint32_t cap;
    unsigned n_slabs;
    IndexLayout() = default;
    IndexLayout(Carver& carve, int K_, uint32_t cap_, int n) : K(K_), cap(cap_) {
        o_tn = carve(sizeof(unsigned int) * K * (size_t)n);
        o_ts = carve(sizeof(unsigned int) * (K + 1) * (size_t)n);
        o_list = carve(sizeof(unsigned int) * (size_t)cap * n);
        o_ws = carve(sizeof(unsigned int) * (K + 1) * (size_t)n);
        n_slabs = (unsigned)((cap + OT_FUSE_CPW - 1) / OT_FUSE_CPW) + (unsigned)K;
        o_slabs = carve(sizeof(double) * OT_TILE_PX * 4 * (size_t)n_slabs * n);
    }
    FuseIndex at(char* ws, int k) const {
        FuseIndex ix{};
        ix.tile_n = (unsigned int*)(ws + o_tn) + (size_t)K * k;
        ix.tstart = (unsigned int*)(ws + o_ts) + (size_t)(K + 1) * k;
        ix.wstart = (unsigned int*)(ws + o_ws) + (size_t)(K + 1) * k;
        ix.n_slabs = n_slabs;
        ix.list = (unsigned int*)(ws + o_list) + (size_t)cap * k;
        ix.slabs = (double*)(ws + o_slabs) + (size_t)OT_TILE_PX * 4 * n_slabs * k;
        return ix;
    }
};

// A detector's chunk pool of the first tile pass: chunk_tile, chunk_fill and the records of rec_size bytes (f.cap set)
struct PoolLayout {
    size_t o_ctile, o_cfill, o_rec;
    PoolLayout() = default;
    PoolLayout(Carver& carve, uint32_t cap, size_t rec_size) {
        o_ctile = carve(sizeof(uint32_t) * cap);
        o_cfill = carve(sizeof(uint32_t) * cap);
        o_rec = carve(rec_size * (size_t)cap * OT_FUSE_CH);
    }
    void point(FuseOne& f, char* ws) const {
        f.chunk_tile = (uint32_t*)(ws + o_ctile);
        f.chunk_fill = (uint32_t*)(ws + o_cfill);
        f.rec = (TileRec*)(ws + o_rec);
    }
};

// what every fused launch knows of a detector: the surface, its crop and projection, and the tile grid of its image
static void fuse_fill_detector(FuseOne& f, const LeafSurface& ls, const ot_surface* detector, const double* crop4, int32_t projection,
                               int32_t tx, int32_t K, bool tiles_ok) {
    std::memset(&f, 0, sizeof(f));
    f.det = ls.d;
    f.Rcurv = detector->R;
    if (crop4) f.crop = {crop4[0], crop4[1], crop4[2], crop4[3], 1};
    f.projection = projection;
    f.tx = tx;
    f.K = K;
    f.tiles_ok = tiles_ok;
}

// The first tile pass over `count` rays from `first` on for n_det detectors with KT tiles in all.  One detector: line
// buffers, else two rays per thread, else one (tp); several: the smallest NDET that fits (unused entries of the unrolled
// detector loop cost registers), and PAIR where the storage has two sections (a tail storage): every hit from the prefetched
// pair, no section search.  SPECX (the automatic extent) has one detector.
template <bool SPECX>
static void launch_tile_pass(const ot_rays& rays, int64_t first, int64_t count, const FuseOne* dd, int n_det, int KT, const TilePool& tp,
                             hipStream_t st) {
    const ot_rays part = rays_from(rays, first);
#define OT_LAUNCH_TILES(ND, RPT, PAIR)                                                                                              \
    hipLaunchKernelGGL((fuse_tiles_kernel<ND, RPT, SPECX, PAIR>), dim3(tp.n_wg), dim3(OT_FUSE_BR), fuse_tiles_lds(KT), st, part, \
                       (uint32_t)count, dd, n_det, KT, (uint32_t)tp.piece)
    if (tp.linebuf) {
        hipLaunchKernelGGL(fuse_tiles_lb_kernel<SPECX>, dim3(tp.n_wg), dim3(OT_LB_BR), fuse_lb_lds(KT), st, part, (uint32_t)count, dd, KT,
                           (uint32_t)tp.piece);
    } else if (n_det == 1) {
        if (tp.small_k) OT_LAUNCH_TILES(1, 2, false); else OT_LAUNCH_TILES(1, 1, false);
    } else if constexpr (!SPECX) {
        if (rays.nt == 2) {
            if (n_det <= 2) OT_LAUNCH_TILES(2, 1, true); else if (n_det <= 4) OT_LAUNCH_TILES(4, 1, true); else OT_LAUNCH_TILES(8, 1, true);
        } else {
            if (n_det <= 2) OT_LAUNCH_TILES(2, 1, false); else if (n_det <= 4) OT_LAUNCH_TILES(4, 1, false); else OT_LAUNCH_TILES(8, 1, false);
        }
    }
#undef OT_LAUNCH_TILES
}

extern "C" int ot_detector_images(const ot_rays* rays, int64_t first, int64_t count, const ot_detector_image_req* reqs,
                                  int32_t n_reqs, void* stream) {
    if (!rays || !reqs || n_reqs < 1) return fail(OT_ERR_INVALID, "ot_detector_images: null argument");
    if (n_reqs > OT_DET_MAX) return fail(OT_ERR_INVALID, "ot_detector_images: at most 8 detectors per call");
    if (!rays->p || !rays->w || !rays->wl) return fail(OT_ERR_INVALID, "ot_detector_images: ray storage has null buffers");
    if (first < 0 || count < 0 || first + count > rays->N) return fail(OT_ERR_INVALID, "ot_detector_images: range outside the storage");
    for (int k = 0; k < n_reqs; k++) {
        const ot_detector_image_req& q = reqs[k];
        if (!q.detector || !q.hist || !q.ill_count || q.Nx < 1 || q.Ny < 1) return fail(OT_ERR_INVALID, "ot_detector_images: bad request");
        if (!(q.extent[1] > q.extent[0]) || !(q.extent[3] > q.extent[2])) return fail(OT_ERR_INVALID, "ot_detector_images: empty image extent");
        if ((int64_t)q.Nx * q.Ny > (1ll << 27)) return fail(OT_ERR_INVALID, "ot_detector_images: image too large");
        if (!std::isfinite(q.weight_scale)) return fail(OT_ERR_INVALID, "ot_detector_images: weight_scale is not finite");
        if (q.projection < OT_PROJ_NONE || q.projection > OT_PROJ_STEREOGRAPHIC) return fail(OT_ERR_INVALID, "unknown projection");
    }
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    std::vector<LeafSurface> ls(n_reqs);
    for (int k = 0; k < n_reqs; k++)
        if (int rc = ls[k].init(reqs[k].detector, st)) return rc;
    if (count == 0) return OT_OK;
    // Detectors that need the numeric hit search (aspheric, tilted, spline surfaces) or a sphere projection with
    // transcendentals take the two-step chain: with the Illinois loop and the projection polynomials inside, the fused
    // kernels need every vector register there is and lose to hit search + binning (C3, 5e7 rays: 3.1 against 2.1 ms).
    for (int k = 0; k < n_reqs; k++) {
        const ot_detector_image_req& q = reqs[k];
        if (fused_ok(*q.detector, q.projection)) continue;
        // this request alone through ot_detector_hits + ot_render_accumulate, the others through the fused kernels
        const size_t o_hw = align_up(sizeof(double) * 2 * (size_t)count);
        const ot_scratch::Lease hits = workspace(OT_WS_FUSED_HITS, o_hw + sizeof(float) * (size_t)count, st);
        char* tmp = hits.p();
        if (!tmp) return fail(OT_ERR_HIP, "ot_detector_images: no memory for the hit list");
        ot_detector_req dq;
        dq.detector = q.detector;
        dq.projection = q.projection;
        dq.xy_only = 1;
        dq.crop4 = q.crop4;
        dq.ph = (double*)tmp;
        dq.hw = (float*)(tmp + o_hw);
        dq.extent4 = nullptr;
        dq.wl_out = nullptr;
        dq.fill = nullptr;
        dq.ill_count = q.ill_count;
        int rc = ot_detector_hits_multi(rays, first, count, &dq, 1, stream);
        if (!rc) rc = render_accumulate(count, nullptr, dq.ph, dq.ph + count, dq.hw, rays->wl + first, q.extent, q.Nx, q.Ny, q.hist, stream,
                                        q.weight_scale);
        if (rc) return rc;
        std::vector<ot_detector_image_req> rest;
        for (int j = 0; j < n_reqs; j++)
            if (j != k) rest.push_back(reqs[j]);
        return rest.empty() ? OT_OK : ot_detector_images(rays, first, count, rest.data(), (int32_t)rest.size(), stream);
    }
    // from here on every request has a closed-form hit and no sphere projection
    const double* table = nullptr;
    if (int rc = detector_setup(&table)) return rc;
    const int cus = cu_count();
    // a tile-kernel workgroup keeps 20 B of LDS per (detector, tile): more tiles than fit -> two calls
    int KT_all = 0;
    for (int k = 0; k < n_reqs; k++) KT_all += tile_count(reqs[k].Nx, reqs[k].Ny);
    if (n_reqs > 1 && KT_all > OT_FUSE_LDS_ENTRIES) {
        const int h = n_reqs / 2;
        if (int rc = ot_detector_images(rays, first, count, reqs, h, stream)) return rc;
        return ot_detector_images(rays, first, count, reqs + h, n_reqs - h, stream);
    }
    const RenderPath pin = render_path();
    // (the threshold counts the hits a call may bin: rays x detectors -- the last, short chunk of an iterative render with six
    // positions then stays on the tile path instead of 6e6 global atomic quadruples)
    const bool want_tiles = !pin.direct && (pin.tiles || count * (int64_t)n_reqs >= OT_TILE_MIN_HITS);
    if (count >= (1ll << 31)) return fail(OT_ERR_UNSUPPORTED, "ot_detector_images: at most 2^31 - 1 rays per call");
    bool small_k = n_reqs == 1;
    for (int k = 0; k < n_reqs; k++) small_k = small_k && tile_count(reqs[k].Nx, reqs[k].Ny) <= 1024;
    const bool linebuf = n_reqs == 1 && fuse_use_linebuf(tile_count(reqs[0].Nx, reqs[0].Ny));
    const TilePool tp(count, linebuf, small_k, cus);

    std::vector<FuseOne> host(n_reqs);
    int KT = 0, Kmax = 1;
    uint32_t capmax = 1;
    Carver carve{0};
    const size_t o_dets = carve(sizeof(FuseOne) * n_reqs);
    const size_t o_flags = carve(sizeof(int) * 4 * n_reqs);  // per detector: spread, -, overflow, pad
    const size_t o_pcnt = carve(sizeof(int) * 2 * n_reqs);   // probe: distinct pixels, workgroups done
    const size_t o_pset = carve(sizeof(int) * OT_TILE_PROBE_SET * (size_t)n_reqs);  // probe: pixel sets
    PoolLayout pools[OT_DET_MAX];
    for (int k = 0; k < n_reqs; k++) {
        FuseOne& f = host[k];
        const ot_detector_image_req& q = reqs[k];
        const int K = tile_count(q.Nx, q.Ny);
        fuse_fill_detector(f, ls[k], q.detector, q.crop4, q.projection, (q.Nx + OT_TILE_W - 1) / OT_TILE_W, K,
                           want_tiles && K <= OT_TILE_MAX && K <= OT_FUSE_LDS_ENTRIES);
        f.a = render_args(q.extent, q.Nx, q.Ny, q.weight_scale);
        f.ill = (unsigned long long*)q.ill_count;
        f.hist = q.hist;
        f.koff = KT;
        if (f.tiles_ok) {
            KT += f.K;
            tp.size(f);
            pools[k] = PoolLayout(carve, f.cap, sizeof(TileRec));
            Kmax = std::max(Kmax, f.K);
            capmax = std::max(capmax, f.cap);
        }
    }
    // second pass (chunks grouped by tile, accumulation, reduction): every detector its own index and slabs, so that one launch
    // per step serves them all (six positions of an iterative render: 400 accumulation workgroups each, 1.6 rounds over 256 CUs
    // when launched one after the other)
    const size_t o_ixs = carve(sizeof(FuseIndexAll));
    const IndexLayout idx(carve, Kmax, capmax, KT ? n_reqs : 0);
    ot_scratch::Lease lease = workspace(OT_WS_FUSED, carve.off, st);
    char* ws = lease.p();
    if (!ws) {
        if (!KT) return fail(OT_ERR_HIP, "ot_detector_images: no scratch memory");
        // no room for the records: bin directly (needs the flags and the detector table only)
        KT = 0;
        for (auto& f : host) f.tiles_ok = 0;
        lease = workspace(OT_WS_FUSED, o_flags + sizeof(int) * 4 * n_reqs + 256, st);
        ws = lease.p();
        if (!ws) return fail(OT_ERR_HIP, "ot_detector_images: no scratch memory");
    }
    int* flags = (int*)(ws + o_flags);
    for (int k = 0; k < n_reqs; k++) {
        FuseOne& f = host[k];
        f.spread = flags + 4 * k;
        f.overflow = flags + 4 * k + 2;
        if (f.tiles_ok) pools[k].point(f, ws);
    }
    hipError_t err = hipMemsetAsync(flags, 0, sizeof(int) * 4 * n_reqs, st);
    if (err == hipSuccess) err = hipMemcpyAsync(ws + o_dets, host.data(), sizeof(FuseOne) * n_reqs, hipMemcpyHostToDevice, st);
    const FuseOne* dd = (const FuseOne*)(ws + o_dets);
    if (err == hipSuccess) {
        if (KT) {
            if (pin.tiles) {  // spread = 1 for every detector with a pool
                std::vector<int> hf(4 * n_reqs, 0);
                for (int k = 0; k < n_reqs; k++) hf[4 * k] = host[k].tiles_ok;
                err = hipMemcpyAsync(flags, hf.data(), sizeof(int) * 4 * n_reqs, hipMemcpyHostToDevice, st);
                (void)hipStreamSynchronize(st);  // hf goes out of scope
            } else {
                int* pcnt = (int*)(ws + o_pcnt);
                int* pset = (int*)(ws + o_pset);
                err = hipMemsetAsync(pcnt, 0, sizeof(int) * 2 * n_reqs, st);
                if (err == hipSuccess) err = hipMemsetAsync(pset, 0xff, sizeof(int) * OT_TILE_PROBE_SET * (size_t)n_reqs, st);
                const dim3 pg(n_reqs, OT_TILE_PROBE / OT_FUSE_PROBE_WG);
                hipLaunchKernelGGL(fuse_probe_kernel, pg, dim3(OT_FUSE_PROBE_WG), 0, st, *rays, first, count, dd, pset, pcnt);
            }
        }
        // the direct kernel (it returns at once for a detector whose verdict is "tiles"), and the tile pass where a detector has a pool
        const dim3 dg((unsigned)std::min<int64_t>(cus, (count + 1023) / 1024));
#define OT_LAUNCH_DIRECT(ND) hipLaunchKernelGGL((fuse_direct_kernel<ND>), dg, dim3(1024), 0, st, *rays, first, count, dd, n_reqs, table)
        if (n_reqs == 1) OT_LAUNCH_DIRECT(1);
        else if (n_reqs <= 2) OT_LAUNCH_DIRECT(2);
        else if (n_reqs <= 4) OT_LAUNCH_DIRECT(4);
        else OT_LAUNCH_DIRECT(8);
#undef OT_LAUNCH_DIRECT
        if (KT) launch_tile_pass<false>(*rays, first, count, dd, n_reqs, KT, tp, st);
        err = hipGetLastError();
        // tile path, all detectors per launch: chunks grouped by tile, LDS accumulation, slabs summed into the images
        if (err == hipSuccess && KT) {
            FuseIndexAll ixs;
            std::memset(&ixs, 0, sizeof(ixs));
            for (int k = 0; k < n_reqs; k++) ixs.v[k] = idx.at(ws, k);
            err = hipMemsetAsync(ws + idx.o_tn, 0, sizeof(unsigned int) * Kmax * (size_t)n_reqs, st);
            if (err == hipSuccess) {
                hipLaunchKernelGGL(put_kernel<FuseIndexAll>, dim3(1), dim3(64), 0, st, ixs, (FuseIndexAll*)(ws + o_ixs));
                const FuseIndex* dix = (const FuseIndex*)(ws + o_ixs);
                const unsigned gc = (capmax + 1024 * OT_FUSE_IDX_PER - 1) / (1024 * OT_FUSE_IDX_PER);
                const unsigned nd = (unsigned)n_reqs;
                hipLaunchKernelGGL(fuse_chunk_hist_multi_kernel, dim3(gc, 1, nd), dim3(1024), 0, st, dd, dix);
                hipLaunchKernelGGL(fuse_chunk_scan_multi_kernel, dim3(1, 1, nd), dim3(1024), 0, st, dd, dix);
                hipLaunchKernelGGL(fuse_chunk_place_multi_kernel, dim3(gc, 1, nd), dim3(1024), 0, st, dd, dix);
                hipLaunchKernelGGL(fuse_accum_multi_kernel, dim3(std::min<unsigned>(idx.n_slabs, (unsigned)cus), 1, nd), dim3(1024), OT_ACCUM_LDS, st,
                                   dd, dix, table);
                hipLaunchKernelGGL(fuse_reduce_multi_kernel, dim3(OT_TILE_PX / 256, (unsigned)Kmax, nd), dim3(256), 0, st, dd, dix);
                err = hipGetLastError();
            }
        }
    }
    HIP_TRY(err);
    return OT_OK;
}

// ---- detector image with an automatic extent in one pass (ot_detector_fused.hpp, last section) ---------------------
// Scratch layout of OT_WS_AUTO: the head (detector record, flags, extent slots) is shared by the sample pass and the image.
struct AutoHead {
    size_t o_dets, o_flags, o_slots, end;
    AutoHead() {
        o_dets = 0;
        o_flags = align_up(sizeof(FuseOne));
        o_slots = o_flags + 256;
        end = o_slots + align_up(sizeof(unsigned long long) * 4 * OT_EXT_SLOTS);
    }
};

struct ot_auto_image {
    FuseOne f;  // host copy; the image grid (a, hist) is filled in by finish
    ot_scratch::Lease lease;  // the records: leased until finish / cancel (neither reused nor trimmed in between)
    char* ws;
    IndexLayout idx;
    hipStream_t st;
};

static int auto_detector(const char* who, const ot_rays* rays, int64_t first, int64_t count, const ot_surface* detector,
                         int32_t projection) {
    if (!rays || !detector) return fail(OT_ERR_INVALID, std::string(who) + ": null argument");
    if (!rays->p || !rays->w || !rays->wl) return fail(OT_ERR_INVALID, std::string(who) + ": ray storage has null buffers");
    if (first < 0 || count < 1 || first + count > rays->N) return fail(OT_ERR_INVALID, std::string(who) + ": range outside the storage");
    if (count >= (1ll << 31)) return fail(OT_ERR_UNSUPPORTED, std::string(who) + ": at most 2^31 - 1 rays per call");
    if (!fused_ok(*detector, projection))
        return fail(OT_ERR_UNSUPPORTED, std::string(who) + ": detectors with a numeric hit search or a sphere projection take ot_detector_hits_multi");
    return OT_OK;
}

extern "C" int ot_detector_extent_sample(const ot_rays* rays, int64_t first, int64_t count, const ot_surface* detector,
                                         int32_t projection, int32_t stride, double* extent4, void* stream) {
    if (int rc = auto_detector("ot_detector_extent_sample", rays, first, count, detector, projection)) return rc;
    if (!extent4 || stride < 1) return fail(OT_ERR_INVALID, "ot_detector_extent_sample: bad argument");
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    LeafSurface ls;
    if (int rc = ls.init(detector, st)) return rc;
    const AutoHead h;
    const ot_scratch::Lease lease = workspace(OT_WS_AUTO, h.end, st);
    char* ws = lease.p();
    if (!ws) return fail(OT_ERR_HIP, "ot_detector_extent_sample: no scratch memory");
    FuseOne f;
    fuse_fill_detector(f, ls, detector, nullptr, projection, 0, 0, false);
    f.g.ext_slots = (unsigned long long*)(ws + h.o_slots);
    hipLaunchKernelGGL(put_kernel<FuseOne>, dim3(1), dim3(64), 0, st, f, (FuseOne*)(ws + h.o_dets));
    hipLaunchKernelGGL(extent_init_kernel, dim3(1), dim3(4 * OT_EXT_SLOTS), 0, st, f.g.ext_slots);
    const int64_t waves = (count + 64ll * stride - 1) / (64ll * stride);
    hipLaunchKernelGGL(spec_sample_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, rays_from(*rays, first), (uint32_t)count,
                       (const FuseOne*)(ws + h.o_dets), (uint32_t)stride);
    hipLaunchKernelGGL(spec_result_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)f.g.ext_slots,
                       (const unsigned int*)nullptr, 0u, extent4);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));  // the caller reads extent4 next (and the detector's tables may go)
    return OT_OK;
}

extern "C" int ot_detector_image_auto_begin(const ot_rays* rays, int64_t first, int64_t count, const ot_surface* detector,
                                            int32_t projection, const double origin[2], const double tile[2],
                                            const int32_t tiles[2], double* result6, ot_auto_image** out, void* stream) {
    if (out) *out = nullptr;
    if (int rc = auto_detector("ot_detector_image_auto_begin", rays, first, count, detector, projection)) return rc;
    if (!origin || !tile || !tiles || !result6 || !out) return fail(OT_ERR_INVALID, "ot_detector_image_auto_begin: null argument");
    if (!(tile[0] > 0.0) || !(tile[1] > 0.0) || tiles[0] < 1 || tiles[1] < 1 || !std::isfinite(origin[0]) || !std::isfinite(origin[1]))
        return fail(OT_ERR_INVALID, "ot_detector_image_auto_begin: bad tile grid");
    const int64_t K = (int64_t)tiles[0] * tiles[1];
    if (K > OT_TILE_MAX || K > OT_FUSE_LDS_ENTRIES) return fail(OT_ERR_UNSUPPORTED, "ot_detector_image_auto_begin: more than 2048 tiles");
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    LeafSurface ls;
    if (int rc = ls.init(detector, st)) return rc;
    const bool small_k = K <= 1024, linebuf = fuse_use_linebuf((int)K);  // as in ot_detector_images
    const TilePool tp(count, linebuf, small_k, cu_count());

    std::unique_ptr<ot_auto_image> im(new ot_auto_image);
    FuseOne& f = im->f;
    fuse_fill_detector(f, ls, detector, nullptr, projection, tiles[0], (int32_t)K, true);
    tp.size(f);
    f.g.X0 = origin[0];
    f.g.Y0 = origin[1];
    f.g.tw = tile[0];
    f.g.th = tile[1];
    f.g.itw = 1.0 / tile[0];
    f.g.ith = 1.0 / tile[1];
    f.g.tx = tiles[0];
    f.g.ty = tiles[1];
    f.g.esc_cap = (unsigned int)std::max<int64_t>(1ll << 18, count / 64);

    const AutoHead h;
    Carver carve{h.end};
    const PoolLayout pool(carve, f.cap, sizeof(SpecRec));
    const size_t o_esc = carve(sizeof(SpecRec) * (size_t)f.g.esc_cap);
    im->idx = IndexLayout(carve, f.K, f.cap, 1);
    im->lease = workspace(OT_WS_AUTO, carve.off, st);
    char* ws = im->lease.p();
    if (!ws) return fail(OT_ERR_UNSUPPORTED, "ot_detector_image_auto_begin: no memory for the records (take the hit-list path)");
    im->ws = ws;
    im->st = st;
    const double* table = nullptr;
    if (int rc = detector_setup(&table)) return rc;
    int* flags = (int*)(ws + h.o_flags);
    f.spread = flags;
    f.overflow = flags + 2;
    f.g.esc_n = (unsigned int*)(flags + 3);
    f.g.ext_slots = (unsigned long long*)(ws + h.o_slots);
    pool.point(f, ws);
    f.g.esc = (SpecRec*)(ws + o_esc);
    hipLaunchKernelGGL(put_kernel<int4>, dim3(1), dim3(64), 0, st, make_int4(1, 0, 0, 0), (int4*)flags);  // spread = 1: tiles always
    hipLaunchKernelGGL(put_kernel<FuseOne>, dim3(1), dim3(64), 0, st, f, (FuseOne*)(ws + h.o_dets));
    hipLaunchKernelGGL(extent_init_kernel, dim3(1), dim3(4 * OT_EXT_SLOTS), 0, st, f.g.ext_slots);
    launch_tile_pass<true>(*rays, first, count, (const FuseOne*)(ws + h.o_dets), 1, f.K, tp, st);
    hipLaunchKernelGGL(spec_result_kernel, dim3(1), dim3(64), 0, st, (const unsigned long long*)f.g.ext_slots,
                       (const unsigned int*)f.g.esc_n, f.g.esc_cap, result6);
    HIP_TRY(hipGetLastError());
    // the caller needs the extent before it can go on: wait here (also: the detector's tables may go)
    HIP_TRY(hipStreamSynchronize(st));
    *out = im.release();
    return OT_OK;
}

extern "C" void ot_detector_image_auto_cancel(ot_auto_image* im) { delete im; }

extern "C" int ot_detector_image_auto_finish(ot_auto_image* im_raw, const double extent[4], int32_t Nx, int32_t Ny,
                                             double* hist, void* stream) {
    std::unique_ptr<ot_auto_image> im(im_raw);  // freed whatever happens
    if (!im || !extent || !hist || Nx < 1 || Ny < 1) return fail(OT_ERR_INVALID, "ot_detector_image_auto_finish: bad argument");
    if (!(extent[1] > extent[0]) || !(extent[3] > extent[2])) return fail(OT_ERR_INVALID, "ot_detector_image_auto_finish: empty image extent");
    if ((int64_t)Nx * Ny > (1ll << 27)) return fail(OT_ERR_INVALID, "ot_detector_image_auto_finish: image too large");
    hipStream_t st = (hipStream_t)stream;
    if (st != im->st) return fail(OT_ERR_INVALID, "ot_detector_image_auto_finish: not the stream of ot_detector_image_auto_begin");
    // (the scratch block of begin is still ours: the handle holds its lease)
    const double* table = nullptr;
    if (int rc = detector_setup(&table)) return rc;
    FuseOne& f = im->f;
    f.a = render_args(extent, Nx, Ny, 1.0);
    f.hist = hist;
    const FuseIndex ix = im->idx.at(im->ws, 0);
    HIP_TRY(hipMemsetAsync(ix.tile_n, 0, sizeof(unsigned int) * f.K, st));
    const unsigned gc = (f.cap + 1024 * OT_FUSE_IDX_PER - 1) / (1024 * OT_FUSE_IDX_PER);
    hipLaunchKernelGGL(fuse_chunk_hist_kernel, dim3(gc), dim3(1024), 0, st, f, ix);
    hipLaunchKernelGGL(fuse_chunk_scan_kernel, dim3(1), dim3(1024), 0, st, f, ix);
    hipLaunchKernelGGL(fuse_chunk_place_kernel, dim3(gc), dim3(1024), 0, st, f, ix);
    hipLaunchKernelGGL(spec_accum_kernel, dim3(std::min<unsigned>(ix.n_slabs, (unsigned)cu_count())), dim3(1024), OT_ACCUM_LDS, st, f, ix, table);
    hipLaunchKernelGGL(spec_reduce_kernel, dim3(OT_TILE_PX / 256, (unsigned)f.K), dim3(256), 0, st, f, ix);
    hipLaunchKernelGGL(spec_escaped_kernel, dim3(64), dim3(256), 0, st, f, table);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

// ---- spectrum rendering ---------------------------------------------------------------------------------------
static int spectrum_range(int64_t n, const unsigned int* fill, const float* wl, const float* w, double* range2, int64_t* count,
                          void* stream) {
    if (n < 0 || !range2 || !count || (n && (!wl || !w))) return fail(OT_ERR_INVALID, "ot_spectrum_range: bad argument");
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const double init[2] = {INFINITY, -INFINITY};
    HIP_TRY(hipMemcpyAsync(range2, init, sizeof(init), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(count, 0, sizeof(int64_t), st));
    if (n == 0) return OT_OK;
    int64_t blocks = (n + 255) / 256;
    const int64_t cap = (int64_t)cu_count() * 8;
    if (blocks > cap) blocks = cap;
    hipLaunchKernelGGL(spectrum_stats_kernel, dim3((unsigned)blocks), dim3(256), 0, st, n, wl, w, range2,
                       (unsigned long long*)count, fill);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

static int spectrum_histogram(int64_t n, const unsigned int* fill, const float* wl, const float* w, const float* edges,
                              int32_t nbins, double* hist, void* stream) {
    if (n < 0 || !edges || !hist || nbins < 1 || (n && (!wl || !w)))
        return fail(OT_ERR_INVALID, "ot_spectrum_histogram: bad argument");
    if (int rc = require_device()) return rc;
    if (n == 0) return OT_OK;
    hipStream_t st = (hipStream_t)stream;
    // sums (f64) + edges (f32) per workgroup
    const HistShape hs = hist_shape(n, (size_t)nbins * sizeof(double) + ((size_t)nbins + 2) * sizeof(float));
    hipLaunchKernelGGL(spectrum_hist_kernel, hs.grid, hs.block, hs.lds, st, n, wl, w, edges, nbins, hs.lds ? nbins : 0, hist, fill);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

extern "C" int ot_spectrum_range(int64_t n, const float* wl, const float* w, double* range2, int64_t* count, void* stream) {
    return spectrum_range(n, nullptr, wl, w, range2, count, stream);
}
extern "C" int ot_spectrum_histogram(int64_t n, const float* wl, const float* w, const float* edges, int32_t nbins,
                                     double* hist, void* stream) {
    return spectrum_histogram(n, nullptr, wl, w, edges, nbins, hist, stream);
}
extern "C" int ot_spectrum_range_compact(int64_t n, const uint32_t* fill, const float* wl, const float* w, double* range2,
                                         int64_t* count, void* stream) {
    if (!fill) return fail(OT_ERR_INVALID, "ot_spectrum_range_compact: fill counts missing");
    return spectrum_range(n, fill, wl, w, range2, count, stream);
}
extern "C" int ot_spectrum_histogram_compact(int64_t n, const uint32_t* fill, const float* wl, const float* w,
                                             const float* edges, int32_t nbins, double* hist, void* stream) {
    if (!fill) return fail(OT_ERR_INVALID, "ot_spectrum_histogram_compact: fill counts missing");
    return spectrum_histogram(n, fill, wl, w, edges, nbins, hist, stream);
}
