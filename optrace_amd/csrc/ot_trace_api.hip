// C-ABI, trace stage: ray generation, the launches of the trace kernel's three forms (ot_trace_kernel.hpp, instantiated in
// ot_trace_f*.hip / ot_trace_t*.hip / ot_trace_p*.hip), the counter reduction, the index, polarisation and section fills and
// the render-only tail storage.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>

#include "ot_host.hpp"
#include "ot_trace_kernel.hpp"

// sums the slot tables into the caller's int64 counters (ADD) and clears them for the next launch:
// one workgroup per counter, one lane per 4 slots, wave shuffle + LDS reduction
template <bool ACCUM>  // ACCUM: add to the caller's counters; otherwise overwrite them (pinned host buffer: no read over PCIe)
__global__ __launch_bounds__(256) void reduce_counters_kernel(unsigned int* __restrict__ slots, int n_cnt,
                                                              unsigned long long* __restrict__ msgs) {
    __shared__ unsigned long long part[4];
    const int k = blockIdx.x;
    unsigned long long sum = 0;
    for (int sidx = threadIdx.x; sidx < OT_CNT_SLOTS; sidx += blockDim.x) {
        unsigned int v = slots[(size_t)sidx * n_cnt + k];
        if (v) {
            sum += v;
            slots[(size_t)sidx * n_cnt + k] = 0u;
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = part[0] + part[1] + part[2] + part[3];
        if (!ACCUM) {
            msgs[k] = (k == n_cnt - 1) ? (t ? 1ull : 0ull) : t;
        } else if (t) {
            if (k == n_cnt - 1) msgs[k] = 1ull; else msgs[k] += t;
        }
    }
}

// RaySource.create_rays only: writes section 0 (ot_rays_generate)
template <bool POL>
__global__ __launch_bounds__(256) void generate_kernel(ot_rays R, const SourceDev* __restrict__ sources, RangeArgs rg,
                                                       uint64_t seed) {
    const int64_t ray = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (ray >= R.N) return;
    NewRay nr;
    if (!generate_lane(rg, sources, ray, seed, !POL, nr)) return;
    const int64_t N = R.N, nt = R.nt;
    R.p[ray] = nr.p.x;
    R.p[ray + N * nt] = nr.p.y;
    R.p[ray + N * 2 * nt] = nr.p.z;
    R.s[ray] = nr.s.x;
    R.s[ray + N] = nr.s.y;
    R.s[ray + 2 * N] = nr.s.z;
    R.w[ray] = nr.w;
    R.wl[ray] = nr.wl;
    if (POL) {
        R.pol[ray] = (float)nr.polx;
        R.pol[ray + N * nt] = (float)nr.poly;
        R.pol[ray + N * 2 * nt] = (float)nr.polz;
    }
}

static int check_rays(const ot_rays* r, bool need_pol) {
    if (!r || r->N < 0 || r->nt < 1) return fail(OT_ERR_INVALID, "bad ray storage");
    if (!r->p || !r->s || !r->w || !r->n || !r->wl) return fail(OT_ERR_INVALID, "ray storage: null buffer");
    if (need_pol && !r->pol) return fail(OT_ERR_INVALID, "ray storage: pol buffer missing although polarisation is on");
    return OT_OK;
}

// the storage of a scene's trace has one section per step and one before the first (`who`: the entry point, for the message)
static int check_sections(const char* who, const ot_scene* sc, const ot_rays* rays) {
    if (rays->nt != sc->h.nt)
        return fail(OT_ERR_INVALID, std::string(who) + ": ray storage has " + std::to_string(rays->nt) +
                                        " sections, the scene needs " + std::to_string(sc->h.nt));
    return OT_OK;
}

extern "C" int ot_rays_generate(const ot_sources* src, const ot_source_range* ranges, int32_t n_ranges, uint64_t seed,
                                int32_t no_pol, const ot_rays* rays, void* stream) {
    if (!src) return fail(OT_ERR_INVALID, "ot_rays_generate: null sources");
    if (int rc = check_rays(rays, !no_pol)) return rc;
    const RangeArgs* rgp = nullptr;
    if (int rc = make_ranges(ranges, n_ranges, src, rays->N, &rgp)) return rc;
    const RangeArgs& rg = *rgp;
    hipStream_t st = (hipStream_t)stream;
    if (rays->N > 0) {
        if (no_pol)
            hipLaunchKernelGGL(generate_kernel<false>, grid_for(rays->N), dim3(256), 0, st, *rays, src->d, rg, seed);
        else
            hipLaunchKernelGGL(generate_kernel<true>, grid_for(rays->N), dim3(256), 0, st, *rays, src->d, rg, seed);
    }
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

// Which kernel variant traces a scene, and its dynamic LDS: spectrum handling x feature set (polarisation and on-device
// generation follow from the scene and the entry point).  ot_rays_fill_pol repeats a trace with the variant chosen here.
struct TraceVariant {
    int feat, spec;
    size_t lds;
    const char* error;
};
static TraceVariant trace_variant(const ot_scene* sc, const ot_sources* src, const double* hurb_normals) {
    const int n_cnt = OT_N_INFOS * sc->h.nt + 1;
    const bool tab = sc->needs_tables || hurb_normals != nullptr;
    TraceVariant v = {OT_FEAT(sc->hit_level, sc->needs_full), 0, 0, nullptr};
    // discrete-spectrum kernels: generated rays only, and no image source (their variant of the generator has none)
    bool lines = src != nullptr && sc->h.n_lines > 0 && hurb_normals == nullptr && !src->has_image;
    // dynamic LDS: the counter table, and with discrete spectra the per-line tables (3 rows per step).  Very long
    // stacks do not fit the 64 KB a kernel gets without asking: the formula kernels (SPEC 0 / 1) trace those.
    const size_t lds_cnt = sizeof(unsigned int) * (size_t)n_cnt + 8;
    const size_t lds_lines = sizeof(double) * (size_t)(3 * sc->h.n_steps + 2) * OT_MAX_LINES;
    // spline surfaces: a 5 x 5 coefficient patch per lane (ot_spline.hpp::PatchCache)
    const size_t lds_patch = (sc->hit_level == OT_HIT_SPLINE) ? 256 * 25 * sizeof(double) + 16 : 0;
    if (lds_cnt + lds_patch > 65000) {
        v.error = lds_patch ? "ot_trace: more than ~650 tracing surfaces in a scene with spline surfaces"
                            : "ot_trace: more than ~3000 tracing surfaces in one scene";
        return v;
    }
    if (lines && lds_cnt + lds_lines + lds_patch > 65000) lines = false;
    v.lds = ((lds_cnt + (lines ? lds_lines : 0) + 7) / 8) * 8 + lds_patch;
    v.spec = lines ? 2 : (tab ? 1 : 0);
    return v;
}

// ---- one launch path for the three forms ----------------------------------------------------------------------------------
typedef void (*TraceLauncher)(const TraceLaunch&);
#define OT_FORM_ROW(FORM)                                                                                              \
    {launch_trace_unit<FORM, 0>, launch_trace_unit<FORM, 1>, launch_trace_unit<FORM, 2>, launch_trace_unit<FORM, 3>,    \
     launch_trace_unit<FORM, 4>, launch_trace_unit<FORM, 5>}
static const TraceLauncher k_trace_launchers[OT_N_FORMS][OT_N_FEATS] = {OT_FORM_ROW(OT_FORM_STORE), OT_FORM_ROW(OT_FORM_TAIL),
                                                                        OT_FORM_ROW(OT_FORM_POL)};

// What every launch of a trace has in common; the caller adds the storage (part or tail).  src / rg: null for rays handed in.
static TraceLaunch make_launch(const ot_scene* sc, const ot_sources* src, const RangeArgs* rg, const TraceVariant& v,
                               uint64_t seed, hipStream_t st) {
    static const RangeArgs no_ranges = {};
    TraceLaunch L = {};
    L.lds = v.lds;
    L.st = st;
    L.sc = sc->d;
    L.sd = src ? src->d : nullptr;
    L.rg = rg ? rg : &no_ranges;
    L.seed = seed;
    L.slots = sc->cnt_slots;
    L.pol = !sc->h.no_pol;
    L.gen = src != nullptr;
    L.spec = v.spec;
    L.sec_first = 0;
    L.sec_end = sc->h.nt;
    return L;
}

// launches the rays [base, base + n) of the bundle (one piece of for_ray_chunks)
static void launch_chunk(int form, int feat, TraceLaunch& L, int64_t base, uint32_t n) {
    L.base = base;
    L.count = n;
    L.grid = grid_for(n);
    k_trace_launchers[form][feat](L);
}

static TailOut tail_out(const ot_rays* tail, uint32_t* fill) {
    TailOut T;
    T.p = tail->p;
    T.w = tail->w;
    T.wl = tail->wl;
    T.fill = fill;
    T.cap = tail->N;
    return T;
}

static size_t msgs_bytes(const ot_scene* sc) { return sizeof(unsigned long long) * (size_t)(OT_N_INFOS * sc->h.nt + 1); }

// the scene's pinned host buffer for the counters of one launch (created on first use)
static int pinned_counters(ot_scene* sc) {
    if (sc->pin_msgs) return OT_OK;
    HIP_TRY(hipHostMalloc((void**)&sc->pin_msgs, msgs_bytes(sc), hipHostMallocMapped | hipHostMallocCoherent));
    std::memset(sc->pin_msgs, 0, msgs_bytes(sc));
    return OT_OK;
}

// The launches of one trace of n_rays rays -- each(base, n) launches a chunk --, timed if the scene asks for it, and the
// counter reduction.  msgs: device counters the trace ADDS to, or nullptr: the counters of this trace alone go to the
// scene's pinned host buffer.
template <class F>
static int trace_chunks(ot_scene* sc, int64_t n_rays, int64_t* msgs, hipStream_t st, F&& each) {
    const int n_cnt = OT_N_INFOS * sc->h.nt + 1;
    unsigned long long* m = (unsigned long long*)msgs;
    if (!msgs) HIP_TRY(hipHostGetDevicePointer((void**)&m, sc->pin_msgs, 0));
    if (sc->timing) HIP_TRY(hipEventRecord(sc->ev0, st));
    for_ray_chunks(0, n_rays, each);
    HIP_TRY(hipGetLastError());
    if (sc->timing) {
        HIP_TRY(hipEventRecord(sc->ev1, st));
        sc->ev_valid = true;
    }
    if (msgs)
        hipLaunchKernelGGL(reduce_counters_kernel<true>, dim3(n_cnt), dim3(256), 0, st, sc->cnt_slots, n_cnt, m);
    else
        hipLaunchKernelGGL(reduce_counters_kernel<false>, dim3(n_cnt), dim3(256), 0, st, sc->cnt_slots, n_cnt, m);
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

// A stored trace: rays handed in (src and rg null) or generated on the device.
static int launch_trace(const ot_scene* sc_c, const ot_sources* src, const RangeArgs* rg, const ot_rays* rays,
                        const double* hurb_normals, uint64_t seed, int64_t* msgs, void* stream) {
    ot_scene* sc = const_cast<ot_scene*>(sc_c);
    if (!sc) return fail(OT_ERR_INVALID, "ot_trace: null argument");
    if (int rc = check_rays(rays, !sc->h.no_pol)) return rc;
    if (int rc = check_sections("ot_trace", sc, rays)) return rc;
    if (!msgs)
        if (int rc = pinned_counters(sc)) return rc;
    if (rays->N == 0) {
        if (!msgs) std::memset(sc->pin_msgs, 0, msgs_bytes(sc));
        return OT_OK;
    }
    const TraceVariant v = trace_variant(sc, src, hurb_normals);
    if (v.error) return fail(OT_ERR_UNSUPPORTED, v.error);
    sc->index_spec = v.spec;  // what ot_rays_fill_index has to repeat
    TraceLaunch L = make_launch(sc, src, rg, v, seed, (hipStream_t)stream);
    L.hurb_normals = hurb_normals;
    // OT_DEFER_SECTIONS: position and weight of the last two sections only, which is all a detector behind the stack and
    // ot_tail_append read; ot_rays_fill_sections writes the rest.  Rays handed in cannot be repeated: every section.
    if ((sc->deferred & OT_DEFER_SECTIONS) && src) L.sec_first = std::max(0, sc->h.nt - 2);
    return trace_chunks(sc, rays->N, msgs, L.st, [&](int64_t base, uint32_t n) {
        L.part = *rays;
        L.part.p += base; L.part.s += base; L.part.w += base; L.part.n += base; L.part.wl += base;
        if (L.part.pol) L.part.pol += base;
        // deferred planes: a null base, the kernel skips the plane (ot_trace.hpp::store_section).  Rays handed in
        // cannot be repeated and carry their polarisation in section 0 of the plane: ot_trace always stores it.
        if (sc->deferred & OT_DEFER_INDEX) L.part.n = nullptr;
        if ((sc->deferred & OT_DEFER_POL) && src) L.part.pol = nullptr;
        launch_chunk(OT_FORM_STORE, v.feat, L, base, n);
    });
}

extern "C" int ot_trace(const ot_scene* scene, const ot_rays* rays, const double* hurb_normals, uint64_t seed,
                        int64_t* msgs, void* stream) {
    if (!msgs) return fail(OT_ERR_INVALID, "ot_trace: null argument");
    return launch_trace(scene, nullptr, nullptr, rays, hurb_normals, seed, msgs, stream);
}

extern "C" int ot_generate_and_trace(const ot_scene* scene, const ot_sources* src, const ot_source_range* ranges,
                                     int32_t n_ranges, uint64_t seed, const ot_rays* rays, int64_t* msgs, void* stream) {
    if (!src || !rays || !msgs) return fail(OT_ERR_INVALID, "ot_generate_and_trace: null argument");
    const RangeArgs* rg = nullptr;
    if (int rc = make_ranges(ranges, n_ranges, src, rays->N, &rg)) return rc;
    return launch_trace(scene, src, rg, rays, nullptr, seed, msgs, stream);
}

// The whole of Raytracer.trace in one synchronous call: launch, wait, counters of this launch in host memory.
// The counter reduction writes into a pinned host buffer of the scene, so the wait for the stream is the only
// synchronisation and nothing is copied back.
extern "C" int ot_generate_and_trace_host(const ot_scene* scene, const ot_sources* src, const ot_source_range* ranges,
                                          int32_t n_ranges, uint64_t seed, const ot_rays* rays, int64_t* msgs_host,
                                          void* stream) {
    if (!scene || !src || !rays || !msgs_host) return fail(OT_ERR_INVALID, "ot_generate_and_trace_host: null argument");
    const RangeArgs* rg = nullptr;
    if (int rc = make_ranges(ranges, n_ranges, src, rays->N, &rg)) return rc;
    if (int rc = launch_trace(scene, src, rg, rays, nullptr, seed, nullptr, stream)) return rc;
    HIP_TRY(hipStreamSynchronize((hipStream_t)stream));
    std::memcpy(msgs_host, scene->pin_msgs, msgs_bytes(scene));
    return OT_OK;
}

// The index plane n[section, ray] of a traced storage, written on its own.  trace_ray sets a ray's index for every lane,
// alive or not, hit or not: section 0 carries the ambient medium, a refracting step (kind <= OT_STEP_IDEAL) the medium behind
// it, every other step the index before it -- a function of (scene, section, wavelength) alone.  This kernel walks the same
// steps with the same device functions the trace kernel of variant SPEC uses (medium_n<TAB>; SPEC 2: the rows of the
// per-line table and ray_line to find a ray's line), so the plane is bit for bit what that trace stores when
// the scene's index store is on.  One ray per lane, 32-bit lane offsets from a wave-uniform plane base that advances by one
// plane per section; streaming stores (the plane is written once and not read here).
template <int SPEC>
__global__ __launch_bounds__(256) void fill_index_kernel(const SceneDev* __restrict__ scp, const float* __restrict__ wlp,
                                                         double* __restrict__ plane, int64_t stride, uint32_t count) {
    constexpr bool TAB = (SPEC == 1);
    const uint32_t local = blockIdx.x * blockDim.x + threadIdx.x;
    if (local >= count) return;
    auto& sc = *as_const(scp);
    const auto steps = as_const(sc.steps);
    const auto media = as_const(sc.media);
    const auto pool = as_const(sc.pool);
    const float wl = wlp[local];
    const double* ltab = sc.line_tab;
    const int lj = ray_line<SPEC>(sc, ltab, wl);
    const double* lrow = ltab + OT_MAX_LINES + lj;  // row 0 of this lane's column (trace_ray)
    double n_cur = (SPEC == 2) ? lrow[(3 * sc.n_steps) * OT_MAX_LINES] : medium_n<TAB>(media[sc.n0], pool, wl);
    __builtin_nontemporal_store(n_cur, &plane[local]);
    for (int i = 0; i < sc.n_steps; i++) {
        auto& st = steps[i];
        if (st.kind <= OT_STEP_IDEAL)
            n_cur = (SPEC == 2) ? lrow[(3 * i + 0) * OT_MAX_LINES] : medium_n<TAB>(media[st.n_next], pool, wl);
        plane += stride;
        __builtin_nontemporal_store(n_cur, &plane[local]);
    }
}

extern "C" int ot_rays_fill_index(const ot_scene* sc, const ot_rays* rays, int64_t first, int64_t count, void* stream) {
    if (!sc || !rays) return fail(OT_ERR_INVALID, "ot_rays_fill_index: null argument");
    if (rays->N < 0 || !rays->n || !rays->wl) return fail(OT_ERR_INVALID, "ot_rays_fill_index: the ray storage needs n and wl");
    if (int rc = check_sections("ot_rays_fill_index", sc, rays)) return rc;
    if (first < 0 || count < 0 || first + count > rays->N) return fail(OT_ERR_INVALID, "ot_rays_fill_index: range outside the storage");
    if (int rc = require_device()) return rc;
    // the variant of the scene's last stored trace; none yet: formulas, as a trace of rays handed in would take
    int spec = sc->index_spec >= 0 ? sc->index_spec : (sc->needs_tables ? 1 : 0);
    if (spec == 2 && sc->h.n_lines < 1) spec = sc->needs_tables ? 1 : 0;
    hipStream_t st = (hipStream_t)stream;
    for_ray_chunks(first, count, [&](int64_t base, uint32_t n) {
        const float* wl = rays->wl + base;
        double* plane = rays->n + base;
        if (spec == 2)
            hipLaunchKernelGGL(fill_index_kernel<2>, grid_for(n), dim3(256), 0, st, sc->d, wl, plane, rays->N, n);
        else if (spec == 1)
            hipLaunchKernelGGL(fill_index_kernel<1>, grid_for(n), dim3(256), 0, st, sc->d, wl, plane, rays->N, n);
        else
            hipLaunchKernelGGL(fill_index_kernel<0>, grid_for(n), dim3(256), 0, st, sc->d, wl, plane, rays->N, n);
    });
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

// The polarisation planes of a storage whose trace left them unwritten (OT_DEFER_POL): the trace once more, storing only them
// (ot_trace_kernel.hpp::trace_pol_kernel).
extern "C" int ot_rays_fill_pol(const ot_scene* sc, const ot_sources* src, const ot_source_range* ranges, int32_t n_ranges,
                                uint64_t seed, const ot_rays* rays, int64_t first, int64_t count, void* stream) {
    if (!sc || !src || !ranges || !rays) return fail(OT_ERR_INVALID, "ot_rays_fill_pol: null argument");
    if (sc->h.no_pol) return fail(OT_ERR_INVALID, "ot_rays_fill_pol: the scene does not track polarisation");
    if (rays->N < 0 || !rays->pol) return fail(OT_ERR_INVALID, "ot_rays_fill_pol: the ray storage needs pol");
    if (int rc = check_sections("ot_rays_fill_pol", sc, rays)) return rc;
    if (first < 0 || count < 0 || first > rays->N || count > rays->N - first)
        return fail(OT_ERR_INVALID, "ot_rays_fill_pol: range outside the storage");
    if (int rc = require_device()) return rc;
    const RangeArgs* rg = nullptr;
    if (int rc = make_ranges(ranges, n_ranges, src, rays->N, &rg)) return rc;
    const TraceVariant v = trace_variant(sc, src, nullptr);
    if (v.error) return fail(OT_ERR_UNSUPPORTED, v.error);
    TraceLaunch L = make_launch(sc, src, rg, v, seed, (hipStream_t)stream);
    L.part.N = rays->N;  // the kernel reads N, nt and pol
    L.part.nt = rays->nt;
    for_ray_chunks(first, count, [&](int64_t base, uint32_t n) {
        L.part.pol = rays->pol + base;
        launch_chunk(OT_FORM_POL, v.feat, L, base, n);
    });
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

// The position and weight planes of the sections a trace left unwritten (OT_DEFER_SECTIONS): the storing kernel of that trace
// once more (trace_variant), writing p and w of the sections [0, nt - 2) -- and, with the same values as before, s and wl.
// The index and polarisation planes are not touched, the counters stay in the workgroups (null slot table), the scene's
// pinned counters and its timing events are left as the trace set them.
extern "C" int ot_rays_fill_sections(const ot_scene* sc, const ot_sources* src, const ot_source_range* ranges, int32_t n_ranges,
                                     uint64_t seed, const ot_rays* rays, int64_t first, int64_t count, void* stream) {
    if (!sc || !src || !ranges || !rays) return fail(OT_ERR_INVALID, "ot_rays_fill_sections: null argument");
    if (rays->N < 0 || !rays->p || !rays->w || !rays->s || !rays->wl)
        return fail(OT_ERR_INVALID, "ot_rays_fill_sections: the ray storage needs p, w, s and wl");
    if (int rc = check_sections("ot_rays_fill_sections", sc, rays)) return rc;
    if (first < 0 || count < 0 || first > rays->N || count > rays->N - first)
        return fail(OT_ERR_INVALID, "ot_rays_fill_sections: range outside the storage");
    if (int rc = require_device()) return rc;
    const RangeArgs* rg = nullptr;
    if (int rc = make_ranges(ranges, n_ranges, src, rays->N, &rg)) return rc;
    if (rays->nt < 3 || count == 0) return OT_OK;  // nothing is ever left out of two sections
    const TraceVariant v = trace_variant(sc, src, nullptr);
    if (v.error) return fail(OT_ERR_UNSUPPORTED, v.error);
    TraceLaunch L = make_launch(sc, src, rg, v, seed, (hipStream_t)stream);
    L.slots = nullptr;
    L.sec_end = rays->nt - 2;
    for_ray_chunks(first, count, [&](int64_t base, uint32_t n) {
        L.part = *rays;
        L.part.p += base; L.part.s += base; L.part.w += base; L.part.wl += base;
        L.part.n = nullptr;
        L.part.pol = nullptr;
        launch_chunk(OT_FORM_STORE, v.feat, L, base, n);
    });
    HIP_TRY(hipGetLastError());
    return OT_OK;
}

// One workgroup per piece: rows in use = ceil(max fill / 64); the slots of this piece between its fill and the end of the
// last row in use get weight 0 and finite positions.  Workgroup 0 reports result2 = {slots in use, living rays}.
__global__ __launch_bounds__(256) void tail_seal_kernel(TailOut T, long long* __restrict__ result2) {
    __shared__ unsigned int s_max[256];
    __shared__ unsigned long long s_sum[256];
    unsigned int mx = 0;
    unsigned long long sum = 0;
    for (int k = threadIdx.x; k < OT_TAIL_PIECES; k += 256) {
        const unsigned int f = T.fill[k];
        mx = f > mx ? f : mx;
        sum += f;
    }
    s_max[threadIdx.x] = mx;
    s_sum[threadIdx.x] = sum;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) {
            s_max[threadIdx.x] = s_max[threadIdx.x] > s_max[threadIdx.x + o] ? s_max[threadIdx.x] : s_max[threadIdx.x + o];
            s_sum[threadIdx.x] += s_sum[threadIdx.x + o];
        }
        __syncthreads();
    }
    const unsigned int rows = (s_max[0] + 63u) >> 6;
    const unsigned int piece = blockIdx.x;
    const int64_t N = T.cap;
    for (unsigned int q = T.fill[piece] + threadIdx.x; q < rows * 64u; q += 256) {
        const int64_t slot = tail_slot(q, piece);
        for (int c = 0; c < 6; c++) T.p[slot + c * N] = 0.0;
        T.w[slot] = 0.f;
        T.w[N + slot] = 0.f;
        T.wl[slot] = 0.f;
    }
    if (piece == 0 && threadIdx.x == 0) {
        result2[0] = (long long)rows * 64 * OT_TAIL_PIECES;
        result2[1] = (long long)s_sum[0];
    }
}

// Render-only chunk of Raytracer.iterative_render (raytracer.py:1235-1267: only the last chunk's rays are kept): n_rays
// rays are generated and traced without storing a section; the last section of every ray that is alive behind the last
// surface goes to the compact two-section storage `tail` (ot_trace_kernel.hpp::trace_tail_kernel).  Synchronous like
// ot_generate_and_trace_host.
extern "C" int64_t ot_tail_capacity(int64_t n_rays) {
    if (n_rays < 0) return 0;
    const int64_t waves = (n_rays + 63) / 64;
    return 65536 * std::max<int64_t>(1, (waves + OT_TAIL_PIECES - 1) / OT_TAIL_PIECES);
}

extern "C" int ot_scene_tail_supported(const ot_scene* scene) { return scene ? 1 : 0; }  // (every feature level has the form)

extern "C" int ot_generate_and_trace_tail(const ot_scene* scene, const ot_sources* src, const ot_source_range* ranges,
                                          int32_t n_ranges, uint64_t seed, int64_t n_rays, const ot_rays* tail,
                                          uint32_t* fill, int64_t* result2, int64_t* msgs_host, void* stream) {
    if (!scene || !src || !tail || !fill || !result2 || !msgs_host)
        return fail(OT_ERR_INVALID, "ot_generate_and_trace_tail: null argument");
    if (n_rays < 1) return fail(OT_ERR_INVALID, "ot_generate_and_trace_tail: no rays");
    if (tail->nt != 2 || !tail->p || !tail->w || !tail->wl)
        return fail(OT_ERR_INVALID, "ot_generate_and_trace_tail: the tail storage has two sections and needs p, w and wl");
    if (tail->N < ot_tail_capacity(n_rays) || tail->N % 65536)
        return fail(OT_ERR_INVALID, "ot_generate_and_trace_tail: tail storage smaller than ot_tail_capacity(n_rays)");
    const RangeArgs* rg = nullptr;
    if (int rc = make_ranges(ranges, n_ranges, src, n_rays, &rg)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const TailOut T = tail_out(tail, fill);
    HIP_TRY(hipMemsetAsync(fill, 0, sizeof(uint32_t) * OT_TAIL_PIECES, st));
    ot_scene* sc = const_cast<ot_scene*>(scene);
    if (int rc = pinned_counters(sc)) return rc;
    const TraceVariant v = trace_variant(sc, src, nullptr);
    if (v.error) return fail(OT_ERR_UNSUPPORTED, v.error);
    TraceLaunch L = make_launch(sc, src, rg, v, seed, st);  // (index_spec stays: no stored trace)
    L.tail = T;
    if (int rc = trace_chunks(sc, n_rays, nullptr, st, [&](int64_t base, uint32_t n) { launch_chunk(OT_FORM_TAIL, v.feat, L, base, n); }))
        return rc;
    hipLaunchKernelGGL(tail_seal_kernel, dim3(OT_TAIL_PIECES), dim3(256), 0, st, T, (long long*)result2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(msgs_host, scene->pin_msgs, msgs_bytes(scene));
    return OT_OK;
}

// The living rays of a STORED chunk join a tail storage: `iterative_render` leaves the rays of its last chunk in the tracer
// (raytracer.py:1235-1267), so that chunk goes through the ray storage -- but its binning need not be a pass of its own (for
// 2^20 rays the fixed costs of the tile chain are most of it: 0.3-0.4 ms, a seventh of a rank's time when 2e8 rays are sharded
// over eight GPUs): the last sections of its living rays are appended to the tail of the render-only chunk before it, weights
// scaled to that chunk's rays (x chunk rays / tail rays, in f64, rounded once), and the two are binned together.
// Wave k of the range continues the round robin over the pieces behind the `waves_before` waves that filled the tail.
__global__ __launch_bounds__(256) void tail_append_kernel(ot_rays R, int64_t first, int64_t count, TailOut T, int64_t waves_before,
                                                          double weight_scale) {
    const int64_t q = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool have = q < count;
    const int64_t r = first + (have ? q : 0), N = R.N;
    const int nt = R.nt, kq = nt - 2;
    const float w = have ? R.w[r + N * kq] : 0.f;
    const bool alive = w > 0.f;
    const unsigned long long m = __ballot(alive);
    if (!m) return;
    const unsigned int n_alive = (unsigned int)__popcll(m);
    const unsigned int rank = __builtin_amdgcn_mbcnt_hi((unsigned int)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned int)m, 0u));
    const unsigned int piece = (unsigned int)((waves_before + (q >> 6)) & (OT_TAIL_PIECES - 1));
    unsigned int q0 = 0;
    if (rank == 0 && alive) q0 = atomicAdd(&T.fill[piece], n_alive);
    q0 = __shfl(q0, __ffsll((long long)m) - 1);
    if (alive) {
        const int64_t slot = tail_slot(q0 + rank, piece);
        const int64_t C = T.cap;
        double* px = T.p + slot;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            px[(2 * c) * C] = R.p[r + N * (kq + (int64_t)nt * c)];
            px[(2 * c + 1) * C] = R.p[r + N * (kq + 1 + (int64_t)nt * c)];
        }
        T.w[slot] = (float)((double)w * weight_scale);
        T.w[C + slot] = 0.f;
        T.wl[slot] = R.wl[r];
    }
}

extern "C" int ot_tail_append(const ot_rays* rays, int64_t first, int64_t count, double weight_scale, int64_t rays_before,
                              const ot_rays* tail, uint32_t* fill, int64_t* result2, void* stream) {
    if (!rays || !tail || !fill || !result2) return fail(OT_ERR_INVALID, "ot_tail_append: null argument");
    if (!rays->p || !rays->w || !rays->wl || rays->nt < 2) return fail(OT_ERR_INVALID, "ot_tail_append: the ray storage needs p, w, wl and two sections");
    if (first < 0 || count < 0 || first + count > rays->N || rays_before < 0) return fail(OT_ERR_INVALID, "ot_tail_append: range outside the storage");
    if (tail->nt != 2 || !tail->p || !tail->w || !tail->wl) return fail(OT_ERR_INVALID, "ot_tail_append: the tail storage has two sections and needs p, w and wl");
    if (!(weight_scale > 0.0) || !std::isfinite(weight_scale)) return fail(OT_ERR_INVALID, "ot_tail_append: weight_scale must be positive");
    const int64_t waves_before = (rays_before + 63) / 64, waves = (count + 63) / 64;
    if (tail->N % 65536 || tail->N < 65536 * std::max<int64_t>(1, (waves_before + waves + OT_TAIL_PIECES - 1) / OT_TAIL_PIECES))
        return fail(OT_ERR_INVALID, "ot_tail_append: tail storage smaller than ot_tail_capacity(rays_before + count + 64)");
    if (int rc = require_device()) return rc;
    hipStream_t st = (hipStream_t)stream;
    const TailOut T = tail_out(tail, fill);
    if (count) hipLaunchKernelGGL(tail_append_kernel, grid_for(count), dim3(256), 0, st, *rays, first, count, T, waves_before, weight_scale);
    hipLaunchKernelGGL(tail_seal_kernel, dim3(OT_TAIL_PIECES), dim3(256), 0, st, T, (long long*)result2);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(st));
    return OT_OK;
}
