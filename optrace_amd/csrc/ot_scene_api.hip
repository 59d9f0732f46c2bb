// C-ABI, scene stage: host-side compilation of surfaces and scenes into their device records (ot_scene.hpp).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ot_device.hpp"
#include "ot_host.hpp"
#include "ot_trace_kernel.hpp"

// ---------------------------------------------------------------------------------------------------------
// scene compilation (host)
// ---------------------------------------------------------------------------------------------------------
static double conic_sag(double rho, double k1rho2, double r2) { return rho * r2 / (1 + std::sqrt(1 - k1rho2 * r2)); }

static int64_t spline_table_len(const ot_surface& s) {
    const int64_t n = s.nknots, nc = n - OT_SPL_K - 1;
    if (s.kind == OT_SURF_DATA1D) return 3 * n;
    if (s.kind == OT_SURF_DATA2D) return n + nc * nc + 2 * (nc - 1) * nc;
    return 0;
}

// cells per dimension of the mask bitmap behind the spline tables (OT_SURF_FLAG_MASK_TABLE), 0 without one, -1 if
// the count stored there is not a whole number in 1 .. 2^15 (2D) or 1 .. 2^20 (1D)
static int64_t mask_table_cells(const ot_surface& s) {
    if (!(s.flags & OT_SURF_FLAG_MASK_TABLE)) return 0;
    const int64_t at = spline_table_len(s);
    if (!s.tab || s.tab_len <= at) return -1;
    const double n = s.tab[at];
    if (!(n >= 1.0 && n <= (s.kind == OT_SURF_DATA1D ? 1048576.0 : 32768.0)) || n != std::floor(n)) return -1;
    return (int64_t)n;
}

static int64_t surface_table_len(const ot_surface& s) {
    int64_t len = spline_table_len(s);
    const int64_t n = mask_table_cells(s);
    if (n > 0) len += 1 + ((s.kind == OT_SURF_DATA1D ? n : n * n) + 63) / 64;
    return len;
}

int compile_surface(const ot_surface& s, SurfDev& d) {
    std::memset(&d, 0, sizeof(d));
    const double NE = OT_N_EPS_SURF;
    d.kind = s.kind;
    d.ncoeff = s.ncoeff;
    d.flat = (s.z_max == s.z_min);
    d.px = s.pos[0];
    d.py = s.pos[1];
    d.pz = s.pos[2];
    d.z_min = s.z_min;
    d.z_max = s.z_max;
    d.z_lo = s.z_min - NE;
    d.z_hi = s.z_max + NE;
    d.z_beh = s.z_max + NE;
    d.zt1 = s.z_min - OT_C_EPS / 10;
    d.zt2 = s.z_max + OT_C_EPS / 10;
    d.edge_val = s.z_max;
    d.r_edge = s.r - NE;
    switch (s.kind) {
        case OT_SURF_CIRCLE:
            d.r_eps2 = std::pow(s.r + NE, 2.0);
            break;
        case OT_SURF_RING:
            d.r_eps2 = std::pow(s.r + NE, 2.0);
            d.ri_eps2 = std::pow(s.ri - NE, 2.0);
            d.ri = s.ri;
            break;
        case OT_SURF_RECT:
        case OT_SURF_SLIT: {
            d.rot = (s.angle != 0.0);
            d.cna = std::cos(-s.angle);
            d.sna = std::sin(-s.angle);
            d.cpa = std::cos(s.angle);
            d.spa = std::sin(s.angle);
            double xs = -s.dim[0] / 2, xe = s.dim[0] / 2, ys = -s.dim[1] / 2, ye = s.dim[1] / 2;
            d.ox_lo = xs - NE;
            d.ox_hi = xe + NE;
            d.oy_lo = ys - NE;
            d.oy_hi = ye + NE;
            if (s.kind == OT_SURF_SLIT) {
                double xsi = -s.dimi[0] / 2, xei = s.dimi[0] / 2, ysi = -s.dimi[1] / 2, yei = s.dimi[1] / 2;
                d.ix_lo = xsi + NE;
                d.ix_hi = xei - NE;
                d.iy_lo = ysi + NE;
                d.iy_hi = yei - NE;
                d.hdx = s.dimi[0] / 2;
                d.hdy = s.dimi[1] / 2;
            }
            break;
        }
        case OT_SURF_CONIC:
        case OT_SURF_ASPHERE: {
            if (s.R == 0.0 || !std::isfinite(s.R)) return fail(OT_ERR_INVALID, "surface: R must be finite and non-zero");
            const bool long_asph = s.kind == OT_SURF_ASPHERE && (s.flags & OT_SURF_FLAG_ASPH_TABLE);
            if (s.kind == OT_SURF_ASPHERE && !long_asph && (s.ncoeff < 1 || s.ncoeff > OT_MAX_ASPH))
                return fail(OT_ERR_UNSUPPORTED, "asphere: ncoeff out of range (more than OT_MAX_ASPH coefficients travel "
                                                "in tab, OT_SURF_FLAG_ASPH_TABLE)");
            if (long_asph && (s.ncoeff < 1 || !s.tab || s.tab_len != (int64_t)s.ncoeff))
                return fail(OT_ERR_INVALID, "asphere: OT_SURF_FLAG_ASPH_TABLE needs tab with tab_len == ncoeff");
            const double* const cf = long_asph ? s.tab : s.coeff;
            d.r_eps2 = std::pow(s.r + NE, 2.0);
            d.k = s.k;
            d.k1 = s.k + 1;
            d.rho = 1 / s.R;
            d.nrho = -d.rho;
            d.rho2 = std::pow(d.rho, 2.0);
            d.k1rho2 = (s.k + 1) * d.rho2;
            d.krho2 = s.k * d.rho2;
            d.inv_rho = 1 / d.rho;
            d.two_inv_rho = 2 / d.rho;
            for (int j = 0; j < s.ncoeff && j < OT_MAX_ASPH; j++) {
                d.coeff[j] = cf[j];
                d.dcoeff[j] = cf[j] * (double)(2 * (j + 1));
            }
            // more coefficients than the record holds: the device reads them from the surface's table (device_table);
            // the host pointer marks that here, the caller swaps in the device copy
            if (long_asph && s.ncoeff > OT_MAX_ASPH) d.tab = s.tab;
            // Surface.values outside the mask: pos_z + _values(r - N_EPS, 0) (surface.py:153-162)
            if (!d.flat) {
                double re = s.r - NE;
                double v;
                if (s.kind == OT_SURF_CONIC) {
                    v = conic_sag(d.rho, d.k1rho2, re * re + 0.0 * 0.0);
                } else {
                    double r = std::sqrt(re * re + 0.0 * 0.0);
                    v = d.rho * (r * r) / (1 + std::sqrt(1 - d.k1rho2 * (r * r)));
                    double y = 0.0;
                    for (int j = s.ncoeff - 1; j >= 0; j--) {
                        y = y * r + cf[j];
                        y = y * r + 0.0;
                    }
                    y = y * r + 0.0;
                    v += y;
                }
                d.edge_val = s.pos[2] + v;
            }
            break;
        }
        case OT_SURF_TILTED: {
            const double* nv = s.normal;
            if (!(nv[2] > 0.0) || !std::isfinite(nv[0]) || !std::isfinite(nv[1]))
                return fail(OT_ERR_INVALID, "tilted surface: normal[2] must be above 0");
            d.r_eps2 = std::pow(s.r + NE, 2.0);
            d.nx = nv[0];
            d.ny = nv[1];
            d.nz = nv[2];
            d.mx = -nv[0] / nv[2];  // tilted_surface.py:69-70
            d.my = -nv[1] / nv[2];
            if (!d.flat) d.edge_val = s.pos[2] + ((s.r - NE) * d.mx + 0.0 * d.my);
            break;
        }
        case OT_SURF_DATA1D:
        case OT_SURF_DATA2D: {
            const int n = s.nknots, nc = n - OT_SPL_K - 1;
            if (!s.tab || nc < OT_SPL_K + 1) return fail(OT_ERR_INVALID, "data surface: spline tables missing or too short");
            if (mask_table_cells(s) < 0) return fail(OT_ERR_INVALID, "data surface: mask table header missing or out of range");
            if (s.tab_len != surface_table_len(s)) return fail(OT_ERR_INVALID, "data surface: tab_len does not match nknots");
            if (!(s.sign == 1.0 || s.sign == -1.0)) return fail(OT_ERR_INVALID, "data surface: sign must be +1 or -1");
            d.r_eps2 = std::pow(s.r + NE, 2.0);
            d.sgn = s.sign;
            d.offs = s.offset;
            d.nk = n;
            d.deriv_unrot = (s.flags & OT_SURF_FLAG_DERIV_UNROTATED) ? 1 : 0;
            d.mask_n = (int32_t)mask_table_cells(s);
            if (d.mask_n) {
                d.mask_off = spline_table_len(s) + 1;
                d.mask_r = s.r;
                d.mask_scale = (s.kind == OT_SURF_DATA1D ? (double)d.mask_n : 0.5 * (double)d.mask_n) / s.r;
            }
            const double span = s.tab[nc] - s.tab[OT_SPL_K];  // t(nk1 + 1) - t(k1)
            if (!(span > 0.0)) return fail(OT_ERR_INVALID, "data surface: knots must increase");
            d.inv_h = (double)(nc - OT_SPL_K - 1 > 0 ? nc - OT_SPL_K - 1 : 1) / span;
            {   // equidistant part of the knots: indices K + 1 .. n - K - 2 (ot_spline.hpp::bspl_basis)
                const int ulo = OT_SPL_K + 1, uhi = n - OT_SPL_K - 2;
                d.ku_lo = s.tab[OT_SPL_K];  // t(k1), t(nk1 + 1): the range arguments are clamped to
                d.ku_hi = s.tab[nc];
                d.ku_t0 = d.ku_h = d.ku_inv_h = 0.0;  // ku_h == 0: no equidistant part (table path everywhere)
                if (uhi - ulo >= 2 * OT_SPL_K) {
                    const double h = (s.tab[uhi] - s.tab[ulo]) / (double)(uhi - ulo);
                    bool uniform = h > 0.0;
                    for (int i = ulo; i <= uhi && uniform; i++)
                        uniform = std::fabs(s.tab[i] - (s.tab[ulo] + (i - ulo) * h)) <= 1e-9 * h;
                    if (uniform) {
                        d.ku_t0 = s.tab[ulo];
                        d.ku_h = h;
                        d.ku_inv_h = 1.0 / h;
                    }
                }
            }
            if (s.kind == OT_SURF_DATA2D) {
                d.rot = (s.angle != 0.0);
                d.cna = std::cos(-s.angle);
                d.sna = std::sin(-s.angle);
                d.cpa = std::cos(s.angle);
                d.spa = std::sin(s.angle);
            }
            d.tab = s.tab;  // host pointer for the edge value below; the caller swaps in the device copy
            if (!d.flat) d.edge_val = s.pos[2] + data_values_rel(d, s.r - NE, 0.0);
            break;
        }
        default:
            return fail(OT_ERR_INVALID, "surface: unknown kind");
    }
    return OT_OK;
}

DeviceTable::DeviceTable(const ot_surface& s, const SurfDev& d) {
    if (!d.tab) return;
    if (s.kind == OT_SURF_ASPHERE) {
        const int npad = asph_padded(s.ncoeff);
        own.assign(2 * (size_t)npad, 0.0);
        for (int j = 0; j < s.ncoeff; j++) {
            own[j] = s.tab[j];
            own[npad + j] = s.tab[j] * (double)(2 * (j + 1));
        }
        src = own.data();
        len = own.size();
    } else {
        src = s.tab;
        len = (size_t)s.tab_len;
    }
}

int LeafSurface::init(const ot_surface* surf, hipStream_t stream) {
    st = stream;
    if (int rc = compile_surface(*surf, d)) return rc;
    if (d.tab) {
        const DeviceTable t(*surf, d);
        HIP_TRY(hipMalloc((void**)&dev_tab, sizeof(double) * t.len));
        HIP_TRY(hipMemcpyAsync(dev_tab, t.src, sizeof(double) * t.len, hipMemcpyHostToDevice, st));
        if (!t.own.empty()) HIP_TRY(hipStreamSynchronize(st));  // the source is a temporary of this call
        d.tab = dev_tab;
    }
    return OT_OK;
}

LeafSurface::~LeafSurface() {
    if (dev_tab) {
        (void)hipStreamSynchronize(st);  // kernels of this call still read the tables
        (void)hipFree(dev_tab);
    }
}

// flatten elements into one step per tracing surface
static int compile_steps(const ot_scene_desc* desc, const std::vector<SurfDev>& surfs, std::vector<StepDev>& steps, int& n_hurb) {
    n_hurb = 0;
    for (int i = 0; i < desc->n_elements; i++) {
        const ot_element& e = desc->elements[i];
        if (e.front < 0 || e.front >= desc->n_surfaces) return fail(OT_ERR_INVALID, "element: front surface out of range");
        StepDev d;
        std::memset(&d, 0, sizeof(d));
        d.surf = e.front;
        d.n_next = -1;
        d.filter = -1;
        d.hurb_slot = -1;
        switch (e.kind) {
            case OT_EL_LENS: {
                if (e.back < 0 || e.back >= desc->n_surfaces) return fail(OT_ERR_INVALID, "lens: back surface out of range");
                if (e.n_lens < 0 || e.n_lens >= desc->n_media || e.n_after < 0 || e.n_after >= desc->n_media)
                    return fail(OT_ERR_INVALID, "lens: medium out of range");
                d.kind = OT_STEP_LENS_FRONT;
                d.n_next = e.n_lens;
                steps.push_back(d);
                d.kind = OT_STEP_LENS_BACK;
                d.surf = e.back;
                d.n_next = e.n_after;
                steps.push_back(d);
                break;
            }
            case OT_EL_IDEAL_LENS:
                if (e.n_after < 0 || e.n_after >= desc->n_media) return fail(OT_ERR_INVALID, "ideal lens: medium out of range");
                if (e.D == 0.0) return fail(OT_ERR_INVALID, "ideal lens: optical power must be non-zero");
                d.kind = OT_STEP_IDEAL;
                d.n_next = e.n_after;
                d.f = 1000 / e.D;
                d.fsign = (d.f > 0) - (d.f < 0);
                steps.push_back(d);
                break;
            case OT_EL_FILTER:
                if (e.filter < 0 || e.filter >= desc->n_filters) return fail(OT_ERR_INVALID, "filter index out of range");
                d.kind = OT_STEP_FILTER;
                d.filter = e.filter;
                steps.push_back(d);
                break;
            case OT_EL_APERTURE:
                d.kind = OT_STEP_APERTURE;
                d.hurb = (desc->use_hurb && e.hurb && i != desc->n_elements - 1) ? 1 : 0;  // raytracer.py:385
                if (d.hurb && surfs[e.front].kind != OT_SURF_RING && surfs[e.front].kind != OT_SURF_SLIT)
                    return fail(OT_ERR_UNSUPPORTED, "HURB is only defined for ring and slit apertures (raytracer.py:548-552)");
                d.hurb_slot = d.hurb ? n_hurb++ : -1;
                steps.push_back(d);
                break;
            default:
                return fail(OT_ERR_INVALID, "element: unknown kind");
        }
    }
    return OT_OK;
}

static int hot_form(const SurfDev& sf) {
    if (sf.kind == OT_SURF_CIRCLE && sf.flat) return OT_HOT_FLAT;
    if (sf.kind == OT_SURF_RING && sf.flat) return OT_HOT_RING;
    if (sf.kind != OT_SURF_CONIC || sf.flat) return OT_HOT_OTHER;
    if (!(sf.k == 0.0)) return OT_HOT_CONIC;  // the comparisons of find_hit_conic and surf_normal, taken once
    return std::fabs(sf.inv_rho) <= OT_PLAIN_SPHERE_R ? OT_HOT_SPHERE : OT_HOT_SPHERE_STABLE;
}

// the hot records of the steps (ot_scene.hpp::HotStep) and one record of padding; hot_steps == 0: every form is OTHER
static void compile_hot_steps(const std::vector<StepDev>& steps, const std::vector<SurfDev>& surfs, bool hot_steps,
                       std::vector<HotStep>& out) {
    out.assign(steps.size() + 1, HotStep{});
    for (size_t i = 0; i < steps.size(); i++) {
        const StepDev& st = steps[i];
        const SurfDev& sf = surfs[st.surf];
        HotStep& h = out[i];
        h.kind = st.kind;
        h.form = hot_steps ? hot_form(sf) : OT_HOT_OTHER;
        h.surf = st.surf;
        h.n_next = st.n_next;
        h.filter = st.filter;
        h.hurb = st.hurb;
        h.hurb_slot = st.hurb_slot;
        h.px = sf.px, h.py = sf.py, h.pz = sf.pz, h.r_eps2 = sf.r_eps2;
        h.z_max = sf.z_max, h.z_lo = sf.z_lo, h.z_hi = sf.z_hi, h.k1 = sf.k1;
        h.inv_rho = sf.inv_rho, h.two_inv_rho = sf.two_inv_rho, h.k = sf.k, h.ri_eps2 = sf.ri_eps2;
        h.nrho = sf.nrho, h.rho2 = sf.rho2, h.krho2 = sf.krho2, h.f = st.f, h.fsign = st.fsign;
    }
}

extern "C" int ot_scene_create(const ot_scene_desc* desc, ot_scene** out) {
    if (!desc || !out) return fail(OT_ERR_INVALID, "ot_scene_create: null argument");
    if (int rc = require_device()) return rc;
    if (desc->n_elements < 1 || desc->n_surfaces < 1 || desc->n_media < 1)
        return fail(OT_ERR_INVALID, "scene needs at least one element, surface and medium");
    if (desc->n0 < 0 || desc->n0 >= desc->n_media) return fail(OT_ERR_INVALID, "scene: n0 out of range");

    std::vector<SurfDev> surfs(desc->n_surfaces);
    for (int i = 0; i < desc->n_surfaces; i++)
        if (int rc = compile_surface(desc->surfaces[i], surfs[i])) return rc;

    std::vector<StepDev> steps;
    int n_hurb = 0;
    if (int rc = compile_steps(desc, surfs, steps, n_hurb)) return rc;
    std::vector<HotStep> hot;
    compile_hot_steps(steps, surfs, true, hot);
    bool needs_hurb = false, needs_ideal_filter = false;  // anything beyond lens surfaces and plain apertures
    int hit_level = OT_HIT_CLOSED;
    for (const StepDev& d : steps) {
        needs_ideal_filter |= d.kind == OT_STEP_IDEAL || d.kind == OT_STEP_FILTER;
        needs_hurb |= d.hurb != 0;
        const SurfDev& sf = surfs[d.surf];
        int lv = OT_HIT_CLOSED;
        if (sf.kind == OT_SURF_DATA1D || sf.kind == OT_SURF_DATA2D) {
            // flat data surfaces have a closed-form hit -- unless a mask_func bitmap has to be consulted
            if (!sf.flat || sf.mask_n != 0) lv = OT_HIT_SPLINE;
        } else if (sf.kind >= OT_SURF_ASPHERE && !sf.flat) {
            // an asphere with more coefficients than the record holds reads them from its table: the table-carrying level
            lv = (sf.kind == OT_SURF_ASPHERE && sf.ncoeff > OT_MAX_ASPH) ? OT_HIT_SPLINE : OT_HIT_ILLINOIS;
        }
        hit_level = std::max(hit_level, lv);
    }
    const int nt = (int)steps.size() + 1;  // sections = tracing surfaces + 2, the end aperture being a step

    std::vector<FilterDev> filts(desc->n_filters > 0 ? desc->n_filters : 1);
    for (int i = 0; i < desc->n_filters; i++) {
        const ot_filter& f = desc->filters[i];
        FilterDev& d = filts[i];
        std::memset(&d, 0, sizeof(d));
        d.type = f.type;
        d.inverse = f.inverse;
        d.tab_len = f.tab_len;
        d.tab_off = f.tab_off;
        d.val = f.val;
        d.wl0 = f.wl0;
        d.wl1 = f.wl1;
        d.mu32 = (float)f.mu;
        d.den32 = (float)(2 * std::pow(f.sig, 2.0));
        d.val32 = (float)f.val;
        if ((f.type == OT_T_DATA || f.type == OT_T_LINES) &&
            (f.tab_off < 0 || f.tab_off + 2 * (int64_t)f.tab_len > desc->table_pool_len))
            return fail(OT_ERR_INVALID, "filter table outside the pool");
    }
    bool needs_tables = false;
    for (int i = 0; i < desc->n_filters; i++)
        needs_tables |= (desc->filters[i].type == OT_T_DATA || desc->filters[i].type == OT_T_LINES);
    for (int i = 0; i < desc->n_media; i++) {
        const ot_medium& m = desc->media[i];
        needs_tables |= (m.model == OT_N_DATA || m.model == OT_N_LINES);
        if ((m.model == OT_N_DATA || m.model == OT_N_LINES) &&
            (m.tab_off < 0 || m.tab_off + 2 * (int64_t)m.tab_len > desc->table_pool_len))
            return fail(OT_ERR_INVALID, "medium table outside the pool");
    }

    // discrete spectra: tabulate n(lambda), n1/n2 and filter T per step and line (IEEE arithmetic on the host, the
    // same expressions the device evaluates; raytracer.py:305, 327-332, 799, 380)
    std::vector<double> line_tab;
    int n_lines = 0;
    if (desc->n_lines > 0 && desc->n_lines <= OT_MAX_LINES && desc->lines) {
        n_lines = desc->n_lines;
        const int rows = 3 * (int)steps.size() + 2;
        line_tab.assign((size_t)rows * OT_MAX_LINES, 0.0);
        for (int j = 0; j < n_lines; j++) {
            const float wl32 = (float)desc->lines[j];
            line_tab[j] = (double)wl32;
            double n_cur = medium_n(desc->media[desc->n0], desc->table_pool, wl32);
            line_tab[(size_t)(1 + 3 * steps.size()) * OT_MAX_LINES + j] = n_cur;  // ambient row
            for (size_t i = 0; i < steps.size(); i++) {
                const StepDev& d = steps[i];
                double n_next = n_cur, Nq = 1.0, T = 1.0;
                if (d.kind <= OT_STEP_IDEAL) {
                    n_next = medium_n(desc->media[d.n_next], desc->table_pool, wl32);
                    Nq = n_cur / n_next;
                } else if (d.kind == OT_STEP_FILTER) {
                    T = filter_T(filts[d.filter], desc->table_pool, wl32);
                }
                line_tab[(size_t)(1 + 3 * i + 0) * OT_MAX_LINES + j] = n_next;
                line_tab[(size_t)(1 + 3 * i + 1) * OT_MAX_LINES + j] = Nq;
                line_tab[(size_t)(1 + 3 * i + 2) * OT_MAX_LINES + j] = T;
                n_cur = n_next;
            }
        }
    }

    // one device blob: header | surfaces | elements | media | filters | pool
    size_t o_hdr = 0;
    size_t o_surf = align_up(o_hdr + sizeof(SceneDev));
    size_t o_elem = align_up(o_surf + sizeof(SurfDev) * surfs.size());
    size_t o_med = align_up(o_elem + sizeof(StepDev) * steps.size());
    size_t o_flt = align_up(o_med + sizeof(ot_medium) * desc->n_media);
    size_t o_pool = align_up(o_flt + sizeof(FilterDev) * filts.size());
    size_t pool_n = desc->table_pool_len > 0 ? (size_t)desc->table_pool_len : 1;
    size_t o_lines = align_up(o_pool + sizeof(double) * pool_n);
    size_t o_cnt = align_up(o_lines + sizeof(double) * (line_tab.size() + 1));
    size_t o_hot = (o_cnt + sizeof(unsigned int) * (size_t)OT_CNT_SLOTS * (OT_N_INFOS * nt + 1) + 63) / 64 * 64;
    size_t o_stab = align_up(o_hot + sizeof(HotStep) * hot.size());
    std::vector<size_t> stab_off(surfs.size(), 0);  // spline tables of data surfaces, coefficients of long aspheres
    std::vector<DeviceTable> stabs;
    stabs.reserve(surfs.size());
    size_t total = o_stab;
    for (size_t i = 0; i < surfs.size(); i++) {
        stabs.emplace_back(desc->surfaces[i], surfs[i]);
        if (!surfs[i].tab) continue;
        stab_off[i] = total;
        total = align_up(total + sizeof(double) * stabs[i].len);
    }
    total = align_up(total + 1);

    std::vector<char> host(total, 0);
    char* blob = nullptr;
    HIP_TRY(hipMalloc((void**)&blob, total));

    SceneDev h;
    std::memset(&h, 0, sizeof(h));
    std::memcpy(h.outline, desc->outline, sizeof(h.outline));
    h.n_surfaces = desc->n_surfaces;
    h.n_steps = (int32_t)steps.size();
    h.n_media = desc->n_media;
    h.n_filters = desc->n_filters;
    h.n0 = desc->n0;
    h.no_pol = desc->no_pol;
    h.use_hurb = desc->use_hurb;
    h.nt = nt;
    h.n_hurb = n_hurb;
    h.hurb_factor = desc->hurb_factor;
    h.surfaces = (const SurfDev*)(blob + o_surf);
    h.steps = (const StepDev*)(blob + o_elem);
    h.media = (const ot_medium*)(blob + o_med);
    h.filters = (const FilterDev*)(blob + o_flt);
    h.pool = (const double*)(blob + o_pool);
    h.pool_len = desc->table_pool_len;
    h.n_lines = n_lines;
    h.line_tab = (const double*)(blob + o_lines);
    h.hot = (const HotStep*)(blob + o_hot);

    for (size_t i = 0; i < surfs.size(); i++) {
        if (!surfs[i].tab) continue;
        std::memcpy(host.data() + stab_off[i], stabs[i].src, sizeof(double) * stabs[i].len);
        surfs[i].tab = (const double*)(blob + stab_off[i]);
    }
    std::memcpy(host.data() + o_hdr, &h, sizeof(h));
    std::memcpy(host.data() + o_surf, surfs.data(), sizeof(SurfDev) * surfs.size());
    std::memcpy(host.data() + o_elem, steps.data(), sizeof(StepDev) * steps.size());
    std::memcpy(host.data() + o_med, desc->media, sizeof(ot_medium) * desc->n_media);
    std::memcpy(host.data() + o_flt, filts.data(), sizeof(FilterDev) * filts.size());
    if (desc->table_pool_len > 0)
        std::memcpy(host.data() + o_pool, desc->table_pool, sizeof(double) * desc->table_pool_len);
    if (!line_tab.empty()) std::memcpy(host.data() + o_lines, line_tab.data(), sizeof(double) * line_tab.size());
    std::memcpy(host.data() + o_hot, hot.data(), sizeof(HotStep) * hot.size());
    hipError_t e = hipMemcpy(blob, host.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(blob);
        return fail(OT_ERR_HIP, std::string("scene upload: ") + hipGetErrorString(e));
    }

    ot_scene* sc = new ot_scene;
    sc->h = h;
    sc->needs_tables = needs_tables;
    sc->cnt_slots = (unsigned int*)(blob + o_cnt);
    // the "full" bit of the kernel variants: HURB; at hit level 0 ideal lenses and filters as well (trace_ray)
    sc->needs_full = needs_hurb || (needs_ideal_filter && hit_level == OT_HIT_CLOSED);
    sc->hit_level = hit_level;
    sc->d = (SceneDev*)(blob + o_hdr);
    sc->blob = blob;
    sc->hot_host = new HotStep[hot.size()];
    std::memcpy(sc->hot_host, hot.data(), sizeof(HotStep) * hot.size());
    (void)hipGetDevice(&sc->device);
    *out = sc;
    return OT_OK;
}

extern "C" void ot_scene_destroy(ot_scene* sc) {
    if (!sc) return;
    (void)hipFree(sc->blob);
    if (sc->pin_msgs) (void)hipHostFree(sc->pin_msgs);
    if (sc->ev0) (void)hipEventDestroy(sc->ev0);
    if (sc->ev1) (void)hipEventDestroy(sc->ev1);
    delete[] sc->hot_host;
    delete sc;
}

// Kernel timing for measurements (bench.py): with timing on, every trace launch is bracketed by two events on its
// own stream, recorded right before and right after the tracing kernel (the counter reduction stays outside).
extern "C" int ot_scene_set_timing(ot_scene* sc, int32_t on) {
    if (!sc) return fail(OT_ERR_INVALID, "ot_scene_set_timing: null scene");
    if (on && !sc->ev0) {
        HIP_TRY(hipEventCreate(&sc->ev0));
        HIP_TRY(hipEventCreate(&sc->ev1));
    }
    sc->timing = on != 0;
    sc->ev_valid = false;
    return OT_OK;
}

// The index plane ot_rays.n is a function of (scene, section, wavelength) alone and nothing in the library reads it: a caller
// who does not need it after every trace switches its stores off and writes it with ot_rays_fill_index when it is asked for.
// The polarisation planes can be repeated from (scene, sources, ranges, seed) by ot_rays_fill_pol, and so can position and
// weight of the sections before the last two (OT_DEFER_SECTIONS, ot_rays_fill_sections).  One mask holds all three.
extern "C" int ot_scene_set_deferred_planes(ot_scene* sc, uint32_t mask) {
    if (!sc) return fail(OT_ERR_INVALID, "ot_scene_set_deferred_planes: null scene");
    if (mask & ~(uint32_t)(OT_DEFER_INDEX | OT_DEFER_POL | OT_DEFER_SECTIONS)) return fail(OT_ERR_INVALID, "ot_scene_set_deferred_planes: unknown bit in the mask");
    sc->deferred = mask;
    return OT_OK;
}

// on: complete storage, every plane (the whole mask is cleared); off: OT_DEFER_INDEX joins the mask
extern "C" int ot_scene_set_index_store(ot_scene* sc, int32_t on) {
    if (!sc) return fail(OT_ERR_INVALID, "ot_scene_set_index_store: null scene");
    return ot_scene_set_deferred_planes(sc, on ? 0u : (sc->deferred | OT_DEFER_INDEX));
}

// The hot records of the step loop (ot_scene.hpp::HotStep) with their forms (on, the default) or with every form OTHER, so
// that every step reads its SurfDev record: the same kernel either way, for comparing the two paths.  Rewrites the device
// table on the scene's own device, whichever device is current; launches already queued there are waited for first.
namespace {
struct SceneDevice {  // the scene's device for the length of a call
    int before = -1;
    explicit SceneDevice(const ot_scene* sc) {
        if (hipGetDevice(&before) != hipSuccess || before == sc->device || hipSetDevice(sc->device) != hipSuccess) before = -1;
    }
    ~SceneDevice() {
        if (before >= 0) (void)hipSetDevice(before);
    }
};
}  // namespace

extern "C" int ot_scene_set_hot_steps(ot_scene* sc, int32_t on) {
    if (!sc) return fail(OT_ERR_INVALID, "ot_scene_set_hot_steps: null scene");
    if ((on != 0) == sc->hot_steps) return OT_OK;
    const size_t n = (size_t)sc->h.n_steps + 1;
    std::vector<HotStep> tab(sc->hot_host, sc->hot_host + n);
    if (!on)
        for (HotStep& h : tab) h.form = OT_HOT_OTHER;
    const SceneDevice on_device(sc);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(const_cast<HotStep*>(sc->h.hot), tab.data(), sizeof(HotStep) * n, hipMemcpyHostToDevice));
    sc->hot_steps = on != 0;
    return OT_OK;
}

// the hot records as the device holds them now (n_steps + 1 records of sizeof(HotStep)), for checks of the switch above
extern "C" int ot_scene_read_hot_steps(const ot_scene* sc, void* buf, int64_t buf_bytes, int32_t* count) {
    if (!sc || !buf || !count) return fail(OT_ERR_INVALID, "ot_scene_read_hot_steps: null argument");
    const size_t n = (size_t)sc->h.n_steps + 1;
    *count = (int32_t)n;
    if (buf_bytes < (int64_t)(n * sizeof(HotStep))) return fail(OT_ERR_INVALID, "ot_scene_read_hot_steps: buffer too small");
    const SceneDevice on_device(sc);
    HIP_TRY(hipDeviceSynchronize());
    HIP_TRY(hipMemcpy(buf, sc->h.hot, sizeof(HotStep) * n, hipMemcpyDeviceToHost));
    return OT_OK;
}

// Host only, no device: the records ot_scene_create compiles from a scene description, copied into the caller's buffer.
// table 0: the hot records (n_steps + 1, the last one padding; hot_steps as for ot_scene_set_hot_steps), 1: the surface
// records (SurfDev; table pointers are the description's host pointers), 2: the step records (StepDev).  `count` and
// `record_bytes` receive the number of records and the size of one; a null buffer asks for those alone.
extern "C" int ot_scene_records_host(const ot_scene_desc* desc, int32_t table, int32_t hot_steps, void* buf, int64_t buf_bytes,
                                     int32_t* count, int32_t* record_bytes) {
    if (!desc || !count || !record_bytes) return fail(OT_ERR_INVALID, "ot_scene_records_host: null argument");
    if (table < 0 || table > 2) return fail(OT_ERR_INVALID, "ot_scene_records_host: table must be 0, 1 or 2");
    if (desc->n_elements < 1 || desc->n_surfaces < 1) return fail(OT_ERR_INVALID, "scene needs at least one element, surface and medium");
    std::vector<SurfDev> surfs(desc->n_surfaces);
    for (int i = 0; i < desc->n_surfaces; i++)
        if (int rc = compile_surface(desc->surfaces[i], surfs[i])) return rc;
    std::vector<StepDev> steps;
    int n_hurb = 0;
    if (int rc = compile_steps(desc, surfs, steps, n_hurb)) return rc;
    std::vector<HotStep> hot;
    compile_hot_steps(steps, surfs, hot_steps != 0, hot);
    const void* src = table == 0 ? (const void*)hot.data() : table == 1 ? (const void*)surfs.data() : (const void*)steps.data();
    const size_t n = table == 0 ? hot.size() : table == 1 ? surfs.size() : steps.size();
    const size_t one = table == 0 ? sizeof(HotStep) : table == 1 ? sizeof(SurfDev) : sizeof(StepDev);
    *count = (int32_t)n;
    *record_bytes = (int32_t)one;
    if (!buf) return OT_OK;
    if (buf_bytes < (int64_t)(n * one)) return fail(OT_ERR_INVALID, "ot_scene_records_host: buffer too small");
    std::memcpy(buf, src, n * one);
    return OT_OK;
}

extern "C" int ot_scene_last_trace_ms(const ot_scene* sc, double* ms) {
    if (!sc || !ms) return fail(OT_ERR_INVALID, "ot_scene_last_trace_ms: null argument");
    if (!sc->ev_valid) return fail(OT_ERR_INVALID, "no timed trace launch on this scene (ot_scene_set_timing)");
    HIP_TRY(hipEventSynchronize(sc->ev1));
    float t = 0.f;
    HIP_TRY(hipEventElapsedTime(&t, sc->ev0, sc->ev1));
    *ms = (double)t;
    return OT_OK;
}

extern "C" int ot_scene_sections(const ot_scene* sc) { return sc ? sc->h.nt : OT_ERR_INVALID; }
