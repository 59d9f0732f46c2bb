// C-ABI, source stage: host-side compilation of the ray sources into their device records (ot_scene.hpp) and of source
// range lists into the generator's argument block (the range cache of a source table).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "ot_generate.hpp"
#include "ot_host.hpp"
#include "ot_trace_kernel.hpp"

// ---------------------------------------------------------------------------------------------------------
// sources (host)
// ---------------------------------------------------------------------------------------------------------
static double gauss_peak1(double x, double mu, double sig) {  // color/srgb.py:447-457
    return 1 / (sig * std::sqrt(2 * M_PI)) * std::exp(-0.5 / (sig * sig) * (x - mu) * (x - mu));
}

static double srgb_primary(int c, double wl) {  // color/srgb.py:469-509
    if (wl < 380. || wl > 780.) return 0.0;
    switch (c) {
        case 0: return 75.1660756583 * 0.951190393 * (gauss_peak1(wl, 639.854491, 30.0) + 0.0500907584 * gauss_peak1(wl, 418.905848, 80.6220465));
        case 1: return 83.4999222966 * 1 * gauss_peak1(wl, 539.13108974, 33.31164968);
        default: return 47.99521746361 * 1.16364585503 * (gauss_peak1(wl, 454.833119, 20.1460206) + 0.184484176 * gauss_peak1(wl, 459.658190, 71.0927568));
    }
}

static double srgb_to_linear(double v) {  // color/srgb.py:30-47
    double a = 0.055, av = std::fabs(v);
    if (av <= 0.04045) return 1 / 12.92 * v;
    double sg = (v > 0) - (v < 0);
    return sg * std::pow(1 / (1 + a) * (av + a), 2.4);
}

// ot_host.hpp: start hints of an inverse-CDF search, ~4 buckets per table node
size_t build_cdf_guide(const double* F, size_t n, double x0, CdfGuide* dst, std::vector<int32_t>& guides) {
    const double x1 = F[n - 1];
    size_t K = 16;
    while (K < 4 * n && K < ((size_t)1 << 22)) K <<= 1;  // ~4 buckets per table node
    dst->K = (int32_t)K;
    dst->x0 = x0;
    dst->scale = (x1 > x0) ? (double)K / (x1 - x0) : 0.0;
    const size_t off = guides.size();
    size_t j = 0;
    for (size_t b = 0; b < K; b++) {
        const double xb = x0 + (double)b / (dst->scale > 0 ? dst->scale : 1.0);
        while (j + 1 < n && F[j + 1] <= xb) j++;
        guides.push_back((int32_t)j);
    }
    return off;
}

// ot_host.hpp: SourceDev::prim_inv, built once per process
const std::vector<double>& srgb_primary_inverse_tables() {
    // The three primaries over wavelengths(5000) (srgb.py:528, 549-551): cumulative trapezoid F_j, and the inverse
    // x(F) the reference interpolates linearly between its nodes (random.py:150-157) sampled at OT_PRIM_M + 1
    // equidistant values of the uniform variable.  Between two samples the device interpolates linearly as well:
    // exact where no node lies between them, elsewhere off by less than the spacing of the reference's own
    // wavelength grid (0.08 nm) except in the few buckets of the far tails (1.5e-5 of the rays each).
    static const std::vector<double> tables = [] {
        std::vector<double> inv(3 * (size_t)(OT_PRIM_M + 1));
        std::vector<double> x(OT_PRIM_N), F(OT_PRIM_N);
        for (int c = 0; c < 3; c++) {
            double prev = 0.0;
            for (int j = 0; j < OT_PRIM_N; j++) {
                x[j] = 380.0 + (780.0 - 380.0) * (double)j / (double)(OT_PRIM_N - 1);
                double f = srgb_primary(c, x[j]);
                F[j] = (j == 0) ? 0.0 : F[j - 1] + (f + prev) / 2;
                prev = f;
            }
            double* o = inv.data() + (size_t)c * (OT_PRIM_M + 1);
            int lo = 0;
            for (int m = 0; m <= OT_PRIM_M; m++) {
                const double X = F[0] + ((double)m / (double)OT_PRIM_M) * (F[OT_PRIM_N - 1] - F[0]);
                while (lo < OT_PRIM_N - 2 && F[lo + 1] <= X) lo++;
                const double dF = F[lo + 1] - F[lo];
                o[m] = (dF > 0) ? x[lo] + (X - F[lo]) / dF * (x[lo + 1] - x[lo]) : x[lo];
            }
        }
        return inv;
    }();
    return tables;
}

extern "C" int ot_sources_create(const ot_source* sources, int32_t n_sources, ot_sources** out) {
    if (!sources || !out || n_sources < 1) return fail(OT_ERR_INVALID, "ot_sources_create: bad argument");
    if (int rc = require_device()) return rc;

    std::vector<SourceDev> devs(n_sources);
    std::vector<double> tabs;                 // all tables, offsets resolved after upload
    std::vector<std::vector<size_t>> offs(n_sources, std::vector<size_t>(9, (size_t)-1));
    auto push_pairs = [&](const double* tab, size_t n) {  // x[n] | F[n]  ->  (F_j, x_j) pairs
        size_t o = tabs.size();
        for (size_t j = 0; j < n; j++) {
            tabs.push_back(tab[n + j]);
            tabs.push_back(tab[j]);
        }
        return o;
    };
    auto push = [&](const double* p, size_t n) {
        size_t o = tabs.size();
        tabs.insert(tabs.end(), p, p + n);
        return o;
    };
    // inverse-CDF start hints (CdfGuide): int32 tables behind the double tables in the same blob
    std::vector<int32_t> guides;
    struct GuideRef { size_t off; CdfGuide* dst; };
    std::vector<GuideRef> grefs;
    auto add_guide = [&](const double* F, size_t n, double x0, CdfGuide* dst) {
        grefs.push_back({build_cdf_guide(F, n, x0, dst, guides), dst});
    };
    struct PickRef { size_t off; int src; };
    std::vector<PickRef> pick_refs;
    bool any_rgb = false;
    for (int i = 0; i < n_sources; i++) {
        const ot_source& s = sources[i];
        SourceDev& d = devs[i];
        std::memset(&d, 0, sizeof(d));
        d.shape = s.shape; d.divergence = s.divergence; d.div_2d = s.div_2d; d.orientation = s.orientation;
        d.polarization = s.polarization; d.spectrum = s.spectrum; d.img_w = s.img_w; d.img_h = s.img_h;
        std::memcpy(d.pos, s.pos, sizeof(d.pos));
        d.r = s.r; d.ri = s.ri; d.dim[0] = s.dim[0]; d.dim[1] = s.dim[1];
        d.ca = (s.angle != 0.0) ? std::cos(s.angle) : 1.0;
        d.sa = (s.angle != 0.0) ? std::sin(s.angle) : 0.0;
        d.div_rad = s.div_angle * (M_PI / 180.0);
        d.div_sin = std::sin(d.div_rad);
        d.div_axis = s.div_axis_angle * (M_PI / 180.0);
        std::memcpy(d.s, s.s, sizeof(d.s));
        std::memcpy(d.conv_pos, s.conv_pos, sizeof(d.conv_pos));
        if (s.orientation == OT_OR_CONSTANT || (s.orientation == OT_OR_CONVERGING && s.shape == OT_SRC_POINT)) {
            if (s.orientation == OT_OR_CONVERGING) {  // misc.normalize(conv_pos - p) with p = pos (ray_source.py:269)
                const double dx = s.conv_pos[0] - s.pos[0], dy = s.conv_pos[1] - s.pos[1], dz = s.conv_pos[2] - s.pos[2];
                const double l = std::sqrt(dx * dx + dy * dy + dz * dz);
                d.s[0] = dx / l; d.s[1] = dy / l; d.s[2] = dz / l;
            }
            const double fa = 1.0 / std::sqrt(1 - d.s[0] * d.s[0]);  // ray_source.py:339-341
            d.fy[0] = 0.0; d.fy[1] = -d.s[2] * fa; d.fy[2] = d.s[1] * fa;
            d.fx[0] = d.s[1] * d.fy[2] - d.s[2] * d.fy[1];
            d.fx[1] = d.s[2] * d.fy[0] - d.s[0] * d.fy[2];
            d.fx[2] = d.s[0] * d.fy[1] - d.s[1] * d.fy[0];
            d.frame_uniform = 1;
        }
        d.pol_angle = s.pol_angle;
        d.pol_cos = std::cos(s.pol_angle);
        d.pol_sin = std::sin(s.pol_angle);
        d.axis_cos = std::cos(d.div_axis);
        d.axis_sin = std::sin(d.div_axis);
        d.px_w = (s.img_w > 0) ? s.dim[0] / (double)s.img_w : 0.0;  // ray_source.py:252-253
        d.px_h = (s.img_h > 0) ? s.dim[1] / (double)s.img_h : 0.0;
        d.inv_img_w = (s.img_w > 0) ? 1.0 / (double)s.img_w : 0.0;
        d.wl = s.wl; d.wl0 = s.wl0; d.wl1 = s.wl1; d.mu = s.mu; d.sig = s.sig;
        d.power = s.power;
        if (s.spectrum == OT_SPEC_GAUSSIAN) {  // light_spectrum.py:117-118
            d.gauss_xl = (1 + std::erf((s.wl0 - s.mu) / (std::sqrt(2.0) * s.sig))) / 2;
            d.gauss_xr = (1 + std::erf((s.wl1 - s.mu) / (std::sqrt(2.0) * s.sig))) / 2;
        }
        if (s.shape < OT_SRC_POINT || s.shape > OT_SRC_IMAGE_GRAY) return fail(OT_ERR_INVALID, "source: unknown shape");
        if (s.orientation < OT_OR_CONSTANT || s.orientation > OT_OR_ARRAY) return fail(OT_ERR_INVALID, "source: unknown orientation");
        if (s.orientation == OT_OR_ARRAY && s.s_or) {
            if (s.n_or < 1) return fail(OT_ERR_INVALID, "source: orientation array without a length");
            d.s_or = s.s_or;
            d.n_or = s.n_or;
        }
        bool needs_spec = s.shape != OT_SRC_IMAGE_RGB && (s.spectrum == OT_SPEC_LINES || s.spectrum == OT_SPEC_TABLE);
        if (needs_spec) {
            if (!s.spec_tab || s.n_spec < 1) return fail(OT_ERR_INVALID, "source: spectrum table missing");
            offs[i][0] = push(s.spec_tab, 2 * (size_t)s.n_spec);
            d.n_spec = s.n_spec;
            const double* F = s.spec_tab + s.n_spec;
            add_guide(F, (size_t)s.n_spec, s.spectrum == OT_SPEC_LINES ? 0.0 : F[0], &d.g_spec);
            if (s.spectrum != OT_SPEC_LINES) offs[i][6] = push_pairs(s.spec_tab, (size_t)s.n_spec);
        }
        if (s.polarization == OT_POL_LIST || s.polarization == OT_POL_TABLE) {
            if (!s.pol_tab || s.n_pol < 1) return fail(OT_ERR_INVALID, "source: polarisation table missing");
            offs[i][1] = push(s.pol_tab, 2 * (size_t)s.n_pol);
            d.n_pol = s.n_pol;
            const double* F = s.pol_tab + s.n_pol;
            add_guide(F, (size_t)s.n_pol, s.polarization == OT_POL_LIST ? 0.0 : F[0], &d.g_pol);
            if (s.polarization != OT_POL_LIST) offs[i][7] = push_pairs(s.pol_tab, (size_t)s.n_pol);
        }
        if (s.divergence == OT_DIV_TABLE) {
            if (!s.div_tab || s.n_div < 2) return fail(OT_ERR_INVALID, "source: divergence table missing");
            offs[i][2] = push(s.div_tab, 2 * (size_t)s.n_div);
            d.n_div = s.n_div;
            add_guide(s.div_tab + s.n_div, (size_t)s.n_div, s.div_tab[s.n_div], &d.g_div);
            offs[i][8] = push_pairs(s.div_tab, (size_t)s.n_div);
        }
        if (s.shape == OT_SRC_IMAGE_RGB || s.shape == OT_SRC_IMAGE_GRAY) {
            size_t npx = (size_t)s.img_w * (size_t)s.img_h;
            if (!s.img_pdf || npx < 1) return fail(OT_ERR_INVALID, "image source: pixel pdf missing");
            if (s.shape == OT_SRC_IMAGE_RGB && !s.img_rgb) return fail(OT_ERR_INVALID, "RGB image source: pixel colours missing");
            std::vector<double> rec(4 * npx, 0.0);
            double acc = 0.0;  // np.cumsum of the pixel pdf (random.py:133 on f_ = f[f > 0]; zero-weight pixels
            const double fr = 0.885651229244, fb = 0.775993481741;  // srgb.py:24-26
            for (size_t j = 0; j < npx; j++) {  // keep the running sum and can never be selected by "next")
                acc += s.img_pdf[j];
                rec[4 * j] = acc;
                if (s.shape == OT_SRC_IMAGE_RGB) {  // color.random_wavelengths_from_srgb srgb.py:522-541
                    double r = srgb_to_linear(s.img_rgb[3 * j]) * fr;
                    double g = srgb_to_linear(s.img_rgb[3 * j + 1]);
                    double b = srgb_to_linear(s.img_rgb[3 * j + 2]) * fb;
                    double c0 = r, c1 = r + g, c2 = r + g + b;
                    double den = (c2 != 0.0) ? c2 : 1.0;
                    rec[4 * j + 1] = c0 / den;
                    rec[4 * j + 2] = c1 / den;
                }
            }
            if (tabs.size() & 1) tabs.push_back(0.0);  // PixRec is read with 16-byte loads
            offs[i][3] = push(rec.data(), rec.size());
            // bucket table of the pixel pick: K ~ 4 buckets per pixel; pick_lo[b] = pixels whose own bucket lies before b.
            // The bucket of a value is the DEVICE's expression (pixel_bucket, monotone in X), so for X in bucket b every
            // pixel before pick_lo[b] has F < X and every pixel from pick_lo[b + 1] on has F > X.
            size_t K = 16;
            while (K < 4 * npx && K < ((size_t)1 << 22)) K <<= 1;
            d.pick_K = (int32_t)K;
            d.pix_total = acc;
            d.pick_scale = (acc > 0.0) ? (double)K / acc : 0.0;
            pick_refs.push_back({guides.size(), i});
            size_t j = 0;
            for (size_t b = 0; b <= K; b++) {
                while (j < npx && (size_t)pixel_bucket(rec[4 * j], d.pick_scale, (int)K) < b) j++;
                guides.push_back((int32_t)j);
            }
            any_rgb = any_rgb || s.shape == OT_SRC_IMAGE_RGB;
        }
    }
    size_t prim_off = (size_t)-1;
    if (any_rgb) {
        const std::vector<double>& inv = srgb_primary_inverse_tables();
        prim_off = push(inv.data(), inv.size());
    }

    size_t o_tab = align_up(sizeof(SourceDev) * n_sources);
    size_t o_guide = align_up(o_tab + sizeof(double) * (tabs.size() + 1));
    size_t total = align_up(o_guide + sizeof(int32_t) * (guides.size() + 1));
    char* blob = nullptr;
    HIP_TRY(hipMalloc((void**)&blob, total));
    const double* dtab = (const double*)(blob + o_tab);
    for (const GuideRef& r : grefs) r.dst->g = (const int32_t*)(blob + o_guide) + r.off;
    for (const PickRef& r : pick_refs) devs[r.src].pick_lo = (const int32_t*)(blob + o_guide) + r.off;
    for (int i = 0; i < n_sources; i++) {
        SourceDev& d = devs[i];
        if (offs[i][0] != (size_t)-1) d.spec_tab = dtab + offs[i][0];
        if (offs[i][1] != (size_t)-1) d.pol_tab = dtab + offs[i][1];
        if (offs[i][2] != (size_t)-1) d.div_tab = dtab + offs[i][2];
        if (offs[i][3] != (size_t)-1) d.pix_rec = dtab + offs[i][3];
        if (prim_off != (size_t)-1) d.prim_inv = dtab + prim_off;
        if (offs[i][6] != (size_t)-1) d.spec_pairs = dtab + offs[i][6];
        if (offs[i][7] != (size_t)-1) d.pol_pairs = dtab + offs[i][7];
        if (offs[i][8] != (size_t)-1) d.div_pairs = dtab + offs[i][8];
    }
    std::vector<char> host(total, 0);
    std::memcpy(host.data(), devs.data(), sizeof(SourceDev) * n_sources);
    if (!tabs.empty()) std::memcpy(host.data() + o_tab, tabs.data(), sizeof(double) * tabs.size());
    if (!guides.empty()) std::memcpy(host.data() + o_guide, guides.data(), sizeof(int32_t) * guides.size());
    hipError_t e = hipMemcpy(blob, host.data(), total, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(blob);
        return fail(OT_ERR_HIP, std::string("source upload: ") + hipGetErrorString(e));
    }
    ot_sources* so = new ot_sources;
    so->d = (SourceDev*)blob;
    so->n = n_sources;
    so->blob = blob;
    so->has_image = false;
    for (int i = 0; i < n_sources; i++) so->has_image = so->has_image || sources[i].shape >= OT_SRC_IMAGE_RGB;
    so->n_or = new int64_t[n_sources];
    so->power = new double[n_sources];
    for (int i = 0; i < n_sources; i++) {
        so->n_or[i] = devs[i].s_or ? devs[i].n_or : -1;
        so->power[i] = devs[i].power;
    }
    (void)hipGetDevice(&so->device);
    *out = so;
    return OT_OK;
}

// per-range constants of the stratified samplers: floor(sqrt(count)), 1 / count and 1 / floor(sqrt(count))
static void range_constants(uint64_t cnt, uint32_t& n2, double& inv_n, double& inv_n2) {
    n2 = (uint32_t)std::sqrt((double)cnt);
    while ((uint64_t)n2 * n2 > cnt) n2--;
    while ((uint64_t)(n2 + 1) * (n2 + 1) <= cnt) n2++;
    inv_n = cnt ? 1.0 / (double)cnt : 0.0;
    inv_n2 = n2 ? 1.0 / (double)n2 : 0.0;
}

// ot_host.hpp: the argument block of the sampler kernels (ot_sample_api.hip) -- no source table behind the ranges, no cache
int sampler_ranges(const char* who, const ot_source_range* ranges, int32_t n_ranges, int64_t N, RangeArgs* out) {
    const std::string w(who);
    if (!ranges || n_ranges < 1) return fail(OT_ERR_INVALID, w + ": at least one range is needed");
    if (n_ranges > OT_MAX_RANGES) return fail(OT_ERR_UNSUPPORTED, w + ": more than 64 ranges");
    RangeArgs& rg = *out;
    rg.ext = nullptr;
    rg.n = n_ranges;
    int64_t covered = 0;
    for (int q = 0; q < n_ranges; q++) {
        if (ranges[q].first < 0 || ranges[q].count < 0) return fail(OT_ERR_INVALID, w + ": negative range");
        if (ranges[q].count > 0xffffffffll) return fail(OT_ERR_UNSUPPORTED, w + ": more than 2^32 - 1 samples in one range");
        if (ranges[q].first != covered) return fail(OT_ERR_INVALID, w + ": the ranges must cover all samples once, in order");
        range_constants((uint64_t)ranges[q].count, rg.n2[q], rg.inv_n[q], rg.inv_n2[q]);
        rg.w[q] = 0.0f;
        rg.source[q] = 0;
        rg.first[q] = ranges[q].first;
        rg.count[q] = ranges[q].count;
        covered += ranges[q].count;
    }
    if (covered != N) return fail(OT_ERR_INVALID, w + ": the ranges must cover all samples once, in order");
    return OT_OK;
}

// What make_ranges derived from the last range list of a source table.  Chunked rendering and repeated traces
// pass the same list again and again: the argument block is reused, and for long lists so is the device copy of
// the records -- no allocation, no upload and no stream synchronisation on the launch path.
struct RangeCache {
    std::vector<ot_source_range> key;
    int64_t N = -1;
    RangeArgs rg;
    RangeRec* ext = nullptr;  // device records (n > OT_MAX_RANGES), owned by the cache
};

void drop_range_cache(ot_sources* s) {
    if (!s->rcache) return;
    if (s->rcache->ext) (void)hipFree(s->rcache->ext);  // hipFree waits for work that may still read the records
    delete s->rcache;
    s->rcache = nullptr;
}

int make_ranges(const ot_source_range* ranges, int32_t n_ranges, const ot_sources* src_c, int64_t N, const RangeArgs** out) {
    ot_sources* src = const_cast<ot_sources*>(src_c);
    if (!ranges || n_ranges < 1) return fail(OT_ERR_INVALID, "at least one source range is needed");
    if (RangeCache* c = src->rcache) {
        if (c->N == N && (int32_t)c->key.size() == n_ranges &&
            std::memcmp(c->key.data(), ranges, sizeof(ot_source_range) * (size_t)n_ranges) == 0) {
            *out = &c->rg;
            return OT_OK;
        }
    }
    RangeArgs rg;
    rg.ext = nullptr;
    rg.n = n_ranges;
    const bool big = n_ranges > OT_MAX_RANGES;
    std::vector<RangeRec> recs(big ? n_ranges : 0);
    // the kernel finds a wave's range by bisection: records sorted by their first ray, gap-free (empty ranges first
    // among equal starts)
    std::vector<int> order(n_ranges);
    for (int k = 0; k < n_ranges; k++) order[k] = k;
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) {
        return ranges[a].first != ranges[b].first ? ranges[a].first < ranges[b].first : ranges[a].count < ranges[b].count;
    });
    int64_t covered = 0;
    for (int q = 0; q < n_ranges; q++) {
        const int k = order[q];
        if (ranges[k].source < 0 || ranges[k].source >= src->n) return fail(OT_ERR_INVALID, "range: source out of range");
        if (ranges[k].first < 0 || ranges[k].count < 0 || ranges[k].first + ranges[k].count > N)
            return fail(OT_ERR_INVALID, "range outside the ray storage");
        if (ranges[k].count > 0xffffffffll) return fail(OT_ERR_UNSUPPORTED, "more than 2^32 rays in one source range");
        if (src->n_or[ranges[k].source] >= 0 && src->n_or[ranges[k].source] != ranges[k].count)
            return fail(OT_ERR_INVALID, "range: ray count differs from the length of the source's orientation array");
        if (ranges[k].first != covered) return fail(OT_ERR_INVALID, "source ranges must cover all N rays exactly once");
        const uint64_t cnt = (uint64_t)ranges[k].count;
        uint32_t n2;
        double inv_n, inv_n2;
        range_constants(cnt, n2, inv_n, inv_n2);
        const float w = (float)(ranges[k].ray_power > 0 ? ranges[k].ray_power
                                                        : (cnt ? src->power[ranges[k].source] / (double)cnt : 0.0));
        if (big) {
            recs[q] = {ranges[k].first, ranges[k].count, ranges[k].source, n2, inv_n, inv_n2, w};
        } else {
            rg.w[q] = w;
            rg.source[q] = ranges[k].source;
            rg.first[q] = ranges[k].first;
            rg.count[q] = ranges[k].count;
            rg.n2[q] = n2;
            rg.inv_n[q] = inv_n;
            rg.inv_n2[q] = inv_n2;
        }
        covered += ranges[k].count;
    }
    // (covered <= N by the checks above; rays behind the last range -- the padding of a storage whose plane stride N is
    // larger than its ray count -- are not generated and not traced)
    RangeRec* d = nullptr;
    if (big) {
        HIP_TRY(hipMalloc((void**)&d, sizeof(RangeRec) * recs.size()));
        hipError_t e = hipMemcpy(d, recs.data(), sizeof(RangeRec) * recs.size(), hipMemcpyHostToDevice);
        if (e != hipSuccess) {
            (void)hipFree(d);
            return fail(OT_ERR_HIP, std::string("range upload: ") + hipGetErrorString(e));
        }
        rg.ext = d;
    }
    drop_range_cache(src);  // the previous list (its device records are no longer needed by any new launch)
    RangeCache* c = new RangeCache;
    c->key.assign(ranges, ranges + n_ranges);
    c->N = N;
    c->rg = rg;
    c->ext = d;
    src->rcache = c;
    *out = &c->rg;
    return OT_OK;
}

extern "C" void ot_sources_destroy(ot_sources* s) {
    if (!s) return;
    drop_range_cache(s);
    (void)hipFree(s->blob);
    delete[] s->n_or;
    delete[] s->power;
    delete s;
}
