/*
 * optrace_amd.h -- C-ABI of the MI355X-native sequential ray-tracing core.
 *
 * The upstream reference (drocheam/optrace, pure NumPy) has no FFI boundary of its own
 * (SURVEY.md section 8b); the drop-in boundary is the Python surface of
 * optrace/tracer/__init__.py:3-63.  This header is the C-ABI that our Python mirror of that
 * surface (package optrace_amd) binds with ctypes.  Every entry point names the reference
 * function(s) it replaces as file:line relative to the reference checkout.
 *
 * Conventions
 *   - All ray buffers are DEVICE pointers (HIP), caller-owned, struct-of-arrays.  Multi-component
 *     quantities use the reference's Fortran-ordered layout (ray_storage.py:80-90): element
 *     (ray r, section i, component c) of an (N, nt, 3) array lives at  r + N*(i + nt*c).
 *   - dtypes follow ray_storage.py:77-90: positions/directions/refractive indices f64,
 *     weights / wavelengths / polarisation f32.
 *   - `stream` is a hipStream_t passed as void* (NULL = default stream).  Calls are asynchronous
 *     with respect to the host unless stated otherwise.
 *   - Return value: 0 on success, negative OT_ERR_* otherwise; ot_last_error() gives the text.
 *   - Nothing here allocates or frees caller buffers.  Handles (ot_scene) own small device tables only.
 */
#ifndef OPTRACE_AMD_H
#define OPTRACE_AMD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OT_ABI_VERSION 9

/* ---- status codes -------------------------------------------------------------------------- */
#define OT_OK 0
#define OT_ERR_INVALID (-1)     /* bad argument / descriptor                                     */
#define OT_ERR_HIP (-2)         /* HIP runtime error (text in ot_last_error)                     */
#define OT_ERR_UNSUPPORTED (-3) /* feature not representable on the device                       */
#define OT_ERR_NO_DEVICE (-4)   /* no HIP device available                                       */

/* ---- numeric contract (reference class constants) ------------------------------------------ */
#define OT_C_EPS 1e-6        /* Surface.C_EPS   surface.py:17        */
#define OT_N_EPS_SURF 1e-10  /* Surface.N_EPS   surface.py:20        */
#define OT_N_EPS_TRACE 1e-11 /* Raytracer.N_EPS raytracer.py:30      */
#define OT_MAX_HIT_ITER 200  /* regula-falsi timeout surface.py:403  */

/* counter rows, Raytracer.INFOS raytracer.py:43-48 */
#define OT_INFO_ABSORB_MISSING 0
#define OT_INFO_TIR 1
#define OT_INFO_ILL_COND 2
#define OT_INFO_OUTLINE_INTERSECTION 3
#define OT_INFO_HURB_NEG_DIR 4
#define OT_N_INFOS 5

/* ---- surfaces (optrace/tracer/geometry/surface/) -------------------------------------------- */
#define OT_SURF_CIRCLE 0  /* CircularSurface    circular_surface.py:9     flat disc               */
#define OT_SURF_RING 1    /* RingSurface        ring_surface.py:10        flat annulus            */
#define OT_SURF_RECT 2    /* RectangularSurface rectangular_surface.py:10 flat, rotated by angle  */
#define OT_SURF_SLIT 3    /* SlitSurface        slit_surface.py:12        rect minus inner rect   */
#define OT_SURF_CONIC 4   /* ConicSurface / SphericalSurface (k = 0) conic_surface.py:10          */
#define OT_SURF_ASPHERE 5 /* AsphericSurface    aspheric_surface.py:9     conic + even polynomial */
#define OT_SURF_TILTED 6  /* TiltedSurface      tilted_surface.py:10      tilted plane inside a disc */
#define OT_SURF_DATA1D 7  /* DataSurface1D / FunctionSurface1D  data_surface_1d.py:6, function_surface_1d.py:8:
                             radial profile z(r) as a FITPACK B-spline (knots + coefficients in `tab`)      */
#define OT_SURF_DATA2D 8  /* DataSurface2D / FunctionSurface2D  data_surface_2d.py:10, function_surface_2d.py:12:
                             z(x, y) as a tensor-product FITPACK B-spline                                   */

#define OT_MAX_ASPH 12 /* even-order coefficients a2 .. a24 */
#define OT_MAX_LINES 8 /* discrete wavelengths tabulated per scene */

typedef struct ot_surface {
    int32_t kind;   /* OT_SURF_*                                                                 */
    int32_t ncoeff; /* ASPHERE: number of even polynomial coefficients                           */
    double pos[3];  /* centre position                                                           */
    double r;       /* outer radius (CIRCLE/RING/CONIC/ASPHERE); RECT/SLIT keep the reference's 1 */
    double ri;      /* RING: inner radius                                                        */
    double dim[2];  /* RECT/SLIT: outer side lengths                                             */
    double dimi[2]; /* SLIT: inner (open) side lengths                                           */
    double angle;   /* RECT/SLIT: rotation about z [rad] (RectangularSurface._angle)             */
    double R;       /* CONIC/ASPHERE: vertex radius of curvature                                 */
    double k;       /* CONIC/ASPHERE: conic constant                                             */
    double z_min;   /* absolute z range of the surface (Surface.z_min / z_max)                   */
    double z_max;
    double coeff[OT_MAX_ASPH]; /* ASPHERE: a2, a4, ... [mm^-1, mm^-3, ...] (more: OT_SURF_FLAG_ASPH_TABLE) */
    double normal[3]; /* TILTED: unit normal with normal[2] > 0 (TiltedSurface.normal)            */
    double sign;      /* DATA1D/2D: +1, or -1 after flip() (DataSurface2D._sign)                   */
    double offset;    /* DATA1D/2D: spline value at the centre, removed from every value (._offset) */
    /* DATA1D/2D: spline tables (host pointer, caller-owned, copied by the callee).  k = OT_SPL_K = 4.
     *   DATA1D: t[nknots] | c[nknots] | dc[nknots]: knots, B-spline coefficients (padded with zeros to nknots,
     *           as FITPACK/SciPy store them) and the coefficients of the first derivative (order k-1 on the
     *           knots t[1..nknots-2]).  scipy InterpolatedUnivariateSpline(k=4) of the mirrored profile.
     *   DATA2D: t[nknots] (same knots in x and y) | c[(nknots-5)^2] | cx[(nknots-6)(nknots-5)] |
     *           cy[(nknots-5)(nknots-6)]: RectBivariateSpline(kx=ky=4) coefficients, row-major with y
     *           fastest (FITPACK order), and those of d/dx and d/dy.  `angle` = DataSurface2D._angle.     */
    const double* tab;
    int64_t tab_len;
    int32_t nknots;
    int32_t flags;    /* OT_SURF_FLAG_* */
} ot_surface;
/* FunctionSurface2D.normals with a user deriv_func evaluates it at the UNROTATED relative coordinates and only
 * rotates the resulting gradient (function_surface_2d.py:229-244); without deriv_func normals come from central
 * differences of the (rotated) surface.  The flag selects the first behaviour so results match the reference. */
#define OT_SURF_FLAG_DERIV_UNROTATED 1
/* FunctionSurface mask_func (function_surface_2d.py:158-191): a Python callable cannot run per ray, so the mask travels
 * as a bitmap sampled at cell centres in the function's own frame (before rotate() and flip(), like the spline).
 * With this flag `tab` continues behind the spline tables with
 *     n (as a double) | ceil(cells / 64) doubles whose bytes are little-endian uint32 words, bit (i & 31) of word i >> 5
 * DATA1D: cells = n over the radius [0, r], cell i covers [i, i + 1) * r / n;
 * DATA2D: cells = n * n over [-r, r]^2, index iy * n + ix, cell (ix, iy) covers [-r + ix h, -r + (ix + 1) h) with
 *         h = 2 r / n in x and likewise in y.
 * A position is on the surface if it is inside r (+ N_EPS) and its cell's bit is set; positions closer to the mask's
 * edge than one cell can therefore differ from the callable.  tab_len counts these doubles too. */
#define OT_SURF_FLAG_MASK_TABLE 2
/* ASPHERE with more than OT_MAX_ASPH coefficients (the reference sets no upper bound, aspheric_surface.py:23): with
 * this flag `tab` holds all of them,
 *     a2 | a4 | ... | a_(2 ncoeff)        tab_len = ncoeff doubles,
 * and coeff[] is ignored (any ncoeff >= 1 may travel this way).  Host pointer, caller-owned, copied by the callee like
 * the spline tables.  Without the flag an asphere is the call it always was: 1 <= ncoeff <= OT_MAX_ASPH coefficients in
 * coeff[], `tab` unused.  ncoeff above OT_MAX_ASPH without the flag, the flag with a NULL `tab` or with
 * tab_len != ncoeff are refused with a negative status; nothing is read through `tab` then. */
#define OT_SURF_FLAG_ASPH_TABLE 4
#define OT_SPL_K 4

/* ---- media: RefractionIndex.__call__ refraction_index.py:62-169 ----------------------------- */
#define OT_N_CONSTANT 0    /* c[0] = n                                                            */
#define OT_N_ABBE 1        /* c = {A, B, d}: n = A + B/(wl2 - d)  (A, B solved on the host exactly
                              as refraction_index.py:85-100 does, including its float32 line table) */
#define OT_N_CAUCHY 2      /* :105 */
#define OT_N_CONRADY 3     /* :101 */
#define OT_N_SELLMEIER1 4  /* :108 */
#define OT_N_SELLMEIER2 5  /* :111 */
#define OT_N_SELLMEIER3 6  /* :114 */
#define OT_N_SELLMEIER4 7  /* :117 */
#define OT_N_SELLMEIER5 8  /* :120 */
#define OT_N_SCHOTT 9      /* :124 */
#define OT_N_HERZBERGER 10 /* :127 */
#define OT_N_HOO1 11       /* "Handbook of Optics 1" :131 */
#define OT_N_HOO2 12       /* "Handbook of Optics 2" :134 */
#define OT_N_EXTENDED 13   /* :137 */
#define OT_N_EXTENDED2 14  /* :141 */
#define OT_N_EXTENDED3 15  /* :145 */
#define OT_N_DATA 16       /* np.interp over an equally spaced table (spectrum.py:103-106), table
                              = tab_len (wl, n) pairs at table_pool[tab_off ...]: first the tab_len
                              wavelengths, then the tab_len values.  Also carries host-tabulated
                              "Function" media.                                                     */
#define OT_N_LINES 17      /* exact per-line values for discrete spectra: n = value[j] where
                              wl == line[j] (same table layout as DATA); used for "Function" media
                              under Monochromatic / Lines sources                                   */

typedef struct ot_medium {
    int32_t model; /* OT_N_* */
    int32_t tab_len;
    int64_t tab_off;
    double c[10];
} ot_medium;

/* ---- filters: TransmissionSpectrum.__call__ transmission_spectrum.py:73-84 -------------------- */
#define OT_T_CONSTANT 0  /* spectrum.py:99   */
#define OT_T_DATA 1      /* spectrum.py:103  np.interp, 0 outside                                  */
#define OT_T_RECTANGLE 2 /* spectrum.py:108  */
#define OT_T_GAUSSIAN 3  /* spectrum.py:113  evaluated in float32 like the reference does for f32 wl */
#define OT_T_LINES 4     /* host-tabulated per-line values ("Function" spectra, discrete sources)   */

typedef struct ot_filter {
    int32_t type;    /* OT_T_* */
    int32_t inverse; /* TransmissionSpectrum.inverse: T -> 1 - T */
    int32_t tab_len;
    int32_t _pad;
    int64_t tab_off;
    double val, wl0, wl1, mu, sig;
} ot_filter;

/* ---- tracing elements: Raytracer.__tracing_elements raytracer.py:492-508 ----------------------- */
#define OT_EL_LENS 0       /* Lens        raytracer.py:314-370 (two refracting surfaces)            */
#define OT_EL_IDEAL_LENS 1 /* IdealLens   raytracer.py:360-363, 720-759                             */
#define OT_EL_FILTER 2     /* Filter      raytracer.py:372-391                                      */
#define OT_EL_APERTURE 3   /* Aperture    raytracer.py:372-391 (the invisible end aperture as well) */

typedef struct ot_element {
    int32_t kind;    /* OT_EL_*                                                                    */
    int32_t front;   /* surface index                                                              */
    int32_t back;    /* surface index (LENS) or -1                                                 */
    int32_t n_lens;  /* LENS: medium index of the lens material                                    */
    int32_t n_after; /* LENS / IDEAL_LENS: medium index behind the lens (n2 or n0, raytracer.py:326) */
    int32_t filter;  /* FILTER: filter index                                                       */
    int32_t hurb;    /* APERTURE: 1 = apply HURB edge bending here (raytracer.py:385)              */
    int32_t _pad;
    double D;        /* IDEAL_LENS: optical power [dpt]                                            */
} ot_element;

typedef struct ot_scene_desc {
    double outline[6]; /* Raytracer.outline [x0,x1,y0,y1,z0,z1]                                      */
    int32_t n_surfaces, n_elements, n_media, n_filters;
    const ot_surface* surfaces;
    const ot_element* elements; /* z-sorted; the last one must be the end aperture (raytracer.py:501) */
    const ot_medium* media;
    const ot_filter* filters;
    const double* table_pool; /* shared table storage for DATA/LINES media and filters               */
    int64_t table_pool_len;
    int32_t n0;       /* ambient medium index (Raytracer.n0)                                         */
    int32_t no_pol;   /* Raytracer.no_pol                                                            */
    int32_t use_hurb; /* Raytracer.use_hurb                                                          */
    int32_t n_lines;  /* > 0: every source has a discrete spectrum; `lines` = the distinct wavelengths       */
    double hurb_factor; /* Raytracer.HURB_FACTOR raytracer.py:33                                     */
    const double* lines; /* n_lines float32 wavelength values (as doubles) or NULL.  With 1..OT_MAX_LINES lines
                            ot_generate_and_trace tabulates n(lambda), n1/n2 and filter transmissions per line
                            once on the host and the kernel reads them from LDS instead of evaluating them per ray */
} ot_scene_desc;

typedef struct ot_scene ot_scene; /* opaque: device copy of the tables */

/* ---- ray sources: RaySource.create_rays ray_source.py:204-437 --------------------------------- */
#define OT_SRC_POINT 0  /* Point  point.py:62                                                       */
#define OT_SRC_LINE 1   /* Line   line.py:81                                                        */
#define OT_SRC_CIRCLE 2 /* CircularSurface.random_positions circular_surface.py:33                  */
#define OT_SRC_RING 3   /* RingSurface.random_positions     ring_surface.py:135                     */
#define OT_SRC_RECT 4   /* RectangularSurface.random_positions rectangular_surface.py:142           */
#define OT_SRC_IMAGE_RGB 5  /* RGBImage: pixel pdf + sRGB primaries ray_source.py:233-258           */
#define OT_SRC_IMAGE_GRAY 6 /* GrayscaleImage: pixel pdf, spectrum from `spectrum`                  */

#define OT_DIV_NONE 0
#define OT_DIV_LAMBERTIAN 1 /* ray_source.py:300-309 */
#define OT_DIV_ISOTROPIC 2  /* ray_source.py:311-318 */
#define OT_DIV_TABLE 3      /* "Function": host-tabulated pdf(theta), ray_source.py:320-333           */

#define OT_OR_CONSTANT 0   /* ray_source.py:266 */
#define OT_OR_CONVERGING 1 /* ray_source.py:269 */
#define OT_OR_ARRAY 2      /* "Function" ray_source.py:272-274: base orientations evaluated by the caller  */

#define OT_POL_CONSTANT 0 /* also "x" (0) and "y" (pi/2), ray_source.py:366-376 */
#define OT_POL_UNIFORM 1  /* :378 */
#define OT_POL_LIST 2     /* "List" and "xy": discrete angles with probabilities :372, :381-385       */
#define OT_POL_TABLE 3    /* "Function": host-tabulated pdf(angle) :387-392                          */

#define OT_SPEC_MONO 0     /* light_spectrum.py:91  */
#define OT_SPEC_UNIFORM 1  /* Constant / Rectangle: uniform in [wl0, wl1] :94-98                     */
#define OT_SPEC_LINES 2    /* :100-103 discrete inverse CDF                                          */
#define OT_SPEC_GAUSSIAN 3 /* :110-122 truncated normal via erfinv                                   */
#define OT_SPEC_TABLE 4    /* Data / Blackbody / Function / Histogram: linear inverse CDF :105,:129   */

typedef struct ot_source {
    int32_t shape;       /* OT_SRC_*                                                                */
    int32_t divergence;  /* OT_DIV_*                                                                */
    int32_t div_2d;      /* RaySource.div_2d                                                        */
    int32_t orientation; /* OT_OR_*                                                                 */
    int32_t polarization; /* OT_POL_*                                                               */
    int32_t spectrum;    /* OT_SPEC_*                                                               */
    int32_t img_w, img_h; /* IMAGE_*: pixel counts                                                  */
    double pos[3];
    double r, ri;        /* LINE: half length r; CIRCLE/RING radii                                  */
    double dim[2];       /* RECT / IMAGE side lengths                                               */
    double angle;        /* RECT rotation [rad]; LINE angle [rad]                                   */
    double div_angle;    /* [deg]                                                                   */
    double div_axis_angle; /* [deg]                                                                 */
    double s[3];         /* unit orientation (CONSTANT)                                             */
    double conv_pos[3];  /* CONVERGING                                                              */
    double pol_angle;    /* [rad] for POL_CONSTANT                                                  */
    double wl, wl0, wl1, mu, sig;
    double power;        /* power of the source; a range without ray_power gives each of its rays
                          * power / count (ray_storage.py:160, ray_source.py:220)                   */
    /* tables (device copies made by ot_sources_create); layouts:
     *   spec_tab : LINES: n_spec lines (as the reference's float32 values upcast) then n_spec weights;
     *              TABLE: n_spec wavelengths then n_spec pdf values
     *   pol_tab  : LIST: n_pol angles [rad] then n_pol probabilities; TABLE: n_pol angles then pdf
     *   div_tab  : TABLE: n_div thetas [rad] then n_div pdf values
     *   img_pdf  : IMAGE_*: img_w*img_h relative pixel powers (RaySource._pIf)
     *   img_rgb  : IMAGE_RGB: img_w*img_h*3 sRGB values in [0,1], row-major (y, x, c)              */
    const double* spec_tab; int64_t n_spec;
    const double* pol_tab;  int64_t n_pol;
    const double* div_tab;  int64_t n_div;
    const double* img_pdf;
    const double* img_rgb;
    /* OR_ARRAY: DEVICE pointer (caller-owned, NOT copied; must stay valid while the table is used) to the base
     * orientation of each ray of this source, x[n_or] | y[n_or] | z[n_or]; every range of this source must
     * hold exactly n_or rays, ray j of the range reads element j.  With a NULL pointer the source emits along
     * `s`: start positions do not depend on the orientation, so the caller runs ot_rays_generate once with NULL,
     * evaluates its orientation function at the positions, and generates again with the result.             */
    const double* s_or; int64_t n_or;
} ot_source;

/* A contiguous block of rays generated from one source: rays [first, first+count) of the launch (the blocks of a
 * launch follow each other without gaps from ray 0 on; slots of the storage behind the last block stay unused).  A block
 * is one stratification domain, as one thread's share is in the reference (ray_storage.py:147-166); a source
 * may be cut into several.  Blocks whose count is a power of two are the cheapest to generate (their stratum
 * permutation needs no rejection step). */
typedef struct ot_source_range {
    int32_t source;  /* index into the source table                                                 */
    int32_t _pad;
    int64_t first;   /* first ray index inside this launch                                          */
    int64_t count;   /* number of rays (stratification domain, ray_storage.py:160-163)              */
    double ray_power; /* power of each ray of the block (`power/N` ray_source.py:220, stored f32);
                       * <= 0: the source's `power` / count                                         */
} ot_source_range;

typedef struct ot_sources ot_sources; /* opaque: device copy of sources + tables */

/* ---- ray storage: RayStorage ray_storage.py:35-90 --------------------------------------------- */
/* N is the number of ray slots AND the plane stride: element (ray r, section i, component c) of p lives at
 * r + N * (i + nt * c).  A caller may make N larger than its ray count so that every plane starts on a 128-byte line
 * (a multiple of 32 rays; with planes off the lines the tracing kernel runs 30-50 % slower): the source ranges of
 * ot_generate_and_trace / ot_rays_generate then cover the first rays only and the slots behind are neither generated
 * nor traced; ot_trace (rays handed in) walks all N slots, so the unused ones must hold weight 0 and a finite
 * direction; every detector / spectrum / focus entry point takes its own first / count. */
typedef struct ot_rays {
    int64_t N;   /* ray slots = plane stride (>= rays of the launch, see above)                     */
    int32_t nt;  /* sections per ray = n tracing surfaces + 2 (raytracer.py:278)                   */
    int32_t _pad;
    double* p;   /* (N, nt, 3) f64 F-order  p_list                                                 */
    double* s;   /* (N, 3)     f64 F-order  s0_list: in = initial, out = final direction           */
    float* w;    /* (N, nt)    f32 F-order  w_list                                                 */
    double* n;   /* (N, nt)    f64 F-order  n_list                                                 */
    float* wl;   /* (N,)       f32          wl_list                                                */
    float* pol;  /* (N, nt, 3) f32 F-order  pol_list; NULL when no_pol                             */
} ot_rays;

/* ---- library --------------------------------------------------------------------------------- */
int ot_abi_version(void);
const char* ot_last_error(void);
/* number of HIP devices visible; negative on error */
int ot_device_count(void);

/* ---- scene ------------------------------------------------------------------------------------ */
/* Validates and uploads the scene tables (replaces nothing 1:1 -- the reference walks Python objects,
 * raytracer.py:274, 492-508).  Synchronous. */
int ot_scene_create(const ot_scene_desc* desc, ot_scene** out);
void ot_scene_destroy(ot_scene* scene);
/* nt = number of tracing surfaces + 2 (raytracer.py:278) */
int ot_scene_sections(const ot_scene* scene);

/* ---- sources ---------------------------------------------------------------------------------- */
int ot_sources_create(const ot_source* sources, int32_t n_sources, ot_sources** out);
void ot_sources_destroy(ot_sources* src);

/* RaySource.create_rays (ray_source.py:204) for every range, writing section 0 of `rays`
 * (p[:,0], s, w[:,0], wl, pol[:,0]) the way RayStorage.thread_rays does (ray_storage.py:156-166).
 * Device RNG: counter-based (Philox-4x32-10) keyed by (seed, range, ray); stratified grids use a
 * keyed bijective index permutation instead of the reference's shuffle (random.py:39-43). */
int ot_rays_generate(const ot_sources* src, const ot_source_range* ranges, int32_t n_ranges,
                     uint64_t seed, int32_t no_pol, const ot_rays* rays, void* stream);

/* ---- tracing ---------------------------------------------------------------------------------- */
/* Raytracer.trace / sub_trace (raytracer.py:262-415) for rays whose section 0 is already in `rays`
 * (injected or produced by ot_rays_generate).  Fills sections 1..nt-1 of p/w/n/pol, n[:,0], the
 * final directions in rays->s and ADDS the per-section counters to msgs (device, int64[5*nt + 1]:
 * the counters row-major (info, section), then one word that is set non-zero if a numeric hit search
 * ran into the 200-iteration timeout, where the reference raises TimeoutError surface.py:403).  hurb_normals: optional device array (2*n_hurb_elements*N f64:
 * for the j-th HURB aperture, N standard-normal draws for the a axis then N for the b axis,
 * replacing np.random.normal raytracer.py:468-469); NULL = device RNG keyed by `seed`. */
int ot_trace(const ot_scene* scene, const ot_rays* rays, const double* hurb_normals, uint64_t seed,
             int64_t* msgs, void* stream);

/* Fused generation + trace: same result as ot_rays_generate followed by ot_trace, but the freshly
 * generated ray never makes a round trip through HBM (one launch, ray state in registers). */
int ot_generate_and_trace(const ot_scene* scene, const ot_sources* src,
                          const ot_source_range* ranges, int32_t n_ranges, uint64_t seed,
                          const ot_rays* rays, int64_t* msgs, void* stream);

/* Raytracer.trace (raytracer.py:262-415) as ONE synchronous call: ot_generate_and_trace, then the wait for
 * `stream`; `msgs_host` (HOST memory, int64[5*nt + 1], layout as above) receives the counters of this
 * launch alone (the reference builds a fresh msgs array per trace, raytracer.py:289).  The device writes them
 * into a pinned buffer of the scene, so there is no device-to-host copy and no second synchronisation. */
int ot_generate_and_trace_host(const ot_scene* scene, const ot_sources* src,
                               const ot_source_range* ranges, int32_t n_ranges, uint64_t seed,
                               const ot_rays* rays, int64_t* msgs_host, void* stream);

/* Render-only chunk of Raytracer.iterative_render (raytracer.py:1235-1267: the images of all chunks are summed, only
 * the LAST chunk's rays stay in the tracer): n_rays rays are generated and traced as by ot_generate_and_trace_host,
 * but no section is stored.  Every ray that is still alive behind the last surface leaves its last section -- the
 * positions at sections nt-2 and nt-1, the weight at nt-2, the wavelength: what a detector behind the last surface
 * reads of a ray (raytracer.py:929-985) -- in `tail`, a ray storage with TWO sections (tail->nt == 2; p (N, 2, 3), w
 * (N, 2): section 1 is written as 0, every ray ends absorbed --, wl (N); s, n, pol unused, may be NULL) of
 * N = tail->N >= ot_tail_capacity(n_rays) slots, N a multiple of 65536.  The living rays are gathered wave by wave
 * into 1024 interleaved pieces (fill: device uint32[1024], scratch of the call); result2 (device-visible HOST memory,
 * int64[2]) receives the number of leading slots in use (a multiple of 65536; slots in it without a ray carry weight
 * 0) and the number of living rays.  The detector entry points (ot_detector_images, ot_detector_hits_multi,
 * ot_detector_extent_sample, ot_detector_image_auto_*) take `tail` with count = result2[0] like any other storage;
 * they give the images of the stored path for every detector that lies behind the last tracing surface.  The order
 * of the rays is not the order of generation (no per-source ranges).  msgs_host as for
 * ot_generate_and_trace_host.  Every scene has the form (ot_scene_tail_supported: 1 for a valid handle; kept for callers
 * written against ABI 7, where scenes with a numeric hit search had none). */
int64_t ot_tail_capacity(int64_t n_rays);
int ot_scene_tail_supported(const ot_scene* scene);
int ot_generate_and_trace_tail(const ot_scene* scene, const ot_sources* src, const ot_source_range* ranges,
                               int32_t n_ranges, uint64_t seed, int64_t n_rays, const ot_rays* tail, uint32_t* fill,
                               int64_t* result2, int64_t* msgs_host, void* stream);

/* The living rays of a stored chunk join the tail of the render-only chunk traced before it (ABI 9): `iterative_render`
 * keeps the rays of its LAST chunk (raytracer.py:1235-1267), which therefore goes through the ray storage -- its binning need
 * not be a pass of its own.  For the rays [first, first + count) of `rays` that are alive in their last section
 * (w[nt - 2] > 0), positions nt - 2 and nt - 1, the wavelength and the weight times weight_scale (formed in f64, rounded to
 * f32 once; the ratio chunk rays / tail rays makes the chunk's rays carry the power of the tail's) are appended to `tail`
 * behind what ot_generate_and_trace_tail(n_rays = rays_before) has written there -- same `fill`, untouched in between --,
 * then the tail is sealed again: result2 as above, for both together.  tail->N >= ot_tail_capacity(rays_before + count + 64).
 * Synchronous. */
int ot_tail_append(const ot_rays* rays, int64_t first, int64_t count, double weight_scale, int64_t rays_before,
                   const ot_rays* tail, uint32_t* fill, int64_t* result2, void* stream);

/* Measurement aid (the reference times `RT.trace` with perf_counter, tests/benchmark.py:81-86): with timing
 * on, every tracing launch of this scene records one HIP event right before and one right after the tracing
 * kernel on the launch stream; ot_scene_last_trace_ms waits for the later one and returns the kernel's
 * duration in milliseconds. */
int ot_scene_set_timing(ot_scene* scene, int32_t on);
int ot_scene_last_trace_ms(const ot_scene* scene, double* ms);

/* The plane rays->n holds, for every ray and section, the refractive index of the medium the section runs in: a function
 * of the scene, the section and the ray's wavelength alone, whether the ray is alive or not (raytracer.py:305, 327-332).
 * Nothing in this library reads it, and it is a sixth of what a trace writes.  ot_scene_set_index_store(scene, 0) makes
 * every later trace of this scene leave the plane untouched (rays->n must still be a valid buffer); the default, 1,
 * stores it with every trace as before.  ot_rays_fill_index writes n[:, section] of the rays [first, first + count) from
 * rays->wl, with the device functions and the spectrum handling (formulas, tables, per-line tables) of this scene's
 * last stored trace -- ot_trace, ot_generate_and_trace, ot_generate_and_trace_host; before any: the formulas --, so
 * that the plane is bit for bit what that trace stores with the switch on.  rays->nt must be the scene's section
 * count; only rays->N, nt, n and wl are used.  Asynchronous on `stream`. */
int ot_scene_set_index_store(ot_scene* scene, int32_t on);
int ot_rays_fill_index(const ot_scene* scene, const ot_rays* rays, int64_t first, int64_t count, void* stream);

/* The planes a trace may leave unwritten, as one mask per scene (default 0: complete storage).  OT_DEFER_INDEX is the
 * switch above.  OT_DEFER_POL: ot_generate_and_trace and ot_generate_and_trace_host leave rays->pol untouched (it must
 * still be a valid buffer when polarisation is on); the polarisation is computed as before -- the weights depend on it --
 * and nothing in this library reads the planes after the trace.  ot_trace stores them whatever the mask: its input
 * polarisation lives in section 0 of the plane and its rays cannot be repeated.
 * ot_scene_set_index_store is defined through the mask: on = 1 clears the WHOLE mask (every plane is stored), on = 0 sets
 * OT_DEFER_INDEX and leaves the other bits.
 * ot_rays_fill_pol writes pol[:, :, ray] of the rays [first, first + count) by repeating the trace: a trace that generates
 * its rays on the device is a function of (scene, sources, ranges, seed) alone, so with the arguments of that trace the
 * planes are bit for bit what it stores without OT_DEFER_POL.  `ranges` must cover the storage as they did for the trace,
 * rays->nt must be the scene's section count and the scene must track polarisation; only rays->N, nt and pol are used.
 * Counters are not touched and a hit-search timeout is not reported.  Asynchronous on `stream`.
 * OT_DEFER_SECTIONS: ot_generate_and_trace and ot_generate_and_trace_host write rays->p and rays->w for the last two sections
 * only (nt - 2 and nt - 1: what a detector behind the last surface and ot_tail_append read); s, wl and the counters as
 * before.  ot_trace stores every section whatever the mask.  ot_rays_fill_sections writes p and w of the sections
 * [0, nt - 2) of the rays [first, first + count) by repeating the trace with its arguments, bit for bit what the trace
 * stores without the bit, frozen and NaN positions of absorbed rays included; it rewrites s and wl with the values they
 * have.  rays->nt must be the scene's section count; rays->N, nt, p, w, s and wl are used, n and pol are not.  The scene's
 * counters, its pinned counter buffer and its timing events (ot_scene_last_trace_ms) are left as the trace set them, and a
 * hit-search timeout is not reported.  Asynchronous on `stream`.  A reader of the early sections pays one more trace. */
#define OT_DEFER_INDEX 1u
#define OT_DEFER_POL 2u
#define OT_DEFER_SECTIONS 4u
int ot_scene_set_deferred_planes(ot_scene* scene, uint32_t mask);
int ot_rays_fill_sections(const ot_scene* scene, const ot_sources* sources, const ot_source_range* ranges, int32_t n_ranges,
                          uint64_t seed, const ot_rays* rays, int64_t first, int64_t count, void* stream);
int ot_rays_fill_pol(const ot_scene* scene, const ot_sources* sources, const ot_source_range* ranges, int32_t n_ranges,
                     uint64_t seed, const ot_rays* rays, int64_t first, int64_t count, void* stream);

/* The step loop of the tracing kernels reads one compact "hot" record per step, compiled by ot_scene_create: the step,
 * the surface constants of the closed-form hit and normal, and a form code that holds the host's evaluation of the
 * wave-uniform decisions of that path (flat disc, ring, plain sphere, stable-root sphere, conic; OTHER = everything else,
 * which reads the surface record as before).  ot_scene_set_hot_steps(scene, 0) rewrites the scene's table with every form
 * OTHER, so that the same kernels take the surface-record path for every step; 1, the default, restores the forms.  The
 * results are bit for bit the same either way: the switch exists to compare the two paths.  Works on the scene's device
 * whichever device is current, and synchronises it.
 * ot_scene_records_host needs no device: it compiles a scene description as ot_scene_create does and copies one table
 * of records into `buf` -- table 0: the hot records (one per step and one of padding; hot_steps as above), 1: the surface
 * records, 2: the step records, in the layouts of csrc/ot_scene.hpp.  `count` and `record_bytes` receive the number of
 * records and the size of one; with buf == NULL nothing else happens. */
int ot_scene_set_hot_steps(ot_scene* scene, int32_t on);
/* the scene's hot records as its device holds them now: count = steps + 1 records of 192 bytes into buf */
int ot_scene_read_hot_steps(const ot_scene* scene, void* buf, int64_t buf_bytes, int32_t* count);
int ot_scene_records_host(const ot_scene_desc* desc, int32_t table, int32_t hot_steps, void* buf, int64_t buf_bytes,
                          int32_t* count, int32_t* record_bytes);

/* ---- leaf operators (public Surface / RefractionIndex methods) ---------------------------------- */
/* Surface.find_hit (surface.py:307, conic_surface.py:126): p, s are (n,3) F-order device arrays;
 * outputs p_hit (n,3) F-order, is_hit (n) uint8, ill (n) uint8: bit 0 = ill-conditioned bracket
 * (always 0 for analytic surfaces), bit 1 = the iteration timed out (surface.py:403). */
int ot_surface_find_hit(const ot_surface* surf, int64_t n, const double* p, const double* s,
                        double* p_hit, uint8_t* is_hit, uint8_t* ill, void* stream);
/* Surface.normals (surface.py:247, conic_surface.py:70, function_surface_2d.py:202): out (n,3) F-order */
int ot_surface_normals(const ot_surface* surf, int64_t n, const double* x, const double* y,
                       double* normals, void* stream);
/* Surface.mask (surface.py:235, ring_surface.py:123, rectangular_surface.py:100, slit_surface.py:89) */
int ot_surface_mask(const ot_surface* surf, int64_t n, const double* x, const double* y,
                    uint8_t* mask, void* stream);
/* Surface.values (surface.py:137) */
int ot_surface_values(const ot_surface* surf, int64_t n, const double* x, const double* y,
                      double* z, void* stream);
/* RingSurface.hurb_props / SlitSurface.hurb_props (ring_surface.py:88, slit_surface.py:65):
 * a_, b_ (n), b (n,3) F-order, inside (n) uint8 */
int ot_surface_hurb_props(const ot_surface* surf, int64_t n, const double* x, const double* y,
                          double* a_, double* b_, double* b, uint8_t* inside, void* stream);
/* RefractionIndex.__call__ (refraction_index.py:62): wl f32 device array as stored in RayStorage */
int ot_refraction_index(const ot_medium* medium, const double* table_pool, int64_t table_pool_len,
                        int64_t n, const float* wl, double* out, void* stream);

/* ---- detector --------------------------------------------------------------------------------- */
#define OT_PROJ_NONE 0          /* flat detector or projection_method=None                           */
#define OT_PROJ_EQUIDISTANT 1   /* spherical_surface.py:64                                          */
#define OT_PROJ_ORTHOGRAPHIC 2  /* :50                                                              */
#define OT_PROJ_EQUAL_AREA 3    /* :87                                                              */
#define OT_PROJ_STEREOGRAPHIC 4 /* :75                                                              */

/* Raytracer._hit_detector (raytracer.py:881-1051) over rays [first, first+count): for every ray
 * the section straddling the detector is searched, the detector surface is intersected with the
 * direction re-derived from stored positions (ray_storage.py:274-279), hits beyond the section end
 * are retried on the next section, and the optional sphere projection is applied.
 * Outputs are dense per-ray arrays (count entries): ph (count,3) F-order projected hit, hw f32 weight
 * (0 = no valid hit; the reference drops those rows, raytracer.py:1023), and ill_count (device
 * int64[2], ADDED to: [0] ill-conditioned rays, [1] rays whose numeric hit search timed out).  extent4 (device f64[4], may be NULL): running xmin,xmax,ymin,ymax of valid hits
 * (raytracer.py:1044-1046), must be initialised by the caller to +inf,-inf,+inf,-inf.
 * crop4 (HOST f64[4] xmin,xmax,ymin,ymax, may be NULL): a user extent; hits outside it are dropped like hits
 * without weight (raytracer.py:1036-1040). */
int ot_detector_hits(const ot_rays* rays, int64_t first, int64_t count, const ot_surface* detector,
                     int32_t projection, const double* crop4, double* ph, float* hw, double* extent4,
                     int64_t* ill_count, void* stream);

/* The same for up to 8 detectors (or positions of one detector) in one pass over the ray sections: the sections are
 * read once, every request gets its own outputs.  Serves Raytracer.iterative_render with a list of detector positions
 * (raytracer.py:1235-1267). */
typedef struct ot_detector_req {
    const ot_surface* detector;
    int32_t projection;   /* OT_PROJ_*                                              */
    int32_t xy_only;      /* 1: ph is (count,2), the z plane is not written         */
    const double* crop4;  /* HOST f64[4] user extent or NULL                        */
    double* ph;           /* device (count,3) F-order, (count,2) with xy_only; ph and hw both NULL (extent4 given):  */
    float* hw;            /* device (count)      extent-only request, nothing but extent4 and ill_count is written   */
    double* extent4;      /* device f64[4] or NULL, initialised by the caller       */
    int64_t* ill_count;   /* device int64[2], added to                              */
    /* Compact hit list (fill != NULL; needs xy_only; ph may be NULL = no positions): only the VALID hits are written, into a list of OT_HIT_PIECES
     * pieces of L = ot_hit_piece_len(count) entries each -- CAPACITY = OT_HIT_PIECES * L entries, which the caller
     * allocates: ph = x plane [CAPACITY] then y plane [CAPACITY], hw [CAPACITY], wl_out [CAPACITY] (the hit's
     * wavelength: the list no longer lines up with the rays).  Piece k holds fill[k] hits at its front, [k * L,
     * k * L + fill[k]); which piece a hit lands in and its place there are arbitrary.  fill (device
     * uint32[OT_HIT_PIECES]) must be zero on entry.  Consumed by ot_render_accumulate_compact. */
    float* wl_out;        /* device (CAPACITY) or NULL                              */
    uint32_t* fill;       /* device uint32[OT_HIT_PIECES] or NULL = dense list      */
} ot_detector_req;
#define OT_HIT_PIECES 1024
int64_t ot_hit_piece_len(int64_t count); /* entries per piece of a compact hit list of capacity count: the power of
                                          * two at or above count / 1024, at least 1024 (the last pieces stay empty) */
int ot_detector_hits_multi(const ot_rays* rays, int64_t first, int64_t count, const ot_detector_req* reqs,
                           int32_t n_reqs, void* stream);

/* Raytracer.detector_image with a known extent (raytracer.py:1053-1098: _hit_detector + RenderImage.render), and
 * the per-chunk, per-position body of iterative_render after its first chunk (raytracer.py:1244-1267), in one pass
 * over the ray sections for up to 8 detectors (or positions of one detector): hit search, projection, user extent,
 * misc.binning_indices_2d and the XYZW histogram update without the hit positions ever being written to memory.
 * Per request: hist (Ny, Nx, 4) f64 device, ADDED to; extent = image extent after RenderImage.__fix_extent;
 * crop4 = the user extent hits are restricted to (HOST f64[4]) or NULL; ill_count as in ot_detector_hits.
 * Same sums as ot_detector_hits_multi + ot_render_accumulate, in another order.
 * Environment (tests, profiling): OT_RENDER_PATH = direct | tiles pins the binning path (default: a probe of 4096 rays
 * decides); OT_TILE_LINEBUF = 0 takes the plain tile kernel where the one with per-tile line buffers in LDS would run
 * (one detector, image of at most 361 tiles of 64 x 64 pixels; also for ot_detector_image_auto_begin). */
typedef struct ot_detector_image_req {
    const ot_surface* detector;
    int32_t projection;   /* OT_PROJ_*                                              */
    int32_t Nx, Ny;       /* pixel counts (render_image.py:383-387)                 */
    int32_t _pad;
    const double* crop4;  /* HOST f64[4] or NULL                                    */
    double extent[4];     /* image extent [x0, x1, y0, y1]                          */
    double* hist;         /* device (Ny, Nx, 4) f64                                 */
    int64_t* ill_count;   /* device int64[2], added to                              */
    double weight_scale;  /* every hit's weight times this (f64) before it is added: 1 for a plain image; the chunks of
                           * an iterative render pass rays_step / N (raytracer.py:1257) and bin straight into one image */
} ot_detector_image_req;
int ot_detector_images(const ot_rays* rays, int64_t first, int64_t count, const ot_detector_image_req* reqs,
                       int32_t n_reqs, void* stream);

/* Detector image with an AUTOMATIC extent (Raytracer.detector_image(extent=None), raytracer.py:1042-1049 + 1053-1098) in
 * one pass over the ray sections, for detectors with a closed-form hit (flat, conic / spherical) without a sphere
 * projection -- others: OT_ERR_UNSUPPORTED, use ot_detector_hits_multi (compact list) + ot_render_accumulate_compact.
 * The image extent is the bounding box of the hits, known only after the last one; the calls below bin the hits on a
 * provisional tile grid first and into the final pixel grid afterwards (csrc/ot_detector_fused.hpp, last section):
 *
 *   ot_detector_extent_sample      extent4 (x0, x1, y0, y1; +-inf without a hit) of the hits of every stride-th wave of 64
 *                                  rays.  It lies inside the extent of all hits.  The caller lays a grid of tiles[0] x
 *                                  tiles[1] <= 2048 tiles of tile[0] x tile[1] mm with its corner at origin over it (plus
 *                                  a margin), such that one tile covers at most 61 x 61 pixels of the final image.
 *   ot_detector_image_auto_begin   hit search, records (x, y, w, wl: 24 B per valid hit) by tile, result6 = the exact
 *                                  extent of all valid hits (as ot_detector_req.extent4 reports it), result6[4] = hits
 *                                  outside the grid (kept in a list of result6[5] entries: more than that -> cancel and
 *                                  take the other path).  OT_ERR_UNSUPPORTED also where the records (24 B per ray,
 *                                  worst case) do not fit the device: the hit-list path needs less.
 *   ot_detector_image_auto_finish  extent = the image extent after RenderImage.__fix_extent, Nx, Ny its pixel counts,
 *                                  hist (Ny, Nx, 4) f64 device, ADDED to.  Same pixels and sums as ot_detector_hits_multi +
 *                                  ot_render_accumulate (sums in another order).  Frees the handle, also on failure.
 *   ot_detector_image_auto_cancel  frees the handle without an image.
 *
 * extent4 / result6: device-visible host memory (pinned, mapped) or device memory (every entry is written by a kernel).
 * Both calls that report wait for the stream before they return.  The records of an image live in a scratch block the
 * handle LEASES from begin until finish / cancel: automatic images may be open side by side (also on one stream, each
 * gets a block of its own), ot_scratch_trim leaves an open image alone.  finish must be given the stream of begin. */
typedef struct ot_auto_image ot_auto_image;
int ot_detector_extent_sample(const ot_rays* rays, int64_t first, int64_t count, const ot_surface* detector,
                              int32_t projection, int32_t stride, double* extent4, void* stream);
int ot_detector_image_auto_begin(const ot_rays* rays, int64_t first, int64_t count, const ot_surface* detector,
                                 int32_t projection, const double origin[2], const double tile[2], const int32_t tiles[2],
                                 double* result6, ot_auto_image** out, void* stream);
int ot_detector_image_auto_finish(ot_auto_image* image, const double extent[4], int32_t Nx, int32_t Ny, double* hist,
                                  void* stream);
void ot_detector_image_auto_cancel(ot_auto_image* image);

/* The binning paths keep their scratch (up to ~25 B per ray and image) between calls: blocks keyed by device, stream
 * and purpose, grown on demand (calls on one stream run in order, so a block serves call after call), not tied to the
 * thread that created them.  A call leases its block until its last launch is enqueued; a block on lease is neither
 * handed to another caller nor freed.  The pool keeps at most a cap of bytes (64 GB; OT_SCRATCH_CAP_GB in the
 * environment, or ot_scratch_set_cap): beyond it, and when an allocation fails, idle blocks go least recently used
 * first.  ot_scratch_trim waits for the device and returns every IDLE block to the driver (for a caller whose own
 * allocator needs the room); ot_scratch_stats reports bytes kept, blocks and blocks on lease.  All three are
 * thread-safe. */
int ot_scratch_trim(void);
int ot_scratch_set_cap(int64_t bytes);
int ot_scratch_stats(int64_t* kept_bytes, int32_t* blocks, int32_t* leased);

/* SphericalSurface.sphere_projection (spherical_surface.py:36-97): p (n,3) F-order -> out (n,3) F-order */
int ot_sphere_projection(const ot_surface* surf, int32_t projection, int64_t n, const double* p, double* out,
                         void* stream);

/* RenderImage.render inner part (render_image.py:396-418 + misc.binning_indices_2d misc.py:59-91 +
 * color.x/y/z_observer observers.py:14-41): bins n hits into hist (Ny, Nx, 4) f64 device array,
 * ADDING w*[xbar(wl), ybar(wl), zbar(wl), 1].  extent = [x0,x1,y0,y1] after RenderImage.__fix_extent.
 * Rays with w == 0 are skipped (they add nothing in the reference either).  Lists of 2^21 hits or more that
 * spread over many pixels are binned tile by tile in LDS (stream-ordered scratch of ~11 B per hit from the
 * device's default memory pool, which is set to keep its memory); the environment variable OT_RENDER_PATH =
 * direct | tiles pins the path. */
int ot_render_accumulate(int64_t n, const double* px, const double* py, const float* w,
                         const float* wl, const double extent[4], int32_t Nx, int32_t Ny,
                         double* hist, void* stream);
/* The same for the compact hit list of a bundle of n rays (see ot_detector_req.fill; px, py, w, wl hold
 * OT_HIT_PIECES * ot_hit_piece_len(n) entries): piece k contributes its first fill[k] entries.  With an automatic extent the hit search writes a third of the bytes (valid hits only) and the binning
 * reads only those. */
int ot_render_accumulate_compact(int64_t n, const uint32_t* fill, const double* px, const double* py, const float* w,
                                 const float* wl, const double extent[4], int32_t Nx, int32_t Ny, double* hist,
                                 void* stream);

/* ---- image conversion (next row) -------------------------------------------------- */
#define OT_IMG_IRRADIANCE 0       /* render_image.py:180 */
#define OT_IMG_ILLUMINANCE 1      /* :184 */
#define OT_IMG_SRGB_ABSOLUTE 2    /* :189  color.xyz_to_srgb srgb.py:379, rendering intent "Absolute"   */
#define OT_IMG_SRGB_PERCEPTUAL 3  /* :189  rendering intent "Perceptual" (L_th, chroma_scale)           */
#define OT_IMG_OUTSIDE_GAMUT 4    /* :197  color.outside_srgb_gamut srgb.py:84                          */
#define OT_IMG_LIGHTNESS 5        /* :202  CIELUV L   luv.py xyz_to_luv                                 */
#define OT_IMG_HUE 6              /* :206  luv_hue                                                      */
#define OT_IMG_CHROMA 7           /* :211  luv_chroma                                                   */
#define OT_IMG_SATURATION 8       /* :216  luv_saturation                                               */

/* added to an sRGB mode: color.xyz_to_srgb(normalize=False) / (clip=False), srgb.py:379-407 (used by convolve()) */
#define OT_IMG_FLAG_NO_NORMALIZE 0x100
#define OT_IMG_FLAG_NO_CLIP 0x200

/* RenderImage.get (render_image.py:131-222): converts the (Ny, Nx, 4) float64 XYZW histogram into a display
 * quantity.  fact joins fact x fact bins first (the reference's cv2.resize INTER_AREA, :174; must divide Nx and
 * Ny).  apx = area of one ORIGINAL pixel, K = luminous efficacy.  chroma_scale = NaN selects the automatic value.
 * out: (Ny/fact, Nx/fact, 3) float64 for the sRGB modes, (Ny/fact, Nx/fact) float64 otherwise.
 * workspace: device scratch of 4*(Nx/fact)*(Ny/fact) + 8 doubles.  Synchronises the stream for the sRGB modes
 * (image-wide decisions of srgb.py:318, 209, 250 are taken on the host). */
int ot_image_convert(const double* hist, int32_t Nx, int32_t Ny, int32_t fact, int32_t mode, double apx, double K,
                     double L_th, double chroma_scale, double* out, double* workspace, void* stream);

/* ---- colour conversions on arrays of the caller (optrace's color module: xyz.py, luv.py, srgb.py) ---- */
#define OT_COL_XYZ_TO_XYY 0            /* xyz.py:17   3 -> 3 channels                                              */
#define OT_COL_XYY_TO_XYZ 1            /* xyz.py:38   3 -> 3                                                       */
#define OT_COL_XYZ_TO_LUV 2            /* luv.py:20   3 -> 3; OT_IMG_FLAG_NO_NORMALIZE: Yn = 1 instead of max Y    */
#define OT_COL_LUV_TO_XYZ 3            /* luv.py:74   3 -> 3                                                       */
#define OT_COL_LUV_TO_UVL 4            /* luv.py:112  3 -> 3                                                       */
#define OT_COL_LUV_HUE 5               /* luv.py:156  3 -> 1                                                       */
#define OT_COL_LUV_CHROMA 6            /* luv.py:146  3 -> 1                                                       */
#define OT_COL_LUV_SATURATION 7        /* luv.py:130  3 -> 1                                                       */
#define OT_COL_SRGB_LINEAR_TO_XYZ 8    /* srgb.py:50  3 -> 3                                                       */
#define OT_COL_SRGB_TO_XYZ 9           /* srgb.py:71  3 -> 3                                                       */
#define OT_COL_XYZ_TO_SRGB_LINEAR 10   /* srgb.py:267 3 -> 3; intent, OT_IMG_FLAG_NO_NORMALIZE, L_th, chroma_scale */
#define OT_COL_XYZ_TO_SRGB 11          /* srgb.py:379 3 -> 3; the same and OT_IMG_FLAG_NO_CLIP                     */
#define OT_COL_OUTSIDE_GAMUT 12        /* srgb.py:84  3 -> 1 (1.0 outside, 0.0 inside)                             */
#define OT_COL_CHROMA_SCALE 13         /* srgb.py:242 Luv -> result[0]; out: NULL or (npx) factors (return_full)   */
#define OT_COL_LOG_SRGB 14             /* srgb.py:410 3 -> 3; result[0] = 1 where the input came back unchanged    */
#define OT_COL_SPECTRAL_COLORMAP 15    /* srgb.py:569 in: (npx) wavelengths in nm, out: (npx, 4) sRGB and alpha    */

/* rendering intent, added to OT_COL_XYZ_TO_SRGB_LINEAR / OT_COL_XYZ_TO_SRGB (neither: "Ignore") */
#define OT_COL_INTENT_ABSOLUTE 0x1000
#define OT_COL_INTENT_PERCEPTUAL 0x2000

/* One conversion of optrace's color module on a device array: in (npx, 3) float64, pixel after pixel; out (npx, 3) or
 * (npx) float64 as listed above.  `in` is not modified; out may be `in` for the two XYZ -> sRGB operations only.
 * L_th and chroma_scale (NaN = automatic) as in ot_image_convert; both are ignored by operations that have no such
 * argument.  result: host array of one double for OT_COL_CHROMA_SCALE and OT_COL_LOG_SRGB, else it may be NULL.
 * The image-wide quantities (max Y, the gamut flags, the minimum chroma factor, the lightness range) are maxima,
 * minima and flags reduced on the device, so no pixel's value depends on its position.  Launches are ordered on
 * `stream`; the stream is synchronised only where an image-wide decision picks the next launch: once for the Absolute
 * and twice for the Perceptual intent (as ot_image_convert), once for OT_COL_CHROMA_SCALE, once more for
 * OT_COL_LOG_SRGB; never for the other operations.  Scratch comes from the library's pool. */
int ot_color_convert(const double* in, int64_t npx, int32_t op, double L_th, double chroma_scale, double* out,
                     double* result, void* stream);

/* RenderImage._apply_rayleigh_filter (render_image.py:257-296): out = "same"-size 2-D convolution of each of the
 * 4 channels of `in` (Ny, Nx, 4) with the (2*ps+1)^2 kernel `psf` (device, row-major), zero padded, negative
 * results clamped to 0.  in and out must not alias.  next row, SURVEY 8f rank 2. */
int ot_image_convolve(const double* in, int32_t Nx, int32_t Ny, const double* psf, int32_t ps, double* out, void* stream);

/* LightSpectrum.render (spectrum/light_spectrum.py:41-79), the histogram behind Raytracer.detector_spectrum
 * (raytracer.py:1100-1132) and Raytracer.source_spectrum (raytracer.py:1307-1328).  Rays come dense: weight 0 =
 * not selected (as ot_detector_hits leaves them).  next row, SURVEY 8f rank 3.
 * ot_spectrum_range: range2[0..1] (device) = min / max wavelength of the rays with w > 0 (+inf / -inf if none),
 *   count[0] (device) = number of such rays (np.count_nonzero(w), light_spectrum.py:60).
 * ot_spectrum_histogram: hist[nbins] (device, f64, accumulated into: zero it first) += weights per bin of the
 *   float32 edges[nbins + 1] (device; np.linspace(wl0, wl1, nbins + 1) as float32).  Bin search as NumPy's
 *   uniform-bin path in float32 (numpy/lib/_histograms_impl.py), last bin closed on the right. */
int ot_spectrum_range(int64_t n, const float* wl, const float* w, double* range2, int64_t* count, void* stream);
int ot_spectrum_histogram(int64_t n, const float* wl, const float* w, const float* edges, int32_t nbins, double* hist,
                          void* stream);
/* The same over a compact hit list of a bundle of n rays (ot_detector_req.fill; positions are not needed: such a request may
 * leave ph NULL): piece k contributes its first fill[k] entries of wl and w. */
int ot_spectrum_range_compact(int64_t n, const uint32_t* fill, const float* wl, const float* w, double* range2,
                              int64_t* count, void* stream);
int ot_spectrum_histogram_compact(int64_t n, const uint32_t* fill, const float* wl, const float* w, const float* edges,
                                  int32_t nbins, double* hist, void* stream);

/* Raytracer.focus_search (raytracer.py:1463-1640).  next row, SURVEY 8f rank 3.
 * ot_focus_prepare: for rays [first, first + count) pick the section crossing z (pos = argmax(z < p_z) - 1,
 *   raytracer.py:1552-1560) and write the hit line ph(z') = pa + sb * z' (raytracer.py:1580-1583):
 *   pasb[4 * count] (device) = pa_x | pa_y | sb_x | sb_y, w[count] (device) = section weight, -1 for rays
 *   without such a section; n_use[0] (device) = number of rays kept.
 * ot_focus_cost: cost function __focus_search_cost_function (raytracer.py:1354-1418) of the kept rays at the nz
 *   positions z[] (host array), mode OT_FOCUS_*; cost[nz] (device).  n_px = image side for the image methods
 *   (100 * int(1 + sqrt(N) / 1500), made odd), workspace (device) >= OT_FOCUS_WS + n_px * n_px doubles.  After the
 *   call workspace[0..3] hold the extent x_min, x_max, y_min, y_max of the hits at the last z sample and, for the
 *   image methods, workspace + OT_FOCUS_WS holds the n_px x n_px image of that sample (row = y pixel).
 * ot_focus_moments: sums[16] (device) for __focus_rms_spot_direct_solution (raytracer.py:1420-1460), the mean
 *   position and the RMS cost curve: [0..4] = sum w, w pa_x, w pa_y, w sb_x, w sb_y; [5] = sum w^2 (dtx^2 + dty^2);
 *   [6] = sum w^2 (dtx dx + dty dy) for the bounds b0 < b1; [7] = sum w^2; [8..10] = sum w x0'^2, w x0' sbx', w sbx'^2
 *   with x0' = pa_x + sb_x z0 - mean, sbx' = sb_x - mean, z0 = (b0 + b1) / 2, [11..13] the same in y: the weighted
 *   variance at any z is ([8] + 2 (z - z0) [9] + (z - z0)^2 [10]) / ([0] - [7] / [0]) (np.cov with aweights). */
#define OT_FOCUS_RMS 0
#define OT_FOCUS_IRR_VAR 1
#define OT_FOCUS_SHARPNESS 2
#define OT_FOCUS_CENTER_SHARPNESS 3
#define OT_FOCUS_WS 16
int ot_focus_prepare(const ot_rays* rays, int64_t first, int64_t count, double z, double* pasb, float* w, int64_t* n_use,
                     void* stream);
int ot_focus_cost(int64_t count, const double* pasb, const float* w, int32_t mode, const double* z, int32_t nz,
                  int32_t n_px, double* workspace, double* cost, void* stream);
int ot_focus_moments(int64_t count, const double* pasb, const float* w, double b0, double b1, double* sums, void* stream);

/* ---- spot analysis (Raytracer.spot_analysis; no counterpart in optrace) ----------------------------------------
 * Figures of the hits of one detector, from the hit list of ot_detector_hits_multi: x[], y[] (f64 planes of ph), w[] (f32),
 * all DEVICE.  fill = NULL: a dense list of n entries; otherwise the compact list of a bundle of n rays
 * (ot_detector_req.fill: piece k contributes its first fill[k] entries).  An entry counts when w > 0; positions of the
 * others are not read into arithmetic.  Launches are ordered on `stream` and nothing is waited for: each call reads what
 * the one before it left in device memory.  Null arguments (fill apart): OT_ERR_INVALID, limits exceeded:
 * OT_ERR_UNSUPPORTED, both before a device is looked for; n = 0 returns OT_OK without a launch and leaves the outputs alone.
 * ot_spot_moments: moments[OT_SPOT_M] (device) = sum w | sum w x | sum w y | number of hits | sum w dx^2 | sum w dy^2 |
 *   sum w dx dy | max (dx^2 + dy^2), with d = p - c formed before squaring, c = (sum w x, sum w y) / sum w: a second pass
 *   over the list.  All zero without a hit.  workspace (device) >= OT_SPOT_WS(0) doubles.
 * ot_spot_radial: hist[n_radii] (device, f64, accumulated into: zero it first) += w per bin
 *   min(floor(r / r_max * n_radii), n_radii - 1), r = sqrt(dx^2 + dy^2), r_max = sqrt(moments[7]); bin 0 when r_max = 0.
 *   1 <= n_radii <= OT_SPOT_MAX_RADII.  The one call whose sums depend on the order of arrival (f64 atomics).
 * ot_spot_otf: otf[4 * K] (device) = re x | im x | re y | im y of sum w exp(-2 pi i freq[k] d) per axis, freq[K] (device)
 *   in cycles per length unit, 1 <= K <= OT_SPOT_MAX_FREQ; workspace (device) >= OT_SPOT_WS(K) doubles.
 * ot_spot_moments and ot_spot_otf add in an order fixed by n, K and the kind of list: the same call returns the same bits. */
#define OT_SPOT_M 8
#define OT_SPOT_MAX_RADII 65536
#define OT_SPOT_MAX_FREQ 4096
#define OT_SPOT_BLOCKS 2048 /* most workgroups whose partial sums the workspace holds */
#define OT_SPOT_WS(K) (32 * OT_SPOT_BLOCKS + 256 * ((K) + 8))
int ot_spot_moments(int64_t n, const uint32_t* fill, const double* x, const double* y, const float* w, double* workspace,
                    double* moments, void* stream);
int ot_spot_radial(int64_t n, const uint32_t* fill, const double* x, const double* y, const float* w, const double* moments,
                   int32_t n_radii, double* hist, void* stream);
int ot_spot_otf(int64_t n, const uint32_t* fill, const double* x, const double* y, const float* w, const double* moments,
                const double* freq, int32_t K, double* workspace, double* otf, void* stream);

/* ---- wavefront analysis (Raytracer.wavefront_analysis; no counterpart in optrace) -------------------------------
 * Optical path of the rays [first, first + count) of a storage to a reference sphere behind section `section`
 * (0 .. nt - 2: from p[section] to p[section + 1]), and reductions of it.  A ray is used when w[section] > 0 and the section
 * has a positive length L; its direction is s = (p[section + 1] - p[section]) / L.  Pointers are DEVICE unless said otherwise.
 * Launches are ordered on `stream` and nothing is waited for.  Null arguments (wl apart), a ray range outside the storage, a
 * section out of range, values that are not finite: OT_ERR_INVALID; limits exceeded: OT_ERR_UNSUPPORTED, both before a device
 * is looked for; count = 0 / n = 0 returns OT_OK without a launch and leaves the outputs alone.
 * ot_wavefront_focus: sums[OT_WF_FOCUS_M] = sum w | rays used | sum w q (3) | sum w s (3) | sum w (I - s s^T): xx xy xz yy yz
 *   zz | sum w (I - s s^T) q (3), with q = p[section] - origin, origin[3] HOST.  The point closest to all ray lines solves
 *   [sum w (I - s s^T)] (c - origin) = sum w (I - s s^T) q.  Reads p and w only.
 * ot_wavefront_paths: per ray, with o = p[section] - focus (focus[3] HOST), b = s . o, D = b^2 - (o . o - radius^2) and
 *   t = -b - sign(radius) sqrt(D): opl = sum_{j < section} n[j] |p[j + 1] - p[j]| + n[section] t, (u, v) = the x and y of
 *   (o + t s) / |radius|, w_out = w[section].  Rays not used, and used ones with D < 0 -- counted in *missed -- get w_out = 0
 *   and NaN elsewhere.  u, v, opl (f64) and w_out (f32) hold `count` entries each.  Reads p, w and n.
 * ot_wavefront_moments: moments[OT_WF_M] over the entries with w > 0 (the others are not read into arithmetic) = sum w |
 *   entries | sum w opl | sum w u | sum w v | sum w wl (0 where wl is NULL) | min opl | max opl | sum w (opl - mean)^2 |
 *   max (du^2 + dv^2) about the means of the first pass: a second pass over the list | the root of that maximum, the pupil
 *   radius the two calls below divide by.
 * ot_wavefront_map: map[2 * n_grid * n_grid] (accumulated into: zero it first) += w | w (opl - mean) per cell
 *   row * n_grid + column, column from x and row from y by min(floor((x + 1) / 2 * n_grid), n_grid - 1), (x, y) =
 *   ((u, v) - mean) / pupil radius.  pupil_radius NaN: moments[10]; otherwise entries with x^2 + y^2 > 1 are left out.
 *   1 <= n_grid <= OT_WF_MAX_GRID.  The one call whose sums depend on the order of arrival (f64 atomics).
 * ot_wavefront_zernike: out[J (J + 1) / 2 + J] = the upper triangle of sum w Z Z^T row by row, then sum w Z (opl - mean), Z
 *   the Noll-ordered orthonormal Zernike polynomials Z_1 .. Z_J at (x, y) as above, 1 <= J <= OT_WF_MAX_J.
 * workspace >= OT_WF_WS doubles.  ot_wavefront_focus, _moments and _zernike add in an order fixed by the counts and J alone:
 * the same call returns the same bits. */
#define OT_WF_FOCUS_M 17
#define OT_WF_M 11
#define OT_WF_MAX_J 36
#define OT_WF_MAX_GRID 1024
#define OT_WF_BLOCKS 2048 /* most workgroups whose partial sums the workspace holds */
#define OT_WF_WS (40 * OT_WF_BLOCKS)
int ot_wavefront_focus(const ot_rays* rays, int64_t first, int64_t count, int32_t section, const double* origin, double* workspace,
                       double* sums, void* stream);
int ot_wavefront_paths(const ot_rays* rays, int64_t first, int64_t count, int32_t section, const double* focus, double radius,
                       double* u, double* v, double* opl, float* w_out, int64_t* missed, void* stream);
int ot_wavefront_moments(int64_t n, const double* u, const double* v, const double* opl, const float* w, const float* wl,
                         double* workspace, double* moments, void* stream);
int ot_wavefront_map(int64_t n, const double* u, const double* v, const double* opl, const float* w, const double* moments,
                     double pupil_radius, int32_t n_grid, double* map, void* stream);
int ot_wavefront_zernike(int64_t n, const double* u, const double* v, const double* opl, const float* w, const double* moments,
                         double pupil_radius, int32_t J, double* workspace, double* out, void* stream);

/* ---- beam footprints (Raytracer.footprints; no counterpart in optrace) ------------------------------------------
 * Per section i of the storage (0: the sources; 1 .. nt - 2: behind tracing surface i - 1; nt - 1: the rays' ends), over the
 * rays [first, first + count): the living rays T = {w[i] > 0}, the arriving rays A = {w[i - 1] > 0} (A = T in section 0) and
 * where the living ones cross the surface.  Reads p and w only; positions and weights of rays outside T and A are not read into
 * arithmetic.  All arithmetic in f64.  Pointers are DEVICE; launches are ordered on `stream` and nothing is waited for.  A null
 * argument, a ray range outside the storage, nt < 2: OT_ERR_INVALID; n_px outside 1 .. OT_FP_MAX_PX, nt above
 * OT_FP_MAX_SECTIONS: OT_ERR_UNSUPPORTED, both before a device is looked for; count = 0 returns OT_OK without a launch and
 * leaves the outputs alone.
 * ot_footprint_moments: records[nt * OT_FP_M], per section
 *    0 sum_T w        1 |T|            2 sum_A w[i - 1]   3 |A|
 *    4 sum_T w x      5 sum_T w y      6 sum_T w z
 *    7 min x  8 max x  9 min y  10 max y  11 min z  12 max z   over T; NaN when T is empty
 *   13 sum_T w dx^2  14 sum_T w dy^2  15 sum_T w dx dy          d = (x, y) - c, c = (slot 4, slot 5) / slot 0, formed before
 *                                                               squaring: a second pass over the planes
 *   16 max_T ((x - ax)^2 + (y - ay)^2)                          (ax, ay) = axis[2 i], axis[2 i + 1]; 0 when T is empty
 *   axis[2 * nt]: the xy of the source (section 0) and of the surfaces; finite.  workspace >= ot_footprint_workspace(count, nt)
 *   doubles (0 for arguments out of range).  All sections go in one launch per pass; the sums are added in an order fixed by
 *   count alone: the same call returns the same bits, and slots 2, 3 of section i are bit for bit slots 0, 1 of section i - 1.
 * ot_footprint_maps: maps[nt * n_px * n_px] (accumulated into: zero it first), section i += w of every ray of T in cell
 *   row * n_px + column, column = min(floor(((x - ax) + R) / (2 R) * n_px), n_px - 1), not below 0, R = sqrt(slot 16) of
 *   records (as ot_footprint_moments left them); row likewise from y; cell 0 when R = 0.  The one call whose sums depend on
 *   the order of arrival (f64 atomics). */
#define OT_FP_M 17
#define OT_FP_MAX_PX 1024
#define OT_FP_MAX_SECTIONS 65535
#define OT_FP_BLOCKS 1024 /* most workgroups per section and 2^28 rays whose partial sums the workspace holds */
int64_t ot_footprint_workspace(int64_t count, int32_t nt);
int ot_footprint_moments(const ot_rays* rays, int64_t first, int64_t count, const double* axis, double* workspace, double* records,
                         void* stream);
int ot_footprint_maps(const ot_rays* rays, int64_t first, int64_t count, const double* axis, const double* records, int32_t n_px,
                      double* maps, void* stream);

/* ---- chromatic analysis (Raytracer.chromatic_analysis; no counterpart in optrace) --------------------------------
 * Per band of wavelengths, over the rays [first, first + count) of a storage and its section `section` (0 .. nt - 2): the sums for
 * the point closest to the band's ray lines, and where the band's rays cross a plane z = const.  key[count] (bytes): the band of
 * ray first + i, 0 .. n_bands - 1, any other value (255 by convention): in no band.  A ray is used when w[section] > 0 and
 * d = p[section + 1] - p[section] has a length L > 0, as in the wavefront analysis; positions, weights and wavelengths of
 * other rays, and of rays of other bands, are not read into a band's arithmetic.  All arithmetic in f64.  Pointers are DEVICE
 * unless said otherwise; launches are ordered on `stream` and nothing is waited for.  A null argument, a ray range outside the
 * storage, a section out of range, z or origin not finite: OT_ERR_INVALID; n_bands outside 1 .. OT_CHROM_MAX_BANDS:
 * OT_ERR_UNSUPPORTED, both before a device is looked for; count = 0 returns OT_OK without a launch and leaves the outputs alone.
 * ot_chromatic_focus: sums[n_bands * OT_WF_FOCUS_M], per band the sums of ot_wavefront_focus over its used rays, with
 *   q = p[section] - origin, origin[3] HOST.  Reads key, p and w.
 * ot_chromatic_plane: records[n_bands * OT_CHROM_M], per band, with t = (z - p_z) / d_z, x = p_x + t d_x, y = p_y + t d_y of
 *   p = p[section] for its used rays with d_z != 0
 *    0 sum w          1 rays in the sums   2 sum w x     3 sum w y     4 sum w wl
 *    5 sum w dx^2     6 sum w dy^2         7 sum w dx dy               (dx, dy) = (x, y) - c, c = (slot 2, slot 3) / slot 0, formed
 *                                                                      before squaring: a second pass over the planes; NaN when
 *                                                                      slot 1 is 0
 *    8 max (dx^2 + dy^2); 0 when slot 1 is 0      9 used rays of the band with d_z == 0, which are in none of the sums
 *   Reads key, p, w and wl.  Both passes, their last kernels and the finish are queued without a host round trip.  Slots 0, 1, 4
 *   and 9 do not depend on z.  (Raytracer.chromatic_analysis refers its shifts to the band with used rays whose mean wavelength
 *   -- the line itself for a band that is one spectral line, slot 4 / slot 0 otherwise, no number when slot 1 is 0 -- lies
 *   nearest to a reference wavelength.)
 * workspace >= ot_chromatic_workspace(count, n_bands) doubles (0 for arguments out of range).  All bands go in one launch per
 * pass; the sums are added in an order fixed by count and n_bands alone: the same call returns the same bits. */
#define OT_CHROM_M 10
#define OT_CHROM_MAX_BANDS 32
#define OT_CHROM_BLOCKS 1024 /* most workgroups per band and 2^28 rays whose partial sums the workspace holds */
int64_t ot_chromatic_workspace(int64_t count, int32_t n_bands);
int ot_chromatic_focus(const ot_rays* rays, int64_t first, int64_t count, int32_t section, const uint8_t* key, int32_t n_bands,
                       const double* origin, double* workspace, double* sums, void* stream);
int ot_chromatic_plane(const ot_rays* rays, int64_t first, int64_t count, int32_t section, const uint8_t* key, int32_t n_bands,
                       double z, double* workspace, double* records, void* stream);

/* ---- field analysis (Raytracer.field_analysis; no counterpart in optrace) ----------------------------------------
 * Per field point and band of wavelengths the first and second moments of the ray lines of section `section` (0 .. nt - 2).
 * fields[n_fields][2] HOST: (first, count) of every field's rays in the storage; the ranges need not touch.  key (bytes):
 * key[r - key_first] is the band of ray r, 0 .. n_bands - 1, any other value (255 by convention): in no band; it covers
 * every field's range.  A ray is used when w[section] > 0 and d = p[section + 1] - p[section] has a length above 0; positions,
 * weights and wavelengths of other rays and of rays in no band are not read into arithmetic.  With q = p[section] - origin
 * (origin[3] HOST), m = (d_x, d_y) / d_z and a = (q_x, q_y) - q_z m -- the ray crosses a plane z at
 * origin_xy + a + (z - origin_z) m --, records[n_fields][n_bands][OT_FIELD_M] holds over the cell's used rays with d_z != 0
 *    0 sum w        1 rays in the sums   2 sum w a_x   3 sum w a_y   4 sum w m_x   5 sum w m_y   6 sum w wl
 *    7 used rays of the cell with d_z == 0, which are in none of the sums
 *    8 sum w da_x^2      9 sum w da_x da_y   10 sum w da_y^2
 *   11 sum w da_x dm_x  12 sum w da_x dm_y   13 sum w da_y dm_x   14 sum w da_y dm_y
 *   15 sum w dm_x^2     16 sum w dm_x dm_y   17 sum w dm_y^2
 *   da = a - (slot 2, slot 3) / slot 0, dm = m - (slot 4, slot 5) / slot 0, formed before multiplying: a second pass over the
 *   planes; slots 8 .. 17 are NaN when slot 1 is 0.  All arithmetic in f64.
 * Both passes request every ray's data once, whatever n_fields and n_bands are: the key byte of every ray of a field, and of a
 * ray with a band w, p[section], p[section + 1] and, in the first pass, wl.  Both passes, their last kernels and the finish are
 * queued on `stream` without a host round trip, and nothing is waited for.  The sums of a field are added in an order fixed by
 * its count and n_bands alone: the same call returns the same bits, and a field's records do not depend on the other fields.
 * A null argument, a ray range outside the storage, a field with rays that starts before key_first, a section out of range,
 * origin not finite: OT_ERR_INVALID; n_fields outside 1 .. OT_FIELD_MAX_FIELDS or n_bands outside 1 .. OT_CHROM_MAX_BANDS:
 * OT_ERR_UNSUPPORTED, both before a device is looked for; no ray in any field returns OT_OK without a launch and leaves the
 * outputs alone.  workspace >= ot_field_workspace(fields, n_fields, n_bands) doubles (0 for arguments out of range). */
#define OT_FIELD_M 18
#define OT_FIELD_MAX_FIELDS 64
#define OT_FIELD_BLOCKS 1024 /* most workgroups per field and 2^28 rays whose partial sums the workspace holds */
int64_t ot_field_workspace(const int64_t* fields, int32_t n_fields, int32_t n_bands);
int ot_field_sums(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key, int64_t key_first,
                  int32_t n_bands, const double* origin, double* workspace, double* records, void* stream);

/* ---- MTF analysis (Raytracer.mtf_analysis; no counterpart in optrace) ---------------------------------------------
 * Per field point, band of wavelengths, plane and spatial frequency the geometric OTF sums of the ray lines of section `section`,
 * along the tangential direction of the field and across it.  rays, fields, section, key, key_first, n_bands, origin: those of the
 * ot_field_sums call that wrote records[n_fields][n_bands][OT_FIELD_M] (DEVICE); the used rays, their bands and their lines
 * origin_xy + a + (z - origin_z) m are the ones of that call, formed by the same operations, and rays with d_z == 0 enter no sum.
 * About the means of the cell, da = a - (slot 2, slot 3) / slot 0, dm = m - (slot 4, slot 5) / slot 0 -- the quotients the second
 * pass of ot_field_sums forms --, with t = (t[f][0], t[f][1]) of the ray's field (t[n_fields][2] HOST) and s = (-t_y, t_x):
 *    al_t = t_x da_x + t_y da_y   mu_t = t_x dm_x + t_y dm_y   al_s = s_x da_x + s_y da_y   mu_s = s_x dm_x + s_y dm_y
 * and per plane j (zeta[n_planes] HOST: the plane's z minus origin_z) and frequency q (freq[n_freq] DEVICE, cycles per length):
 *    e = al + zeta_j mu,  tau = freq_q e,  tau -= rint(tau),  (sn, cs) = sin, cos (2 pi tau)
 *    sums[f][b][j][q] = (sum w cs_t, -sum w sn_t, sum w cs_s, -sum w sn_s)
 * over the rays in the record's sums: divided by slot 0 the OTF of the cell on the plane about its centroid there.  All arithmetic
 * in f64 without fused multiply-adds outside the sine and cosine.  A cell without a ray in the record's sums (slot 1 is 0) gets
 * zeros.  The launches are queued on `stream` without a host round trip, and nothing is waited for.  The sums of a field are added
 * in an order fixed by its count and (n_bands, n_planes, n_freq) alone: the same call returns the same bits, and a field's sums do
 * not depend on the other fields.  No atomics.
 * A null argument, a ray range outside the storage, a field with rays that starts before key_first, a section out of range,
 * origin, t or zeta not finite: OT_ERR_INVALID; n_fields outside 1 .. OT_FIELD_MAX_FIELDS, n_bands outside 1 ..
 * OT_CHROM_MAX_BANDS, n_planes outside 1 .. OT_MTF_MAX_PLANES or n_freq outside 1 .. OT_MTF_MAX_FREQ: OT_ERR_UNSUPPORTED, both
 * before a device is looked for; no ray in any field returns OT_OK without a launch and leaves the outputs alone.
 * workspace >= ot_mtf_workspace(fields, n_fields, n_bands, n_planes, n_freq) doubles (0 for arguments out of range): per field a
 * list of partials as long as the longest field's; a workgroup takes a group of KB = min(n_bands, 4) bands side by side and a tile
 * of TILE = 8 / KB (plane, frequency) pairs, 3 for KB = 3, and writes a partial of KB * 4 * TILE doubles; a field has a workgroup
 * per 256 rays, at most max(OT_MTF_MIN_BLOCKS, OT_MTF_BLOCKS / (groups * tiles)) per 2^28 rays.  A ray whose phase is no number
 * (|freq e| beyond the range of a double) turns the sums of that plane and frequency into no numbers for its own band and for
 * the other bands of its group in its field. */
#define OT_MTF_MAX_FREQ 64
#define OT_MTF_MAX_PLANES 65
#define OT_MTF_BLOCKS 1024   /* workgroups per field and 2^28 rays over all groups of bands and tiles, about */
#define OT_MTF_MIN_BLOCKS 16 /* ... and the fewest the largest fields are walked by */
int64_t ot_mtf_workspace(const int64_t* fields, int32_t n_fields, int32_t n_bands, int32_t n_planes, int32_t n_freq);
int ot_mtf_sums(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key, int64_t key_first,
                int32_t n_bands, const double* origin, const double* records, const double* t, const double* zeta, int32_t n_planes,
                const double* freq, int32_t n_freq, double* workspace, double* sums, void* stream);

/* ---- spot diagrams (Raytracer.spot_diagram; no counterpart in optrace) -------------------------------------------
 * Per field point, band of wavelengths and plane where the ray lines of section `section` land about a centre: a power map of
 * n_px x n_px cells, the rays binned and outside it, and the largest and the power-weighted sum of the squared distances from
 * the centre.  rays, fields, section, key, key_first, n_bands, origin: those of an ot_field_sums call; the used rays, their bands
 * and their lines origin_xy + a + (z - origin_z) m are the ones of that call, formed by the same operations, and a used ray with
 * d_z == 0 (slot 7 of that call's record) enters nothing.  centre[n_fields][n_bands][n_planes][2] DEVICE: the point every tile is
 * taken about, relative to origin_xy; zeta[n_planes] HOST: the plane's z minus origin_z.  For a ray of field f and band b on
 * plane j, every line one f64 operation per component and no fused product:
 *    x = a + zeta_j m          e = x - centre[f][b][j]
 *    scale = (double)n_px / size          half = 0.5 * n_px
 *    column = floor(e_x * scale + half)   row = floor(e_y * scale + half)
 * The ray is binned when column and row both lie in [0, n_px): maps[f][b][j][row][column] += w and counts[f][b][j][0] += 1.
 * Otherwise -- a value that is no number included -- counts[f][b][j][1] += 1 and outside_power[f][b][j] += w; nothing is clamped
 * into the map.  A ray with e = -size / 2 exactly lies in cell 0, one with e = +size / 2 exactly outside.  size: the side of every
 * tile, the same for all.  maps (f64), counts (64 bits, unsigned) and outside_power (f64) are accumulated into: the caller zeroes
 * them.  The sums of the maps and of outside_power depend on the order of arrival (f64 atomics); the counts do not.
 * ot_spotdiag_extent: ext[f][b][j] = (max |e|^2, sum w |e|^2), |e|^2 = e_x e_x + e_y e_y, over the same rays; a cell without a ray
 * gets zeros; a ray whose |e|^2 is no number is skipped by the maximum and turns the sum into no number.  The values of a field
 * are folded in an order fixed by its count and (n_bands, n_planes) alone: the same call returns the same bits, and a field's
 * values do not depend on the other fields.  workspace >= ot_spotdiag_workspace(fields, n_fields, n_bands, n_planes) doubles (0
 * for arguments out of range): per field a list of partials as long as the longest field's; a workgroup takes KB =
 * min(n_bands, 4) bands side by side and TILE = 8 / KB planes, 3 for KB = 3, and writes a partial of KB * 2 * TILE doubles; a field
 * has a workgroup per 256 rays, at most max(OT_SD_MIN_BLOCKS, OT_SD_BLOCKS / (groups * tiles)) per 2^28 rays.
 * ot_spotdiag_maps: a workgroup holds a chunk of T = OT_SD_LDS_BYTES / (8 n_px^2 + 40) whole (band, plane) tiles of a field in
 * LDS, K Z at the most, and the K Z tiles go in ot_spotdiag_chunks(n_bands, n_planes, n_px) = ceil(K Z / T) chunks; where T is 0
 * the cells are added to `maps` directly, in one chunk (ot_spotdiag_chunks: 1; 0 for arguments out of range).
 * All launches are queued on `stream` without a host round trip, and nothing is waited for.  Neither pass reads the direction,
 * index or polarisation planes.
 * A null argument, a ray range outside the storage, a field with rays that starts before key_first, a section out of range,
 * origin or zeta not finite, a size that is not finite or not above 0: OT_ERR_INVALID; n_fields outside 1 .. OT_FIELD_MAX_FIELDS,
 * n_bands outside 1 .. OT_CHROM_MAX_BANDS, n_planes outside 1 .. OT_MTF_MAX_PLANES, n_px outside 1 .. OT_SD_MAX_PX or
 * n_fields n_bands n_planes n_px^2 above OT_SD_MAX_CELLS: OT_ERR_UNSUPPORTED, both before a device is looked for; no ray in any
 * field returns OT_OK without a launch and leaves the outputs alone. */
#define OT_SD_MAX_PX 1024
#define OT_SD_MAX_CELLS ((int64_t)1 << 28)
#define OT_SD_BLOCKS 1024          /* extent pass: workgroups per field and 2^28 rays over all groups of bands and tiles, about */
#define OT_SD_MIN_BLOCKS 16        /* ... and the fewest the largest fields are walked by */
#define OT_SD_LDS_BYTES (159 * 1024) /* map pass: dynamic LDS of a workgroup at the most, one workgroup of 1024 lanes per CU */
#define OT_SD_MAP_BLOCKS 512       /* map pass: workgroups per field and 2^28 rays over all chunks, about */
#define OT_SD_MAP_MIN_BLOCKS 4     /* ... and the fewest the largest fields are walked by */
int64_t ot_spotdiag_workspace(const int64_t* fields, int32_t n_fields, int32_t n_bands, int32_t n_planes);
int32_t ot_spotdiag_chunks(int32_t n_bands, int32_t n_planes, int32_t n_px);
int ot_spotdiag_extent(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key,
                       int64_t key_first, int32_t n_bands, const double* origin, const double* centre, const double* zeta,
                       int32_t n_planes, double* workspace, double* ext, void* stream);
int ot_spotdiag_maps(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key,
                     int64_t key_first, int32_t n_bands, const double* origin, const double* centre, const double* zeta,
                     int32_t n_planes, int32_t n_px, double size, double* maps, uint64_t* counts, double* outside_power, void* stream);

/* ---- wavefront across the field (Raytracer.wavefront_field; no counterpart in optrace) ----------------------------
 * Per field point and band of wavelengths -- a cell -- the wavefront analysis above: the sums for a reference sphere, the optical
 * path of every ray to the sphere of its cell, the moments of the paths and the normal equations of a Zernike fit.  fields, key,
 * key_first, section, n_bands and the used rays: those of ot_field_sums; rays that are not used and rays in no band are not read
 * into arithmetic.  The dense planes u, v, opl (f64), w_out (f32) and the wl handed to ot_wavefield_moments start at ray
 * key_first, as key does: entry r - key_first belongs to ray r, and entries of no field are left alone.  All arithmetic in f64.
 * Pointers are DEVICE unless said otherwise; every entry queues its launches on `stream` without a host round trip, and nothing
 * is waited for.
 * ot_wavefield_focus: sums[n_fields][n_bands][OT_WF_FOCUS_M], per cell the sums of ot_wavefront_focus over its used rays, with
 *   q = p[section] - origin, origin[3] HOST.  Reads key, p and w.
 * ot_wavefield_paths: spheres[n_fields][n_bands][4] = (c_x, c_y, c_z, R) per cell; a cell has a sphere when all four are finite
 *   and R != 0.  A used ray of a cell with a sphere gets opl, (u, v) and w_out by the step of ot_wavefront_paths with (c, R):
 *   the same device function, so the same bits as that call with that sphere.  Every other ray of a field gets w_out = 0 and NaN
 *   elsewhere.  counts[n_fields][n_bands][2] (int64; zeroed here): used rays of the cell whose line misses its sphere | used
 *   rays of a cell without a sphere.  Reads key, p, w and n.
 * ot_wavefield_moments: an entry counts when its key is a band and w_out > 0.  moments[n_fields][n_bands][OT_WFF_M] =
 *    0 sum w   1 entries   2 sum w opl   3 sum w u   4 sum w v   5 sum w wl   6 min opl   7 max opl
 *    8 sum w (opl - slot 2 / slot 0)^2, the difference formed before squaring: a second pass over the planes
 *   a cell without an entry: slots 0 .. 7 are 0 and slot 8 is NaN.  pupil[n_fields][OT_WFF_PUPIL_M], common to the bands of a
 *   field: the centre (sum_b slot 3, sum_b slot 4) / sum_b slot 0, added in band order | the largest squared distance of the
 *   field's entries from it (0 without an entry) | its root, the pupil radius.
 * ot_wavefield_zernike: out[n_fields][n_bands][J (J + 1) / 2 + J], per cell the layout of ot_wavefront_zernike, Z at
 *   (x, y) = ((u, v) - the field's centre) / pupil radius by the same polynomial code, opl against the cell's mean.
 *   pupil_radius NaN: pupil[f][3]; otherwise entries with x^2 + y^2 > 1 are left out.  1 <= J <= OT_WF_MAX_J.  A cell without
 *   an entry: zeros.
 * focus and moments request every ray's data once, whatever n_fields and n_bands are: the key byte of every ray of a field and
 * the data of a ray with a band; paths likewise, one thread per ray.  zernike requests a field's key bytes once per band and
 * chunk of the triangle ((JT + 1) / 2 chunks, JT = 15 or 36) and an entry's planes once per chunk.  The sums of a field are
 * added in an order fixed by its count, n_bands and J alone and without f64 atomics: the same call returns the same bits, and
 * a field's outputs do not depend on the other fields.
 * A null argument, a ray range outside the storage, a field with rays that starts before key_first, a section out of range,
 * origin not finite, J below 1, a pupil radius that is neither NaN nor finite and above 0: OT_ERR_INVALID; n_fields outside
 * 1 .. OT_FIELD_MAX_FIELDS, n_bands outside 1 .. OT_CHROM_MAX_BANDS, J above OT_WF_MAX_J: OT_ERR_UNSUPPORTED, both before a
 * device is looked for; no ray in any field returns OT_OK without a launch and leaves the outputs alone.
 * workspace >= ot_wavefield_workspace(fields, n_fields, n_bands, J) doubles, for every entry (0 for arguments out of range). */
#define OT_WFF_M 9
#define OT_WFF_PUPIL_M 4
#define OT_WFF_FIT_BLOCKS 64 /* most workgroups per field, 2^28 rays, band and chunk whose partial sums of the fit the workspace holds */
int64_t ot_wavefield_workspace(const int64_t* fields, int32_t n_fields, int32_t n_bands, int32_t J);
int ot_wavefield_focus(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key,
                       int64_t key_first, int32_t n_bands, const double* origin, double* workspace, double* sums, void* stream);
int ot_wavefield_paths(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key,
                       int64_t key_first, int32_t n_bands, const double* spheres, double* u, double* v, double* opl, float* w_out,
                       int64_t* counts, void* stream);
int ot_wavefield_moments(const int64_t* fields, int32_t n_fields, const double* u, const double* v, const double* opl, const float* w,
                         const float* wl, const uint8_t* key, int64_t key_first, int32_t n_bands, double* workspace, double* moments,
                         double* pupil, void* stream);
int ot_wavefield_zernike(const int64_t* fields, int32_t n_fields, const double* u, const double* v, const double* opl, const float* w,
                         const uint8_t* key, int64_t key_first, int32_t n_bands, const double* moments, const double* pupil,
                         double pupil_radius, int32_t J, double* workspace, double* out, void* stream);

/* ---- ray fans (Raytracer.ray_fans; no counterpart in optrace) ----------------------------------------------------
 * Per band of wavelengths the transverse ray aberration and the optical path difference along two cuts of the pupil, from the
 * dense planes u, v, opl, w_out that ot_wavefront_paths left for the rays [first, first + count) and the moments record of
 * ot_wavefront_moments.  key[count] (bytes): the band of entry i, 0 .. n_bands - 1, any other value (255 by convention): in no
 * band.  An entry counts when w > 0; the other planes of entries that do not count, and of other bands, are not read into a
 * band's arithmetic.  All arithmetic in f64.  Pointers are DEVICE unless said otherwise; launches are ordered on `stream` and
 * nothing is waited for.  A null argument, count < 0, a ray range outside the storage, a section out of range, a focus that is
 * not finite, slab outside (0, 1], a pupil radius that is neither NaN nor above zero: OT_ERR_INVALID; n_bands outside
 * 1 .. OT_CHROM_MAX_BANDS, n_bins outside 1 .. OT_FAN_MAX_BINS: OT_ERR_UNSUPPORTED, both before a device is looked for;
 * count = 0 returns OT_OK without a launch and leaves the outputs alone.
 * ot_fans_transverse: for the entries with w > 0 (w[count], f32: the w_out of ot_wavefront_paths), with p = p[section],
 *   d = p[section + 1] - p and t = (focus_z - p_z) / d_z: ex = p_x + t d_x - focus_x, ey = p_y + t d_y - focus_y, where the ray
 *   crosses the plane z = focus z, against the focus (focus[3] HOST).  An entry with d_z == 0 is counted in *n_parallel and
 *   its w is set to 0, here, in place; it and the entries with w = 0 get NaN in ex and ey.  Reads p.
 * ot_fans_bands: records[n_bands * OT_FAN_M], per band over its entries with w > 0
 *    0 sum w          1 entries        2 sum w opl      3 sum w ex       4 sum w ey       5 sum w wl
 *    6 min opl        7 max opl                                                           0 when slot 1 is 0
 *    8 sum w opd^2    9 sum w dex^2   10 sum w dey^2   11 sum w dex dey                   opd = opl - slot 2 / slot 0, (dex, dey) =
 *                                                       (ex, ey) - (slot 3, slot 4) / slot 0, formed before squaring: a second
 *                                                       pass over the planes; slots 9 .. 11 NaN when slot 1 is 0, slot 8 is 0
 *   12 max (dex^2 + dey^2); 0 when slot 1 is 0
 *   workspace >= ot_fans_workspace(count, n_bands) doubles (0 for arguments out of range).  All bands go in one launch per
 *   pass; the sums are added in an order fixed by count and n_bands alone: the same call returns the same bits.
 * ot_fans_bins: out[n_bands][2][n_bins][OT_FAN_BIN_M] (accumulated into: zero it first).  (x, y) = ((u, v) - mean) / pupil
 *   radius as for ot_wavefront_map (pupil_radius NaN: moments[10]; otherwise entries with x^2 + y^2 > 1 are left out).  Fan 0,
 *   the tangential one, takes an entry when |x| <= slab and bins c = y; fan 1, the sagittal one, takes it when |y| <= slab and
 *   bins c = x; bin = min(floor((c + 1) / 2 * n_bins), n_bins - 1), not below 0.  Per bin, of the entries of the band:
 *    0 sum w    1 entries    2 sum w c    3 sum w ex    4 sum w ey    5 sum w opd, opd = opl - slot 2 / slot 0 of the band's
 *   record (as ot_fans_bands left it).  Slot 1 is exact; the other sums depend on the order of arrival (f64 atomics). */
#define OT_FAN_M 13
#define OT_FAN_BIN_M 6
#define OT_FAN_MAX_BINS 256
int64_t ot_fans_workspace(int64_t count, int32_t n_bands);
int ot_fans_transverse(const ot_rays* rays, int64_t first, int64_t count, int32_t section, const double* focus, float* w, double* ex,
                       double* ey, int64_t* n_parallel, void* stream);
int ot_fans_bands(int64_t count, const double* opl, const double* ex, const double* ey, const float* w, const float* wl,
                  const uint8_t* key, int32_t n_bands, double* workspace, double* records, void* stream);
int ot_fans_bins(int64_t count, const double* u, const double* v, const double* opl, const double* ex, const double* ey, const float* w,
                 const uint8_t* key, const double* moments, double pupil_radius, const double* records, int32_t n_bands, int32_t n_bins,
                 double slab, double* out, void* stream);

/* ---- Huygens point spread function (Raytracer.huygens_psf; no counterpart in optrace) -----------------------------
 * The coherent sum of one spherical wavelet per ray over the points of an image plane, from the rays' places and optical
 * paths on the reference sphere of the wavefront analysis above.  Pointers are DEVICE unless said otherwise; launches are
 * ordered on `stream` and nothing is waited for.  Bad arguments: OT_ERR_INVALID, n_px above OT_PSF_MAX_PX:
 * OT_ERR_UNSUPPORTED, both before a device is looked for; count = 0 / n = 0 returns OT_OK without a launch.
 * ot_psf_rays: rec[OT_PSF_REC * count], six planes of `count` entries: q (3) = (p[section] + t s - focus) / |radius|, the
 *   ray's place on the sphere by the step of ot_wavefront_paths (focus[3] HOST) | tau0 = (opl - mean) / lambda, turns, with
 *   opl[count] as ot_wavefront_paths wrote it, its mean moments[2] / moments[0] of ot_wavefront_moments and lambda = 1e-6 wl
 *   in mm | kappa = n[section] / lambda | a = sqrt(w[section]).  Rays that ot_wavefront_paths does not use: six zeros.
 *   Reads p, w, n and wl.
 * ot_psf_sum: with delta = x - focus, h = |radius| q and sg = sign(radius), U(x) = sum_i a_i exp(2 pi i tau_i),
 *   tau_i = tau0_i + sg kappa_i (|delta - h_i| - |radius|), the difference formed as
 *   (delta . delta - 2 |radius| delta . q) / (|delta - h| + |radius|).  field[2 * n_px * n_px] = Re U | Im U at the points
 *   delta = ((column + 1/2 - n_px / 2) size / n_px, (row + 1/2 - n_px / 2) size / n_px, dz), index row * n_px + column;
 *   centre[4] = Re U, Im U at delta = (0, 0, dz) | sum a | sum a^2.  1 <= n_px <= OT_PSF_MAX_PX, size finite and above
 *   zero, dz finite, radius finite and not zero.  workspace >= ot_psf_workspace(n, n_px) doubles (0 for arguments out of
 *   range).  The rays are added in an order fixed by n and n_px alone: the same call returns the same bits. */
#define OT_PSF_MAX_PX 1024
#define OT_PSF_REC 6
int64_t ot_psf_workspace(int64_t n, int32_t n_px);
int ot_psf_rays(const ot_rays* rays, int64_t first, int64_t count, int32_t section, const double* focus, double radius,
                const double* opl, const double* moments, double* rec, void* stream);
int ot_psf_sum(int64_t n, const double* rec, double radius, int32_t n_px, double size, double dz, double* workspace, double* field,
               double* centre, void* stream);

/* The same sum per band of the rays and per image plane (Raytracer.huygens_stack): rays of one band add coherently, bands add
 * in intensity.  Checks and codes as above; n_bands above OT_PSF_MAX_BANDS, n_planes above OT_PSF_MAX_PLANES and a request
 * whose workspace bound plus field exceeds OT_PSF_STACK_CAP doubles: OT_ERR_UNSUPPORTED.
 * ot_psf_stack: rec[OT_PSF_REC * n] grouped, band b the records [starts[b], starts[b + 1]), starts[n_bands + 1] HOST, ascending
 *   from 0 to n; plane z at dz[z], dz[n_planes] HOST.  field[n_planes][n_bands][2][n_px * n_px] = Re U | Im U of the band as
 *   ot_psf_sum forms them; sums[n_planes][n_bands][5] = Re U, Im U on the axis | sum a | sum a^2 | sum a^2 kappa.  A band
 *   without a record gives zeros.  One launch over (point tiles, ray chunks, planes): no chunk straddles a band, the chunk
 *   length is that of ot_psf_sum for n records with its workgroups, times min(n_planes, 4), divided among the planes.  The result is a function of
 *   rec, starts, n_px, size and dz alone; with one band and one plane it is ot_psf_sum's, bit for bit.
 *   workspace >= ot_psf_stack_workspace(n, n_bands, n_px, n_planes) doubles, a bound that needs no starts (0 for arguments out
 *   of range; with one band and one plane ot_psf_workspace(n, n_px)).
 * ot_psf_combine: from field and sums, with W = sum a^2, A = sum a, kb = sum a^2 kappa / W and the bands with W > 0 in
 *   ascending order: g[b] = W kb^2 / sum_c W_c kb_c^2 (0 for a band without a ray), band_strehl[n_planes][n_bands] = |U axis|^2 / A^2
 *   (NaN for such a band), intensity[n_planes][n_px * n_px] = sum_b g_b |U|^2 / A_b^2, strehl[n_planes] = sum_b g_b band_strehl,
 *   noise_floor[1] = sum_b g_b W_b / A_b^2. */
#define OT_PSF_MAX_BANDS 32
#define OT_PSF_MAX_PLANES 64
#define OT_PSF_STACK_CAP ((int64_t)1 << 28)
int64_t ot_psf_stack_workspace(int64_t n, int32_t n_bands, int32_t n_px, int32_t n_planes);
int ot_psf_stack(int64_t n, const double* rec, int32_t n_bands, const int64_t* starts, double radius, int32_t n_px, double size,
                 int32_t n_planes, const double* dz, double* workspace, double* field, double* sums, void* stream);
int ot_psf_combine(int32_t n_bands, int32_t n_planes, int32_t n_px, const double* field, const double* sums, double* intensity,
                   double* band_strehl, double* strehl, double* g, double* noise_floor, void* stream);

/* The stack for the fields of a field series in one call (Raytracer.huygens_field): cell f n_bands + b holds the rays of field f
 * in band b, every field has a reference sphere of its own.  Checks and codes as above, with the name of the entry point in
 * ot_last_error; n_fields above OT_FIELD_MAX_FIELDS: OT_ERR_UNSUPPORTED.
 * ot_psf_field_rays: rec[OT_PSF_REC * span], entry i ray key_first + i: the record of ot_psf_rays against the sphere
 *   spheres[f][b][4] = (c, R) and the mean path moments[f][b][2] / moments[f][b][0] (ot_wavefield_moments) of the ray's cell --
 *   f the field whose range fields[f] = (first, count) (HOST) holds the ray, b = key[i] --, with opl[span] as
 *   ot_wavefield_paths wrote it.  A ray of no field, a key of n_bands or above, a cell whose sphere holds no number, and the
 *   rays that ot_wavefield_paths does not use: six zeros.  Every field lies within [key_first, key_first + span).
 * ot_psf_field_sum: rec[OT_PSF_REC * n] grouped by cell, starts[n_fields * n_bands + 1] HOST, ascending from 0 to n;
 *   radius[n_fields] HOST, finite and not zero (of a field without a record: any such number).
 *   field[n_fields][n_planes][n_bands][2][n_px * n_px] and sums[n_fields][n_planes][n_bands][5] as ot_psf_stack forms them per
 *   band.  One launch over (point tiles, ray chunks, planes): no chunk straddles a cell, a cell without a record owns none, the
 *   chunk length is that of ot_psf_stack for ceil(n / g) records, g the fields that hold a record, and n_planes planes.  table: OT_PSF_FIELD_TABLE(n_fields * n_bands)
 *   8-byte words on the DEVICE that the call fills with the cells.  The result is a function of rec, starts, radius, n_px, size
 *   and dz alone; with one field it is ot_psf_stack's, bit for bit.  workspace >= ot_psf_field_workspace(...) doubles, a bound
 *   that needs no starts (0 for arguments out of range; with one field ot_psf_stack_workspace); workspace bound plus field above
 *   OT_PSF_STACK_CAP doubles, or a bound of more than 65535 chunks (the grid's second dimension): OT_ERR_UNSUPPORTED.
 * ot_psf_field_combine: ot_psf_combine per field: intensity[n_fields][n_planes][n_px * n_px], band_strehl[n_fields][n_planes]
 *   [n_bands], strehl[n_fields][n_planes], g[n_fields][n_bands], noise_floor[n_fields]; a field without a ray: NaN in intensity,
 *   strehl and noise_floor.
 * ot_psf_field_otf: with J = intensity - noise_floor of the field, the pixel centres (x, y) of ot_psf_sum relative to the focus,
 *   t[n_fields][2] HOST and s = (-t_y, t_x): out[n_fields][n_planes][n_freq][6] = Re, Im of sum_p J_p exp(-2 pi i nu (t . x_p)) |
 *   Re, Im of the same along s | their moduli over |sum_p J_p|.  frequencies[n_freq] HOST, 1 <= n_freq <= OT_PSFF_MAX_FREQ
 *   (OT_ERR_UNSUPPORTED above), finite, not below zero and not above n_px / (2 size).  The sums are added in an order fixed by
 *   n_px alone (csrc/ot_psf_field.hpp). */
#define OT_PSFF_MAX_FREQ 64
#define OT_PSF_FIELD_TABLE(cells) (4 * (int64_t)(cells) + 2)
int64_t ot_psf_field_workspace(int64_t n, int32_t n_fields, int32_t n_bands, int32_t n_px, int32_t n_planes);
int ot_psf_field_rays(const ot_rays* rays, const int64_t* fields, int32_t n_fields, int32_t section, const uint8_t* key,
                      int64_t key_first, int64_t span, int32_t n_bands, const double* spheres, const double* opl,
                      const double* moments, double* rec, void* stream);
int ot_psf_field_sum(int64_t n, const double* rec, int32_t n_fields, int32_t n_bands, const int64_t* starts, const double* radius,
                     int32_t n_px, double size, int32_t n_planes, const double* dz, int64_t* table, double* workspace, double* field,
                     double* sums, void* stream);
int ot_psf_field_combine(int32_t n_fields, int32_t n_bands, int32_t n_planes, int32_t n_px, const double* field, const double* sums,
                         double* intensity, double* band_strehl, double* strehl, double* g, double* noise_floor, void* stream);
int ot_psf_field_otf(int32_t n_fields, int32_t n_planes, int32_t n_px, double size, const double* intensity,
                     const double* noise_floor, const double* t, int32_t n_freq, const double* frequencies, double* out, void* stream);

/* ---- field-dependent convolution (ot.convolve_field; no counterpart in optrace) -----------------------------------
 * An image spread by a gy x gx grid of point spread functions, one per field point, blended bilinearly over the image's
 * interior: the PSF belongs to the SOURCE pixel.  Planar layouts: img[n_ch][ny][nx], psf[gy][gx][py][px],
 * out[n_ch][ny + py - 1][nx + px - 1], the full convolution.  The interior is the rectangle [y0, y0 + ny_in) x
 * [x0, x0 + nx_in) of the plane; pixels outside it (a padding rim) take the weights of the nearest interior pixel.  Node
 * (b, a) belongs to the interior's row fraction b / (gy - 1) and column fraction a / (gx - 1).  With hat(u) = max(0, 1 - |u|),
 *   t_x(i) = clamp((i - x0) / (nx_in - 1), 0, 1) (gx - 1)   (0 when gx = 1 or nx_in = 1; t_y alike),
 *   W[b][a](j, i) = hat(t_y(j) - b) hat(t_x(i) - a),
 *   out[c][y][x] = sum_{b,a} sum_{dy,dx} psf[b][a][dy][dx] W[b][a](y - dy, x - dx) img[c][y - dy][x - dx]
 * over the taps with 0 <= y - dy < ny, 0 <= x - dx < nx.  Pointers are DEVICE; the launch is ordered on `stream` and nothing is
 * waited for.  A null pointer, n_ch outside 1..3, a size below 1, an interior that is not inside the plane: OT_ERR_INVALID;
 * py or px above OT_CONVF_MAX_PSF, gy or gx above OT_CONVF_MAX_GRID, an output plane above 2^31 - 1 elements:
 * OT_ERR_UNSUPPORTED; all before a device is looked for.  Every output element is written once by one lane, its terms added in
 * f64 with fused multiply-adds in an order fixed by the shapes alone: the same call returns the same bits. */
#define OT_CONVF_MAX_PSF 512  /* py, px */
#define OT_CONVF_MAX_GRID 64  /* gy, gx */
int ot_convolve_field(const double* img, int32_t n_ch, int32_t ny, int32_t nx, int32_t y0, int32_t x0, int32_t ny_in,
                      int32_t nx_in, const double* psf, int32_t gy, int32_t gx, int32_t py, int32_t px, double* out, void* stream);

/* ---- samplers: optrace/tracer/random.py, Surface.random_positions, color.random_wavelengths_from_srgb ---------
 * The samplers of the ray generator (ot_rays_generate) as entry points of their own: sample i of a call is what the
 * generator draws for ray i of a launch with the same seed and the same ranges -- counter-based dither keyed by (seed, i),
 * strata assigned by a keyed permutation of each range instead of the reference's shuffle (random.py:39-43, 65-66).
 * `ranges`: the stratification domains, as for ot_rays_generate (`source` and `ray_power` are not read): at most 64 of
 * them, in order and without gaps over [0, n); each holds at most 2^32 - 1 samples (OT_ERR_UNSUPPORTED beyond).  A range
 * whose count is a power of two of 4 or more fills a 2^ceil(m/2) x 2^floor(m/2) jittered grid with ALL its samples in the
 * 2-D samplers; other counts use floor(sqrt(count))^2 cells and draw the rest uniformly, as the reference does.
 * All outputs are DEVICE arrays of float64; launches are ordered on `stream`; n = 0 returns OT_OK without a launch;
 * arguments are checked before a device is looked for. */
#define OT_SAMPLE_INTERVAL 0   /* stratified_interval_sampling random.py:48; bounds = {a, b}; flag: shuffle             */
#define OT_SAMPLE_RECTANGLE 1  /* stratified_rectangle_sampling random.py:8; bounds = {a, b, c, d}                       */
#define OT_SAMPLE_RING 2       /* stratified_ring_sampling random.py:70; bounds = {ri, r}; flag: polar                   */
/* out0[n] and, for the 2-D kinds, out1[n]: x | x, y | x, y or, polar, |r|, theta [rad] (random.py:104-110).  Interval with
 * flag = 0: stratum i holds sample i of its range (ascending within a range). */
int ot_sample_stratified(int32_t kind, int32_t flag, const double* bounds, const ot_source_range* ranges, int32_t n_ranges,
                         uint64_t seed, int64_t n, double* out0, double* out1, void* stream);

/* random_positions of the source shapes (point.py:62, line.py:81, circular_surface.py:33, ring_surface.py:135,
 * rectangular_surface.py:142): p = x[n] | y[n] | z[n].  Of `shape` only shape, pos, r, ri, dim and angle are read;
 * OT_SRC_IMAGE_* return OT_ERR_UNSUPPORTED. */
int ot_sample_positions(const ot_source* shape, const ot_source_range* ranges, int32_t n_ranges, uint64_t seed, int64_t n,
                        double* p, void* stream);

#define OT_SAMPLE_DISCRETE 0    /* random.py:136-146: entries with f > 0, the first whose running sum reaches X         */
#define OT_SAMPLE_CONTINUOUS 1  /* random.py:150-157: linear inverse of the cumulative trapezoid                         */
/* inverse_transform_sampling random.py:113-159 of the pdf f[m] over x[m] (HOST arrays, f >= 0 with a positive sum).
 * S: DEVICE array of n values in [0, 1], the caller's uniform variable (ranges are not read then), or NULL: n values
 * stratified over the ranges.  out[n].  The tables go to the device in stream order; the call waits for that copy. */
int ot_sample_inverse(int32_t kind, const double* x, const double* f, int64_t m, const double* S, int64_t n,
                      const ot_source_range* ranges, int32_t n_ranges, uint64_t seed, double* out, void* stream);

/* color.random_wavelengths_from_srgb srgb.py:513-553: rgb (n, 3) DEVICE, row-major sRGB values; wl[n] in nm.  The primary
 * of a row is chosen by a variable stratified over the rows of its range, which, rescaled, also places the wavelength inside
 * the primary (as for the pixels of an RGB image source); a black row takes the blue primary, as in the reference. */
int ot_sample_srgb_wavelengths(const double* rgb, int64_t n, const ot_source_range* ranges, int32_t n_ranges, uint64_t seed,
                               double* wl, void* stream);

/* ---- diagnostics ------------------------------------------------------------------------------------------
 * The tracing loop issues f64 division and square root as their bare cores (reciprocal / reciprocal-square-root seed +
 * the refinement steps of the IEEE sequence, without its range scaling and special-value fix-up; csrc/ot_device.hpp).
 * Bit-exact hit masks need those cores to return the bits of IEEE `/` and sqrt on every operand the path produces.
 * ot_selftest_arith draws n random operand sets of a class ON THE DEVICE, evaluates core and IEEE operator side by side
 * and counts sets whose result bits differ (two NaNs count as equal); first_bad4 (HOST f64[4]) receives the operands
 * a, b, c and the core's first result of one differing set.  mismatches is a HOST int64.
 *   op:    0 ot_div(a, b) | 1 ot_sqrt(|a|) | 2 normalize3(a, b, c) | 3 two quotients a / c, b / c sharing one reciprocal
 *   class: 0 uniform mantissas, exponents +-500 (sqrt: 2^-760 .. 2^1020, normalize3: +-250) | 1 mm geometry 2^-20 .. 2^14
 *          | 2 refractive indices [1, 2.5] | 3 direction cosines near 0 and near 1
 * op 4 with class 4 is a measurement instead: the relative error |1 - a y| of y = the hardware reciprocal seed, the seed
 * with one and with two Newton steps, and the fast reciprocal the refraction step uses, over n operands a of the range that
 * step produces (positive, exponents +-60).  first_bad4 receives the four largest errors in that order; mismatches counts
 * the operands on which the shipped reciprocal exceeds the bound stated at its definition (csrc/ot_device.hpp).
 * ot_selftest_eval evaluates both on caller-supplied DEVICE operands (special values); outputs are (n, 3) F-order. */
int ot_selftest_arith(int32_t op, int32_t operand_class, int64_t n, uint64_t seed, int64_t* mismatches,
                      double* first_bad4, void* stream);
int ot_selftest_eval(int32_t op, int64_t n, const double* a, const double* b, const double* c, double* core_out,
                     double* ieee_out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* OPTRACE_AMD_H */
