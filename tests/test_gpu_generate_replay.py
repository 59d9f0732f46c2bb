"""Ray generation, ray by ray, against the host replay of its draws (tests/generate_replay.py).

The generator is stateless: ray j of a range is a function of (seed, global index, range id, j, n, source record).  The
replay repeats the integer part bit for bit and evaluates RaySource.create_rays (ray_source.py:204-437) in longdouble behind
the same uniform variables, so every ray of every case is compared on its own: p, s, pol, w and wl.

Order of every case: the replay first; it must report near == 0 (no ray whose uniform variable lies within 8 eps of a table
node, a cell edge or a branch point -- otherwise another seed is chosen); only then is the device consulted.

Integer facts are exact: which stratum / cell, which spectral line, which pixel, `w == float32(power / n)`, a monochromatic
wl.  Continuous outputs carry (roundings in the chain) x eps x scale, counted where they are asserted; ot_div, ot_sqrt and
the ot_rsqrt normalisations return IEEE bits (tests/test_gpu_arith_exact.py).

Coverage of the arms of generate_ray by the sources of `SOURCES` (each at n = 1000 and 4096, S02 and S07 also at 1 and 3):

    id   shape        divergence          orientation     polarisation   spectrum
    S01  point        none                tilted const    constant 30    monochromatic (float32 rounding of wl)
    S02  point        Lambertian 3-D      converging      uniform        rectangle
    S03  point        isotropic 2-D  35   tilted const    list (a zero)  lines (a zero-weight line)
    S04  line 30      function 3-D        tilted const    function       Gaussian
    S05  circle       isotropic 3-D       const z         no_pol         d65 (tabulated)
    S06  ring         Lambertian 2-D -50  tilted const    x              d65
    S07  rect 25      function 2-D   70   converging      uniform        blackbody
    S08  rect 25      isotropic 3-D       function        list           rectangle
    S09  line 30      none                function        function       lines
    S10  circle       none                converging      constant 75    d65
    S11  RGB image    Lambertian 3-D      tilted const    uniform        (primaries)
    S12  grey image   isotropic 2-D  20   converging      list           Gaussian
    S13  ring         function 3-D        converging      no_pol         blackbody
    S14  point        none                const z (s_z = 1: the unrotated polarisation)  uniform   monochromatic
    S15  RGB image    none                converging      no_pol         (primaries)
    S16  grey image   function 3-D        tilted const    function       d65

Functions without a stated accuracy.  sincospi_small and sincos reach float64 outputs (p of a disc, s of a diverging source):
their error is measured here against the longdouble replay (`test_function_errors`, printed), recorded below, and every
assertion that has one of them in its chain grants 4 x the recorded figure on top of its counted roundings.  The figures
include the few roundings in front of the function (the sampler's).
    sincospi_small   worst |error| / scale   3.72e-16   (p of a unit disc, s of a 60 degree Lambertian cone)
    sincos           worst |error| / scale   2.39e-16   (s of an 80 degree isotropic fan)
erfinv (Gaussian spectrum) and ot_rcp3 (polarisation frame) only reach float32 outputs (wl, pol): beyond half a float32 ulp
their error cannot be seen from outside, and within it they are held to it: |wl - reference| <= ulp32 / 2 + the float64
bound of the chain, likewise pol.  `test_function_errors` prints their worst deviation in float32 ulps: 0.49997 (wl of a
Gaussian spectrum) and 0.50000 (pol), that is, the float32 rounding of the reference value and nothing else.
The condition of the issue -- none above 1e-13 relative to its scale -- is asserted for the two measurable ones.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd._device import stream_ptr
from optrace_amd.image import srgb_r_primary, srgb_g_primary, srgb_b_primary
from optrace_amd.ray_storage import SourceTable, stratification_blocks
from optrace_amd.spectrum import wavelengths
import generate_replay as gr
import scenes

pytestmark = pytest.mark.gpu

EPS = gr.EPS
# worst |device - replay| / scale measured on the MI355X by test_function_errors (seeds 77 and HI_SEED, n = 1000 and 4096)
MEASURED = {"sincospi_small": 3.72e-16, "sincos": 2.39e-16}
HI_SEED = (0x5eed << 32) | 12345  # a non-zero high word: stream_key and the Philox key both use it
X_DEF = gr.primary_inverse((srgb_r_primary, srgb_g_primary, srgb_b_primary), wavelengths(gr.PRIM_N))


# ---- device side and comparison --------------------------------------------------------------------------------------------
def device_rays(sources, ranges, seed, no_pol, powers=None, s_or=None):
    """ot_rays_generate into fresh one-section buffers -> dict of host arrays p, s, pol (N, 3), w, wl"""
    lib = _capi.load_library()
    N = max(r[1] + r[2] for r in ranges)
    powers = [rs.power for rs in sources] if powers is None else powers
    dev_or = None
    if s_or:
        dev_or = {i: torch.from_numpy(np.ascontiguousarray(np.asarray(a, dtype=np.float64).T).reshape(-1)).cuda() for i, a in s_or.items()}
    tab = SourceTable(sources, powers, dev_or)
    buf = {k: torch.full((m * N,), float("nan"), dtype=dt, device="cuda") for k, m, dt in
           (("p", 3, torch.float64), ("s", 3, torch.float64), ("w", 1, torch.float32), ("n", 1, torch.float64),
            ("wl", 1, torch.float32), ("pol", 3, torch.float32))}
    rays = _capi.Rays()
    rays.N, rays.nt = N, 1
    rays.p, rays.s, rays.w, rays.n, rays.wl = (buf[k].data_ptr() for k in ("p", "s", "w", "n", "wl"))
    rays.pol = None if no_pol else buf["pol"].data_ptr()
    rng = (_capi.SourceRange * len(ranges))()
    for r, (src, first, count, ray_power) in zip(rng, ranges):
        r.source, r.first, r.count, r.ray_power = src, first, count, ray_power
    _capi.check(lib.ot_rays_generate(tab.handle, rng, len(rng), seed, int(no_pol), C.byref(rays), stream_ptr()))
    torch.cuda.synchronize()
    out = {k: buf[k].cpu().numpy() for k in ("w", "wl")}
    for k in ("p", "s", "pol"):
        out[k] = buf[k].cpu().numpy().reshape(3, N).T
    return out


def fields_of(sources, powers=None):
    out = []
    for i, rs in enumerate(sources):
        f = rs._source_fields()
        f["power"] = float(rs.power if powers is None else powers[i])
        out.append(f)
    return out


def ulp32(v):
    """the float32 spacing in the binade of |v|"""
    a = np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -126)
    return 2.0 ** (np.floor(np.log2(a)) - 23)


def worst(dev, ref):
    return float(np.abs(dev.astype(gr.LD) - ref).max(initial=0))


def check_rays(dev, rep, fields, no_pol, label):
    """every ray of `dev` against the replay `rep`"""
    covered = rep["rid"] >= 0
    assert np.array_equal(dev["w"][covered], rep["w"][covered]), f"{label}: w"  # float32(power / n), exact
    assert np.isnan(dev["w"][~covered]).all(), f"{label}: rays outside every range were written"
    for first, count, src, o in rep["facts"]:
        f, sl, tag = fields[src], slice(first, first + count), f"{label} [source {src}, rays {first}+{count}]"
        p, s, pol, wl = dev["p"][sl], dev["s"][sl], dev["pol"][sl], dev["wl"][sl]
        ring = f["shape"] in (gr.SRC_CIRCLE, gr.SRC_RING)
        div, d2 = f["divergence"] != gr.DIV_NONE, bool(f["div_2d"])
        # -- p.  Scale: the largest coordinate of the source's points.  Roundings: 4 per sampler coordinate (1 / n, the cell width,
        # the product, the sum), Shirley's map 3 (quotient, its scaling, r * cos), the annulus 5, the rotation 3, + pos 1: <= 16;
        # image sources: px_w, the sum PX + rx, the product, the sum: 4.  Discs and rings go through sincospi_small.
        scale = float(np.abs(o["p"][:, :2]).max())
        tol_p = (16 * EPS + (4 * MEASURED["sincospi_small"] if ring else 0)) * scale
        err = worst(p, o["p"])
        assert err <= tol_p, f"{tag}: p off by {err:.3e} > {tol_p:.3e}"
        assert np.array_equal(p[:, 2], np.full(count, f["pos"][2])), f"{tag}: p_z"
        # -- integer facts behind p
        if "stratum" in o:  # line: the sample lies inside the stratum the permutation assigns (closed by the bound above)
            ang = f.get("angle", 0.0)
            t = (p[:, 0] - f["pos"][0]) * np.cos(ang) + (p[:, 1] - f["pos"][1]) * np.sin(ang)
            cell = 2 * f["r"] / count
            k = o["stratum"]
            assert np.all(t >= -f["r"] + k * cell - tol_p) and np.all(t <= -f["r"] + (k + 1) * cell + tol_p), f"{tag}: stratum"
            assert np.array_equal(np.sort(k), np.arange(count)), f"{tag}: the strata are no permutation"
        if "pixel" in o:  # the jitter is centred: at least 2^-17 of a pixel away from every edge, so floor() is exact
            W, H = f["img_w"], f["img_h"]
            PX = np.floor((p[:, 0] - (f["pos"][0] - f["dim"][0] / 2)) / (f["dim"][0] / W)).astype(int)
            PY = np.floor((p[:, 1] - (f["pos"][1] - f["dim"][1] / 2)) / (f["dim"][1] / H)).astype(int)
            assert np.array_equal(PY * W + PX, o["pixel"]), f"{tag}: pixel"
            assert np.all(np.asarray(f["img_pdf"])[o["pixel"]] > 0), f"{tag}: a dark pixel emitted"
        # -- s.  Scale 1.  No divergence: the normalisation of a converging direction (3 products, 2 sums, rsqrt, product: 7) or
        # the constant itself (0).  With divergence: the sampler pair 8, Shirley's quotient 2, (sin, cos) of theta 4, the frame
        # (difference, 3 + 2 for each norm, 2 x rsqrt, 2 products each: 14, the cross product 9) and the combination
        # ct s_or + st (ca sx + sa sy): 6 -> <= 48; an error d of theta or alpha moves s by at most d.  Tabulated divergence adds
        # the table's own condition (s_extra, from the replay); function orientations the float64 evaluation of or_func (3 products,
        # 5 sums, the norm 4) on positions that are off by tol_p (slopes of 0.03): 12.
        tol_s = 0.0
        if f["orientation"] == gr.OR_CONVERGING:
            tol_s = 8 * EPS
        if f["orientation"] == gr.OR_ARRAY:
            tol_s = 12 * EPS
        if div:
            tol_s = 48 * EPS + 4 * MEASURED["sincos"] + (0 if d2 else 4 * MEASURED["sincospi_small"])
        tol_s = tol_s + o["s_extra"][:, None]
        err_s = np.abs(s.astype(gr.LD) - o["s"])
        assert np.all(err_s <= tol_s), f"{tag}: s off by {float(err_s.max()):.3e}, allowed {float(np.max(tol_s)):.3e}"
        if not div and f["orientation"] == gr.OR_CONSTANT:
            assert np.array_equal(s, np.broadcast_to(np.asarray(f["s"], dtype=np.float64), s.shape)), f"{tag}: constant s"
        # -- wl: float32 storage
        if f["shape"] == gr.SRC_IMAGE_RGB:
            # inside the ray's bucket of the 65536-bucket inverse table, edges from the definition; the device interpolates a
            # monotone function linearly inside it.  Slack: the float32 rounding and 8 eps of the wavelength.
            lo, hi = o["wl_bucket"]
            slack = ulp32(hi) / 2 + 8 * EPS * 780.
            wld = wl.astype(gr.LD)
            assert np.all(wld >= lo - slack) and np.all(wld <= hi + slack), \
                f"{tag}: RGB wl outside its bucket by {float(np.maximum(lo - wld, wld - hi).max()):.3e}"
        elif f["spectrum"] in (gr.SPEC_MONO, gr.SPEC_LINES):
            assert np.array_equal(wl, o["wl"].astype(np.float64).astype(np.float32)), f"{tag}: wl (exact)"
        else:
            tol = ulp32(o["wl"]) / 2 + o["wl_bound"]  # half a float32 ulp + the float64 chain (counted in the replay)
            err_wl = np.abs(wl.astype(gr.LD) - o["wl"])
            assert np.all(err_wl <= tol), f"{tag}: wl off by {float((err_wl / ulp32(o['wl'])).max()):.3f} float32 ulps"
        # -- pol: float32 storage.  Float64 chain: (cos, sin) of the angle, ps (2 products), A_ts / A_tp (3 each), pp (cross: 9),
        # the combination (3 per component): <= 24 on scale 1, plus the condition of 1 / (sqrt(1 - s_z^2) + 1e-16) at the ray's own
        # s_z: an error e of s_z moves 1 - s_z^2 by 2 e, so fa (and with it ps, pp) relatively by e / (1 - s_z^2), e <= tol_s + eps.
        if no_pol:
            continue
        q2 = np.maximum(rep["pol_q2"][sl], 1e-300)
        e_s = np.max(tol_s * np.ones((count, 3)), axis=1) + EPS
        tol64 = 24 * EPS + 4 * max(MEASURED.values()) + o["pol_cond"] + 4 * e_s / q2
        tol_pol = ulp32(o["pol"]) / 2 + tol64[:, None]
        err_pol = np.abs(pol.astype(gr.LD) - o["pol"])
        assert np.all(err_pol <= tol_pol), f"{tag}: pol off by {float((err_pol / ulp32(o['pol'])).max()):.3f} float32 ulps"


def run_case(sources, ranges, seed, no_pol, label, powers=None, or_funcs=None):
    """replay (near == 0 from the replay alone), then the device, then ray by ray"""
    fields = fields_of(sources, powers)
    s_or_rep = s_or_dev = None
    if or_funcs:  # orientation "Function": or_func at the replayed positions (longdouble) and, for the device, at its own
        pre = gr.replay(fields, ranges, seed, True)
        assert pre["near"] == 0
        pre_dev = device_rays(sources, ranges, seed, True, powers)
        s_or_rep, s_or_dev = {}, {}
        for i, fn in or_funcs.items():
            (first, count), = [(r[1], r[2]) for r in ranges if r[0] == i]
            sl = slice(first, first + count)
            s_or_rep[i] = fn(pre["p"][sl, 0], pre["p"][sl, 1])
            s_or_dev[i] = fn(pre_dev["p"][sl, 0], pre_dev["p"][sl, 1])
    rep = gr.replay(fields, ranges, seed, no_pol, s_or_rep, X_DEF)
    assert rep["near"] == 0, f"{label}: {rep['near']} rays within {gr.NEAR} eps of a node or edge: choose another seed"
    dev = device_rays(sources, ranges, seed, no_pol, powers, s_or_dev)
    check_rays(dev, rep, fields, no_pol, label)
    return dev, rep


def source_ranges(n):
    """the ranges RayStorage._source_ranges cuts the n rays of a single source into"""
    return [(0, first, count, 0.0) for first, count in stratification_blocks(0, n, 64)]


# ---- strata and permutations --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [77, HI_SEED])
@pytest.mark.parametrize("n", [1, 2, 3, 4, 63, 64, 65, 1000, 4096, 65535, 65536 + 1000, 1 << 20])
def test_strata_and_permutations(n, seed):
    """One Line source, no divergence, monochromatic: every ray's stratum is the keyed permutation's, in every size class of
    permute_index (one sample, ragged with cycle walking, powers of two, a cut range, permute_pow2_large at 2^20)."""
    rs = ot.RaySource(ot.Line(r=2.5, angle=30), pos=[0.5, -1.0, 2.0], divergence="None", s=[0, 0, 1],
                      spectrum=ot.LightSpectrum("Monochromatic", wl=550.123), polarization="x")
    ranges = source_ranges(n)
    assert len(ranges) == (2 if n == 65536 + 1000 else 1)
    run_case([rs], ranges, seed, False, f"line n={n}")


# ---- every arm of generate_ray ----------------------------------------------------------------------------------------------
def _rect25():
    s = ot.RectangularSurface(dim=[2.0, 3.5])
    s.rotate(25)
    return s


def _div_func(x):
    return np.cos(x) ** 2 + 0.2


def _pol_func(x):
    return 1.2 + np.sin(2 * x)


def _or_func(x, y):
    """a smooth field of unit vectors leaning away from the axis (slopes of 0.02 per mm: the float64 rounding of the positions
    does not show)"""
    v = np.stack([0.02 * x + 0.1, -0.03 * y + 0.05, 1 + 0 * x], axis=1)
    return v / np.sqrt((v * v).sum(axis=1))[:, None]


TILT = [0.12, -0.2, 0.97]
LINES = dict(lines=[450., 486.13, 550., 610.5, 680.], line_vals=[1, 2, 0, 1, 0.5])


def _sources():
    LS, RS = ot.LightSpectrum, ot.RaySource
    d65, bb = ot.presets.light_spectrum.d65, LS("Blackbody", T=5000.)
    rgb = ot.RGBImage(scenes.synthetic_rgb_image(), [4.0, 3.0])
    grey = ot.GrayscaleImage(scenes.synthetic_gray_image(), [2.0, 2.5])
    return {
        "S01": (RS(ot.Point(), pos=[0.5, -1, 2], divergence="None", s=TILT, polarization="Constant", pol_angle=30.,
                   spectrum=LS("Monochromatic", wl=550.123)), False, None),
        "S02": (RS(ot.Point(), pos=[0.5, -1, 2], divergence="Lambertian", div_angle=20., orientation="Converging",
                   conv_pos=[1.5, 0.5, 12.], polarization="Uniform", spectrum=LS("Rectangle", wl0=420., wl1=680.)), False, None),
        "S03": (RS(ot.Point(), pos=[0, 0, 0], divergence="Isotropic", div_angle=15., div_2d=True, div_axis_angle=35., s=TILT,
                   polarization="List", pol_angles=[0., 45., 80., 135.], pol_probs=[1., 0., 2., 0.5], spectrum=LS("Lines", **LINES)),
                False, None),
        "S04": (RS(ot.Line(r=2.5, angle=30), pos=[0, 1, -3], divergence="Function", div_func=_div_func, div_angle=25., s=TILT,
                   polarization="Function", pol_func=_pol_func, spectrum=LS("Gaussian", mu=550., sig=80.)), False, None),
        "S05": (RS(ot.CircularSurface(r=2.0), pos=[1, 2, 0], divergence="Isotropic", div_angle=30., s=[0, 0, 1], spectrum=d65),
                True, None),
        "S06": (RS(ot.RingSurface(r=3.0, ri=1.0), pos=[-1, 0.5, 4], divergence="Lambertian", div_angle=40., div_2d=True,
                   div_axis_angle=-50., s=TILT, polarization="x", spectrum=d65), False, None),
        "S07": (RS(_rect25(), pos=[1.5, -2, 3], divergence="Function", div_func=_div_func, div_angle=10., div_2d=True,
                   div_axis_angle=70., orientation="Converging", conv_pos=[0.5, 0.2, 30.], polarization="Uniform", spectrum=bb),
                False, None),
        "S08": (RS(_rect25(), pos=[1.5, -2, 3], divergence="Isotropic", div_angle=12., orientation="Function", or_func=_or_func,
                   polarization="List", pol_angles=[10., 100.], spectrum=LS("Rectangle", wl0=500., wl1=501.)), False, _or_func),
        "S09": (RS(ot.Line(r=2.5, angle=30), pos=[0, 1, -3], divergence="None", orientation="Function", or_func=_or_func,
                   polarization="Function", pol_func=_pol_func, spectrum=LS("Lines", **LINES)), False, _or_func),
        "S10": (RS(ot.CircularSurface(r=2.0), pos=[1, 2, 0], divergence="None", orientation="Converging", conv_pos=[0, 0, 25.],
                   polarization="Constant", pol_angle=75., spectrum=d65), False, None),
        "S11": (RS(rgb, pos=[0.3, -0.2, 1], divergence="Lambertian", div_angle=20., s=TILT, polarization="Uniform"), False, None),
        "S12": (RS(grey, pos=[0, 0, -2], divergence="Isotropic", div_angle=8., div_2d=True, div_axis_angle=20.,
                   orientation="Converging", conv_pos=[0.2, -0.1, 20.], polarization="List", pol_angles=[0., 60., 120.],
                   spectrum=LS("Gaussian", mu=550., sig=80.)), False, None),
        "S13": (RS(ot.RingSurface(r=3.0, ri=1.0), pos=[-1, 0.5, 4], divergence="Function", div_func=_div_func, div_angle=25.,
                   orientation="Converging", conv_pos=[0, 0, 40.], spectrum=bb), True, None),
        "S14": (RS(ot.Point(), pos=[0, 0, 0], divergence="None", s=[0, 0, 1], polarization="Uniform",
                   spectrum=LS("Monochromatic", wl=632.8)), False, None),
        "S15": (RS(rgb, pos=[0.3, -0.2, 1], divergence="None", orientation="Converging", conv_pos=[0, 0, 15.]), True, None),
        "S16": (RS(grey, pos=[0, 0, -2], divergence="Function", div_func=_div_func, div_angle=25., s=TILT,
                   polarization="Function", pol_func=_pol_func, spectrum=d65), False, None),
    }


ARMS = [(name, n) for name in (f"S{i:02d}" for i in range(1, 17)) for n in (1000, 4096)] + \
       [(name, n) for name in ("S02", "S07") for n in (1, 3)]


@pytest.fixture(scope="module")
def sources():
    with ot.global_options.no_warnings():
        return _sources()


@pytest.mark.parametrize("name, n", ARMS)
def test_every_arm(sources, name, n):
    rs, no_pol, orf = sources[name]
    run_case([rs], source_ranges(n), 77 if n != 4096 else HI_SEED, no_pol, f"{name} n={n}", or_funcs={0: orf} if orf else None)


# ---- image sources -------------------------------------------------------------------------------------------------------------
def _images():
    """the images of test_gpu_sources.py::test_pixel_pick_edge_cases and the synthetic test card; widths 1, 2, 23, 64, 31, 32"""
    rng = np.random.default_rng(3)
    out = {"one_pixel": (np.full((1, 1, 3), 0.7), False)}
    im = np.zeros((1, 2, 3))
    im[0, 1] = [1, 0.5, 0.2]
    out["dark_next_to_lit"] = (im, False)
    im = rng.uniform(0, 1, (17, 23, 3))
    im[rng.uniform(size=(17, 23)) < 0.6] = 0
    out["mostly_dark_17x23"] = (im, False)
    im = np.full((64, 64, 3), 1e-3)
    im[10, 20] = 1.0
    out["dominant_pixel_64x64"] = (im, False)
    g = rng.uniform(0, 1, (9, 31))
    g[g < 0.3] = 0
    out["grey_9x31"] = (g, True)
    out["test_card"] = (scenes.synthetic_rgb_image(), False)
    return out


IMAGES = _images()


@pytest.mark.parametrize("n", [1000, 4096])
@pytest.mark.parametrize("name", list(IMAGES))
def test_image_sources(name, n):
    """Pixel by searchsorted on cumsum(pdf), row / column by divmod (widths that are no power of two: the reciprocal fix-up),
    centred 16-bit jitter, the primary and its wavelength; 3-D divergence next to the 16-bit slicing of block A."""
    data, grey = IMAGES[name]
    img = ot.GrayscaleImage(data, [2.0, 1.0]) if grey else ot.RGBImage(data, [2.0, 1.0])
    kw = dict(spectrum=ot.LightSpectrum("Rectangle", wl0=500., wl1=600.)) if grey else {}
    with ot.global_options.no_warnings():
        rs = ot.RaySource(img, pos=[0.25, -0.5, 1], divergence="Isotropic", div_angle=10., s=TILT, polarization="Uniform", **kw)
    run_case([rs], source_ranges(n), 5, False, f"image {name} n={n}")


@pytest.mark.parametrize("n", [1000, 4096])
def test_image_source_with_2d_divergence(n):
    """block B (32-bit words) drawn next to the 16-bit halves of block A"""
    with ot.global_options.no_warnings():
        rs = ot.RaySource(ot.RGBImage(IMAGES["mostly_dark_17x23"][0], [2.0, 1.0]), pos=[0.25, -0.5, 1], divergence="Lambertian",
                          div_angle=25., div_2d=True, div_axis_angle=40., s=TILT, polarization="Uniform")
    run_case([rs], source_ranges(n), 5, False, f"image 2-D n={n}")


# ---- range plumbing ----------------------------------------------------------------------------------------------------------------
def _plumbing_sources():
    LS = ot.LightSpectrum
    return [ot.RaySource(ot.Line(r=2.5, angle=30), pos=[0, 1, -3], divergence="None", s=TILT, polarization="Uniform",
                         spectrum=LS("Rectangle", wl0=420., wl1=680.), power=2.0),
            ot.RaySource(ot.CircularSurface(r=2.0), pos=[1, 2, 0], divergence="Isotropic", div_angle=20., s=[0, 0, 1],
                         polarization="x", spectrum=LS("Lines", **LINES)),
            ot.RaySource(ot.Point(), pos=[0.5, -1, 2], divergence="Lambertian", div_angle=20., div_2d=True, div_axis_angle=10.,
                         s=TILT, polarization="List", pol_angles=[0., 60.], spectrum=LS("Monochromatic", wl=550.123), power=0.5)]


def _ranges(n_ranges):
    """Counts cycle through 1, 2, 3, 5, 0, 64, 65, 130, 7 (waves straddle; a zero-count range shares its start with the next
    one), the sources interleave, every fourth range names its ray power, the rest leave it 0 (power / count); the list is
    shuffled before the call."""
    counts = [1, 2, 3, 5, 0, 64, 65, 130, 7]
    out, first = [], 0
    for i in range(n_ranges):
        cnt = counts[i % len(counts)]
        out.append((i % 3, first, cnt, 0.125 if i % 4 == 1 else 0.0))
        first += cnt
    order = np.random.default_rng(11).permutation(n_ranges)
    return [out[i] for i in order]


@pytest.mark.parametrize("n_ranges", [70, 64, 9])
def test_range_plumbing(n_ranges):
    """70 ranges: records in device memory and bisection; 64 and 9: the argument block and locate_range.  The range id that
    keys the permutations is the position after the stable sort by (first, count)."""
    ranges = _ranges(n_ranges)
    assert any(r[2] == 0 for r in ranges) and any(r[1] % 64 for r in ranges)
    empty = [r for r in ranges if r[2] == 0][0]
    assert any(r[1] == empty[1] and r[2] > 0 for r in ranges)  # the zero-count range shares its start
    with ot.global_options.no_warnings():
        srcs = _plumbing_sources()
    dev, rep = run_case(srcs, ranges, HI_SEED, False, f"{n_ranges} ranges")
    assert np.array_equal(np.unique(rep["rid"]), [q for q, r in enumerate(gr.range_ids(ranges)) if r[2]])
    given = np.zeros(dev["w"].shape[0], dtype=bool)
    for src, first, count, ray_power in ranges:
        given[first:first + count] = ray_power > 0
    assert np.all(dev["w"][given] == np.float32(0.125)) and np.all(dev["w"][~given] != np.float32(0.125))


# ---- generation inside the trace kernels ---------------------------------------------------------------------------------------------
def _hurb_polychromatic(ot_, **kw):
    RT = scenes.hurb_slit_lens(ot_, **kw)
    RT.ray_sources[0].spectrum = ot.LightSpectrum("Rectangle", wl0=450., wl1=650.)  # off the discrete-spectrum kernels
    return RT


TRACE_SCENES = {"image_source": scenes.c4_image_render, "tabulated_medium": scenes.mixed_geometry, "hurb": _hurb_polychromatic}


@pytest.mark.parametrize("name", list(TRACE_SCENES))
def test_trace_kernels_generate_the_same_rays(name):
    """Section 0 of a trace (rays generated in registers by the trace kernel of the scene's family) is bit-equal to
    ot_rays_generate with the same seed, table and ranges: p, w, pol and wl.  (The storage keeps no initial direction after a
    trace -- `ot_rays.s` is the final one on return -- and section 1 only holds it through a hit search.)"""
    lib, N, seed = _capi.load_library(), 10_037, 77
    with ot.global_options.no_warnings():
        RT = TRACE_SCENES[name](ot, seed=seed)
        RT.trace(N)
        st = RT.rays
        nt, Np, no_pol = st.Nt, st._Np, RT.no_pol
        got = {"p": st._dev["p"].view(3, nt, Np)[:, 0, :N].cpu().numpy(),
               "w": st._dev["w"].view(nt, Np)[0, :N].cpu().numpy(), "wl": st._dev["wl"][:N].cpu().numpy()}
        if not no_pol:
            got["pol"] = st._dev["pol"].view(3, nt, Np)[:, 0, :N].cpu().numpy()
        tab, rng = st._source_table(seed), st._source_ranges()
        buf = {k: torch.empty(m * N, dtype=dt, device="cuda") for k, m, dt in
               (("p", 3, torch.float64), ("s", 3, torch.float64), ("w", 1, torch.float32), ("n", 1, torch.float64),
                ("wl", 1, torch.float32), ("pol", 3, torch.float32))}
        rays = _capi.Rays()
        rays.N, rays.nt = N, 1
        rays.p, rays.s, rays.w, rays.n, rays.wl = (buf[k].data_ptr() for k in ("p", "s", "w", "n", "wl"))
        rays.pol = None if no_pol else buf["pol"].data_ptr()
        _capi.check(lib.ot_rays_generate(tab.handle, rng, len(rng), seed, int(no_pol), C.byref(rays), stream_ptr()))
        torch.cuda.synchronize()
    for k, a in got.items():
        b = buf[k].cpu().numpy().reshape(a.shape)
        assert np.array_equal(a, b), f"{name}: {k} of section 0 differs from ot_rays_generate at {np.argwhere(a != b)[:4].tolist()}"


# ---- ot.random -----------------------------------------------------------------------------------------------------------------------
def _sampler_ctx(seed, N, identity=False):
    return gr.Ctx(seed, 0, 0, N, True, False, identity=identity)


@pytest.mark.parametrize("shuffle", [True, False])
def test_random_interval(shuffle):
    """ot.random.stratified_interval_sampling: the generator's position stream (kernels of their own build the context)"""
    a, b, N, seed = -1.5, 2.25, 1000, 21
    c = _sampler_ctx(seed, N, identity=not shuffle)
    want = gr.strat_interval(c, gr.ST_POS, a, b)
    got = ot.random.stratified_interval_sampling(a, b, N, shuffle=shuffle, seed=seed)
    assert worst(got, want) <= 4 * EPS * 2.25  # 1 / n, the cell width, the product, the sum


def test_random_rectangle():
    a, b, cc, d, N, seed = -1.0, 3.0, 0.5, 2.0, 1000, 22
    c = _sampler_ctx(seed, N)
    wx, wy, (ix, iy, nx, ny) = gr.strat_rect(c, gr.ST_POS, a, b, cc, d)
    assert c.near == 0
    x, y = ot.random.stratified_rectangle_sampling(a, b, cc, d, N, seed=seed)
    assert worst(x, wx) <= 4 * EPS * 3.0 and worst(y, wy) <= 4 * EPS * 2.0  # as for the interval
    grid = ix >= 0  # the 31^2 cells, exact: the centred dither keeps every sample 2^-33 of a cell away from its edges
    assert grid.sum() == 961 and nx == 31
    assert np.array_equal(np.floor((x[grid] - a) / ((b - a) / nx)).astype(int), ix[grid])
    assert np.array_equal(np.floor((y[grid] - cc) / ((d - cc) / ny)).astype(int), iy[grid])


@pytest.mark.parametrize("polar", [False, True])
def test_random_ring(polar):
    ri, r, N, seed = 1.0, 3.0, 1000, 23
    c = _sampler_ctx(seed, N)
    w0, w1 = gr.strat_ring(c, gr.ST_POS, ri, r, polar)
    assert c.near == 0
    g0, g1 = ot.random.stratified_ring_sampling(ri, r, N, polar=polar, seed=seed)
    # the sampler pair 8, Shirley's quotient and scaling 2, the annulus 5, then r cos / r sin through sincospi_small, or
    # theta = pi * (theta / pi): 1 -- <= 16 on the scale r (of pi for the angle)
    tol = 16 * EPS + 4 * MEASURED["sincospi_small"]
    assert worst(g0, w0) <= tol * r and worst(g1, w1) <= tol * (np.pi if polar else r)


# ---- the functions without a stated accuracy ---------------------------------------------------------------------------------------
def test_function_errors():
    """Measures sincospi_small and sincos against the longdouble replay where they reach a float64 output directly, prints the
    worst figure of each (pytest -s), holds it to 1e-13 and to the recorded figure; erfinv and ot_rcp3 in float32 ulps."""
    LS = ot.LightSpectrum
    worst_of = {"sincospi_small": 0.0, "sincos": 0.0, "erfinv [float32 ulps of wl]": 0.0, "ot_rcp3 [float32 ulps of pol]": 0.0}
    with ot.global_options.no_warnings():
        disc = ot.RaySource(ot.CircularSurface(r=1.0), pos=[0, 0, 0], divergence="Lambertian", div_angle=60., s=[0, 0, 1],
                            polarization="x", spectrum=LS("Gaussian", mu=550., sig=80.))
        fan = ot.RaySource(ot.Point(), pos=[0, 0, 0], divergence="Isotropic", div_angle=80., div_2d=True, div_axis_angle=0.,
                           s=[0, 0, 1], polarization="Uniform", spectrum=LS("Monochromatic", wl=550.))
    for seed in (77, HI_SEED):
        for n in (1000, 4096):
            for rs, key in ((disc, "sincospi_small"), (fan, "sincos")):
                f = fields_of([rs])
                rep = gr.replay(f, source_ranges(n), seed, False, None, X_DEF)
                assert rep["near"] == 0
                dev = device_rays([rs], source_ranges(n), seed, False)
                # disc: p = r (cos, sin)(pi theta) on scale r = 1, s = (st ca, st sa, ct) on scale 1; fan: s = (sin, 0, cos)(theta)
                e = max(worst(dev["p"], rep["p"]), worst(dev["s"], rep["s"])) if key == "sincospi_small" else worst(dev["s"], rep["s"])
                worst_of[key] = max(worst_of[key], e)
                if key == "sincospi_small":
                    u = np.abs(dev["wl"].astype(gr.LD) - rep["wl"]) / ulp32(rep["wl"])
                    worst_of["erfinv [float32 ulps of wl]"] = max(worst_of["erfinv [float32 ulps of wl]"], float(u.max()))
                u = np.abs(dev["pol"].astype(gr.LD) - rep["pol"]) / ulp32(rep["pol"])
                worst_of["ot_rcp3 [float32 ulps of pol]"] = max(worst_of["ot_rcp3 [float32 ulps of pol]"], float(u.max()))
    for k, v in worst_of.items():
        print(f"worst error {k}: {v:.4e}")
    for k in ("sincospi_small", "sincos"):
        assert worst_of[k] <= 1e-13, f"{k}: {worst_of[k]:.3e} relative to its scale -- a finding, not a tolerance"
        assert worst_of[k] <= 4 * MEASURED[k], f"{k}: {worst_of[k]:.3e} against the recorded {MEASURED[k]:.3e}"
    assert worst_of["erfinv [float32 ulps of wl]"] <= 0.5 + 1e-6 and worst_of["ot_rcp3 [float32 ulps of pol]"] <= 0.5 + 1e-6
