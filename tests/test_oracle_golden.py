"""Pins the CPU oracle (oracle/oracle.c) and the host scene flattening against golden vectors produced by
the reference itself (tests/golden/generate_golden.py).  CPU only.

Bars (BASELINE.json north_star): hit masks / counters bit-exact; positions, directions 1e-6 relative
(we check far tighter: the oracle follows the reference's operation order); weights / polarisation to
float32 rounding; images 1e-4 in image norm.
"""
import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd.scene import CompiledScene

import oracle_bridge as ob
import scenes
import wavelength_cases as wc
from helpers import load, assert_close, sparse_to_dense, image_rel_l1

@pytest.fixture(scope="module")
def zoo():
    with ot.global_options.no_warnings():
        return scenes.surface_zoo(ot)


@pytest.fixture(scope="module")
def leaf():
    return load("leaf_surfaces.npz")


SURFACE_NAMES = ["circle", "ring", "rect", "rect_rot", "slit", "slit_rot", "sphere_pos", "sphere_neg",
                 "conic_m025", "conic_m75", "conic_p3", "conic_parab", "asphere_a", "asphere_b"]


@pytest.mark.parametrize("name", SURFACE_NAMES)
def test_host_surface_parameters_match_reference(zoo, leaf, name):
    """z_min/z_max/pos as the reference computes them: these feed every kernel."""
    sf = zoo[name]
    assert sf.z_min == float(leaf[f"{name}/param/z_min"])
    assert sf.z_max == float(leaf[f"{name}/param/z_max"])
    assert np.array_equal(sf.pos, leaf[f"{name}/param/pos"])
    if f"{name}/param/angle" in leaf and hasattr(sf, "_angle"):
        assert sf._angle == float(leaf[f"{name}/param/angle"])


@pytest.mark.parametrize("name", SURFACE_NAMES)
def test_oracle_find_hit(zoo, leaf, name):
    sd = zoo[name]._desc()
    ph, hit, ill, st = ob.find_hit(sd, leaf[f"{name}/p"], leaf[f"{name}/s"])
    assert st == 0
    assert np.array_equal(hit, leaf[f"{name}/is_hit"]), "hit mask must be bit-exact"
    assert np.array_equal(ill, leaf[f"{name}/ill"]), "ill-conditioned mask must be bit-exact"
    assert_close(ph, leaf[f"{name}/p_hit"], rtol=1e-13, atol=1e-13, what=f"{name} p_hit")


@pytest.mark.parametrize("name", SURFACE_NAMES)
def test_oracle_mask_values_normals(zoo, leaf, name):
    sd = zoo[name]._desc()
    x, y = leaf[f"{name}/x"], leaf[f"{name}/y"]
    assert np.array_equal(ob.mask(sd, x, y), leaf[f"{name}/mask"])
    assert_close(ob.values(sd, x, y), leaf[f"{name}/values"], rtol=1e-14, atol=1e-15, what=f"{name} values")
    assert_close(ob.normals(sd, x, y), leaf[f"{name}/normals"], rtol=1e-12, atol=1e-14, what=f"{name} normals")


@pytest.mark.parametrize("name", ["ring", "slit", "slit_rot"])
def test_oracle_hurb_props(zoo, leaf, name):
    sd = zoo[name]._desc()
    a_, b_, b, inside = ob.hurb_props(sd, leaf[f"{name}/x"], leaf[f"{name}/y"])
    assert np.array_equal(inside, leaf[f"{name}/hurb_inside"])
    assert_close(a_, leaf[f"{name}/hurb_a"], rtol=1e-13, atol=1e-15, what="a_")
    assert_close(b_, leaf[f"{name}/hurb_b"], rtol=1e-13, atol=1e-15, what="b_")
    assert_close(b, leaf[f"{name}/hurb_bvec"], rtol=1e-13, atol=1e-15, what="b")


@pytest.fixture(scope="module")
def media():
    return load("leaf_media.npz")


@pytest.mark.parametrize("name", list(scenes.MEDIA.keys()))
def test_oracle_refraction_index(media, name):
    ri = ot.RefractionIndex(name.split("_")[0], **scenes.MEDIA[name])
    pool: list = []
    md = ri._desc(pool)
    n = ob.refraction_index(md, np.array(pool), media["wl"])
    # basic IEEE ops are reproduced exactly; pow() for |exponent| >= 3 may differ in the last bits
    assert_close(n, media[f"n/{name}"], rtol=4e-16 if name in ("Constant", "Abbe", "Abbe_lines", "Data") else 1e-14,
                 what=name)


def test_oracle_transmission(media):
    for name, t in scenes.transmission_zoo(ot).items():
        pool: list = []
        fd = t._desc(pool, None)
        T = ob.filter_T(fd, np.array(pool), media["wl"])
        if not name.startswith("Gaussian"):
            assert_close(T, media[f"T/{name}"], rtol=1e-15, atol=0, what=name)
            continue
        # float32 around one expf (wavelength_cases, THE BARS): oracle and reference are each within the bar of
        # fl32(val32 exp(q)), q from float32 basic operations and exp to 64 bits here -- in float32 units of T, also where
        # the filter is inverse (1 - T; the reference rounds that once more, 2^-25)
        bar = wc.gaussian_bar(load("wavelength_step.npz"))
        q = wc.gaussian_q(media["wl"], t.mu, t.sig).astype(np.longdouble)
        truth = (np.longdouble(np.float32(t.val)) * np.exp(q)).astype(np.float32)
        for what, got in (("oracle", T), ("reference", media[f"T/{name}"])):
            Tg = (1 - np.asarray(got, dtype=np.float64)) if t.inverse else np.asarray(got, dtype=np.float64)
            err = np.abs(Tg - truth.astype(np.float64))
            assert np.all(err <= bar * np.spacing(truth).astype(np.float64) + (2.0 ** -25 if t.inverse else 0)), (name, what, float(err.max()))


def test_oracle_observers(media):
    xyz = ob.observers(media["obs/wl"])
    assert_close(xyz, media["obs/xyz"], rtol=1e-15, atol=0, what="observers")


def test_oracle_binning(media):
    xi, yi, wm = ob.binning(media["bin/x"], media["bin/y"], media["bin/w"], 945, 315, media["bin/extent"])
    assert np.array_equal(xi, media["bin/xi"])
    assert np.array_equal(yi, media["bin/yi"])
    assert np.array_equal(wm, media["bin/wm"])


# --------------------------------------------------------------------------------------------------------
TRACES = list(scenes.SCENES.keys()) + ["double_gauss_nopol", "asphere_nopol"] + list(scenes.SCENES2.keys()) + list(scenes.SCENES3.keys())
ALL_SCENES = {**scenes.SCENES, **scenes.SCENES2, **scenes.SCENES3}


def build(name):
    no_pol = name.endswith("_nopol")
    base = name[:-6] if no_pol else name
    with ot.global_options.no_warnings():
        return ALL_SCENES[base][0](ot, **({"no_pol": True} if no_pol else {}))


def oracle_trace(name):
    g = load(f"trace_{name}.npz")
    RT = build(name)
    RT._geometry_checks()
    assert not RT.geometry_error
    sc = CompiledScene(RT)
    N = int(g["N"])
    rays = ob.HostRays(N, sc.nt, RT.no_pol)
    rays.set_initial(g["p0"], g["s0"], g["pol0"] if not RT.no_pol else None, g["w0"], g["wl"])
    hn = g["hurb_normals"] if "hurb_normals" in g else None
    msgs, st = ob.trace(sc.desc, rays, hn)
    assert st == 0
    return g, RT, sc, rays, msgs


@pytest.mark.parametrize("name", TRACES)
def test_oracle_trace(name):
    g, RT, sc, rays, msgs = oracle_trace(name)
    assert sc.nt == g["p_list"].shape[1]
    assert np.array_equal(msgs, g["msgs"]), f"counters differ:\n{msgs}\n{g['msgs']}"
    # alive masks per section bit-exact
    assert np.array_equal(rays.w_list > 0, g["w_list"] > 0)
    # "freeform" holds a FunctionSurface2D, which this framework carries as a spline table (the reference calls
    # the Python function per ray): agreement there is bounded by the tabulation residual, not by rounding
    tab = name in ("freeform", "masked")
    assert_close(rays.p_list, g["p_list"], rtol=1e-12, atol=1e-7 if tab else 1e-12, what="p_list")
    assert_close(rays.n_list, g["n_list"], rtol=1e-14, what="n_list")
    # float32 storage rounding; scenes with a float32-evaluated Gaussian filter (spectrum.py:113) or a
    # host-tabulated "Function" spectrum get the north-star bar of 1e-6
    loose = name.startswith(("asphere", "mixed", "freeform", "masked"))
    assert_close(rays.w_list, g["w_list"], rtol=1e-6 if loose else 2e-7, atol=1e-15 if loose else 1e-30, what="w_list")
    assert_close(rays.s_final, g["s_final"], rtol=1e-11, atol=1e-8 if tab else 1e-13, what="s_final")
    if not RT.no_pol:
        assert_close(rays.pol_list, g["pol_list"], rtol=1e-5, atol=2e-7, what="pol_list")


@pytest.mark.parametrize("name", ["c1_single_lens", "double_gauss", "mixed_geometry", "arizona_eye", "asphere"])
def test_oracle_detector(name):
    g = load(f"trace_{name}.npz")
    RT = build(name)
    rays = ob.HostRays.from_lists(g["p_list"], g["w_list"], g["wl"])
    for di, det in enumerate(RT.detectors):
        projs = [None] if not isinstance(det.surface, ot.SphericalSurface) else \
            ["Equidistant", "Orthographic", "Equal-Area", "Stereographic"]
        for proj in projs:
            key = f"det{di}/{proj}"
            ph, hw, ext, ill, st = ob.detector_hits(rays, 0, rays.N, det.surface._desc(), _capi.PROJECTIONS[proj])
            assert st == 0
            sel = hw > 0
            assert np.count_nonzero(sel) == g[f"{key}/w"].shape[0], "number of detector hits must be exact"
            assert np.array_equal(hw[sel], g[f"{key}/w"])
            assert_close(ph[sel], g[f"{key}/ph"], rtol=1e-9, atol=1e-11, what=f"{key} ph")
            assert ill == int(g[f"{key}/ill"])
            if np.any(sel):
                assert_close(ext, g[f"{key}/extent"], rtol=1e-9, atol=1e-11, what="extent")
            # render with the reference's (fixed-up) extent
            ref = sparse_to_dense(g, f"{key}/img")
            Ny, Nx = ref.shape[:2]
            img = ob.render(ph[sel, 0], ph[sel, 1], hw[sel], g["wl"][sel], g[f"{key}/img/extent"], Nx, Ny)
            assert abs(img[..., 3].sum() - float(g[f"{key}/img/power"])) <= 1e-12 * float(g[f"{key}/img/power"])
            assert np.all(image_rel_l1(img, ref) < 1e-4), image_rel_l1(img, ref)
