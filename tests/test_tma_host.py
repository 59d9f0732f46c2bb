"""Paraxial analysis (ot.TMA, Lens.tma, Group.tma, Raytracer.tma) against the reference's recorded results
(tests/golden/tma.npz, written by tests/golden/generate_golden_tma.py from tests/scenes_tma.py and tests/tma_cases.py).
Host only: no test here needs a device.

Tolerances.  abcd: 1e-13 of max |abcd| (the project's value tolerance for leaf quantities); derived scalars and method
results: rtol 1e-12; quantities that are differences of z positions (ffl, bfl, d, the focal lengths in both definitions)
additionally atol 1e-12 times the largest |z| among the cardinal and vertex points.  The reference evaluated twice (lens
list reversed; wl as int) agrees with itself exactly -- the generator prints 0 for abcd and 0 for the derived values, for
the near-afocal telescope as well -- so these bounds are more than 10 x above its own deviation, and the telescope needs
no tolerance of its own.
"""
import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd.base import mutation_epoch
from optrace_amd.tma import index_at

import scenes
import scenes_tma as st
import tma_cases
from helpers import load, assert_close

ATTRS = ("wl", "vertex_points", "n1", "n2", "abcd", "principal_points", "nodal_points", "focal_points", "focal_lengths",
         "ffl", "bfl", "d", "efl", "efl_n", "focal_lengths_n", "powers", "powers_n", "optical_center")
POINT_METHODS = ("image_position", "image_magnification", "object_position", "object_magnification")
Z_DIFFERENCES = ("ffl", "bfl", "d", "focal_lengths", "efl", "efl_n", "focal_lengths_n")
RTOL, ABCD_TOL = 1e-12, 1e-13


@pytest.fixture(scope="module")
def golden():
    g = load("tma.npz")
    return g, st.unpack(g, "sys")


def same_specials(a, b, what):
    """NaN and infinities (with their sign) in the same places."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    special = ~np.isfinite(a) | ~np.isfinite(b)
    assert np.array_equal(a[special], b[special], equal_nan=True), (what, a, b)


def close(a, b, what, atol=0.0):
    same_specials(a, b, what)
    assert_close(a, b, rtol=RTOL, atol=atol, what=what)


with ot.global_options.no_warnings():
    SYSTEMS = list(st.systems(ot))


def test_fixture_lists_these_systems(golden):
    assert [str(s) for s in golden[1]["systems"]] == SYSTEMS


@pytest.mark.parametrize("name", SYSTEMS)
def test_attributes_and_methods_match_reference(golden, name):
    _, g = golden
    with ot.global_options.no_warnings():
        tma, lenses = st.analysis(ot, st.systems(ot)[name])
    ref = {k[len(name) + 1:]: v for k, v in g.items() if k.startswith(name + "/")}

    # attributes: names, types, values
    z_scale = max([abs(v) for k in ("vertex_points", "principal_points", "nodal_points", "focal_points")
                   for v in ref[f"attr/{k}"] if np.isfinite(v)], default=0.)
    for attr in ATTRS:
        v = getattr(tma, attr)
        assert type(v).__name__ == str(ref[f"type/{attr}"]), (attr, type(v))
        if isinstance(v, tuple):
            assert len(v) == 2 and all(type(e) is float for e in v), (attr, v)
        if attr == "abcd":
            assert v.shape == (2, 2) and v.dtype == np.float64
            same_specials(v, ref["attr/abcd"], "abcd")
            assert np.abs(v - ref["attr/abcd"]).max() <= ABCD_TOL * np.abs(ref["attr/abcd"]).max()
        else:
            close(v, ref[f"attr/{attr}"], attr, atol=RTOL * z_scale if attr in Z_DIFFERENCES else 0.)

    # methods, at the recorded arguments (which are the ones scenes_tma.arguments gives here)
    args = st.arguments(lenses)
    for key in ("z", "zz", "zs"):
        assert np.array_equal(args[key], ref[key]), key
    with np.errstate(all="ignore"):
        for method in POINT_METHODS:
            for z, want, err in zip(ref["z"], ref[method], ref[f"err/{method}"]):
                if str(err) != "none":
                    with pytest.raises(Exception) as info:
                        getattr(tma, method)(float(z))
                    assert type(info.value).__name__ == str(err), (method, z)
                    continue
                got = getattr(tma, method)(float(z))
                assert type(got) is float
                close(got, want, f"{method}({z})")
        for (zg, zb), want in zip(ref["zz"], ref["matrix_at"]):
            got = tma.matrix_at(float(zg), float(zb))
            assert isinstance(got, np.ndarray) and got.shape == (2, 2)
            same_specials(got, want, f"matrix_at({zg}, {zb})")
            fin = np.isfinite(want)
            assert np.all(np.abs(got - want)[fin] <= RTOL * np.abs(want[fin]).max(initial=0.)), (zg, zb, got, want)
        for zs, pos, mag in zip(ref["zs"], ref["pupil_position"], ref["pupil_magnification"]):
            got_p, got_m = tma.pupil_position(float(zs)), tma.pupil_magnification(float(zs))
            for got in (got_p, got_m):
                assert type(got) is tuple and len(got) == 2 and all(type(e) is float for e in got)
            close(got_p, pos, f"pupil_position({zs})")
            close(got_m, mag, f"pupil_magnification({zs})")


def test_special_cases_are_in_the_fixture(golden):
    """What the comparison above covers: exact afocal plate, empty list, infinite results, all four pupil paths."""
    _, g = golden
    assert g["plate/attr/abcd"][1, 0] == 0.0 and np.all(np.isnan(g["plate/attr/focal_points"]))
    assert np.isnan(g["plate/attr/optical_center"]) and np.isnan(g["plate/attr/efl"])
    assert np.array_equal(g["empty/attr/abcd"], np.eye(2)) and np.all(np.isnan(g["empty/attr/vertex_points"]))
    assert g["telescope/attr/abcd"][1, 0] != 0 and abs(g["telescope/attr/efl"]) > 1e4
    assert any(np.isinf(g[f"{s}/matrix_at"]).any() for s in SYSTEMS)
    assert any((g[f"{s}/err/image_position"] == "ValueError").any() for s in SYSTEMS)
    trio = g["trio/list/555/zs"]
    v1, v2 = g["trio/list/555/attr/vertex_points"]
    assert (trio < v1).any() and (trio > v2).any() and ((trio > v1) & (trio < v2)).sum() >= 4  # inside lenses, in gaps


def test_error_and_argument_cases(golden):
    g, _ = golden
    with ot.global_options.no_warnings():
        cases = tma_cases.cases(ot)
        assert sorted(f"raises/{k}" for k in cases) == sorted(k for k in g.files if k.startswith("raises/"))
        for name, case in cases.items():
            assert tma_cases.outcome(case) == str(g[f"raises/{name}"]), name
    recorded = {str(g[k]) for k in g.files if k.startswith("raises/")}
    assert {"none", "RuntimeError", "ValueError", "TypeError", "AttributeError"} <= recorded


@pytest.mark.parametrize("name", list(scenes.MEDIA))
def test_host_index_matches_reference(name):
    """`tma.index_at` (float64, host) against the reference's n for every model (leaf_media.npz; its wavelengths are
    float32 numbers, exact in float64).  The formulas are a few float64 operations; pow() of whole-number exponents may
    differ in the last bits between array and scalar evaluation, hence 1e-14, a hundredth of what the analysis is held to."""
    media = load("leaf_media.npz")
    ri = ot.RefractionIndex(name.split("_")[0], **scenes.MEDIA[name])
    got = np.array([index_at(ri, float(wl)) for wl in media["wl"]])
    assert_close(got, media[f"n/{name}"], rtol=1e-14, what=name)


def test_host_index_errors():
    with pytest.raises(RuntimeError):  # outside the table
        index_at(ot.RefractionIndex("Data", wls=np.linspace(400., 700., 31), vals=np.full(31, 1.5)), 390.)
    with pytest.raises(RuntimeError):  # n < 1
        index_at(ot.RefractionIndex("Cauchy", coeff=[0.9, 0., 0., 0.]), 555.)
    with pytest.raises(TypeError):
        index_at(ot.RefractionIndex("Cauchy"), 555.)
    with pytest.raises(TypeError):
        index_at(ot.RefractionIndex("Abbe", n=1.5), 555.)


def _lens(z=0.):
    return ot.Lens(ot.SphericalSurface(r=3, R=20), ot.SphericalSurface(r=3, R=-20), de=0.2,
                   n=ot.RefractionIndex("Abbe", n=1.6, V=40.), pos=[0, 0, z])


def test_locked_after_construction():
    tma = _lens().tma()
    for attr in ("wl", "abcd", "efl", "vertex_points"):
        with pytest.raises(RuntimeError):
            setattr(tma, attr, 1.)
    with pytest.raises(AttributeError):
        tma.something_new = 1.
    with pytest.raises(ValueError):
        tma.abcd[0, 0] = 2.  # (arrays of a locked object are read-only)
    tma.desc = "still allowed, like for every locked object"


def test_is_a_snapshot():
    L = _lens()
    G = ot.Group([L, _lens(15.)])
    tma = G.tma()
    before = (tma.vertex_points, tma.focal_points, tma.abcd.copy(), tma.pupil_position(8.), tma.image_position(-50.))
    L.move_to([0, 0, -20])
    G.lenses[1].n2 = ot.RefractionIndex("Constant", n=1.3)
    G.remove(G.lenses[1])
    after = (tma.vertex_points, tma.focal_points, tma.abcd.copy(), tma.pupil_position(8.), tma.image_position(-50.))
    assert before[:2] == after[:2] and np.array_equal(before[2], after[2]) and before[3:] == after[3:]
    assert G.tma().vertex_points != tma.vertex_points


def test_an_analysis_is_no_scene_change():
    """Host part: nothing about a TMA reaches the change counter that `Raytracer.trace`'s shortcut compares."""
    RT = ot.Raytracer(outline=[-5, 5, -5, 5, -10, 60], n0=ot.RefractionIndex("Constant", n=1.1))
    RT.add([_lens(), _lens(15.)])
    G = ot.Group([_lens()])
    e0 = mutation_epoch()
    tmas = [RT.tma(), RT.tma(600.), G.tma(), RT.lenses[0].tma(n0=RT.n0), ot.TMA(RT.lenses, n0=RT.n0, desc="x")]
    tmas[0].desc = "a description"
    tmas[0].image_position(-100.), tmas[0].pupil_position(3.), tmas[0].matrix_at(-5., 40.)
    assert mutation_epoch() == e0
    assert not any(RT.has(t) if isinstance(t, ot.Lens) else False for t in tmas) and len(RT.lenses) == 2
    RT.lenses[0].move_to([0, 0, -1])   # (the counter works)
    assert mutation_epoch() > e0


def test_callers_pass_their_medium():
    n0 = ot.RefractionIndex("Constant", n=1.33)
    RT = ot.Raytracer(outline=[-5, 5, -5, 5, -10, 60], n0=n0)
    L = _lens()
    RT.add(L)
    assert isinstance(RT.tma(), ot.TMA) and RT.tma().n1 == 1.33 and ot.Group([L], n0=n0).tma().n1 == 1.33
    assert L.tma().n1 == 1.0 and L.tma(n0=n0).n1 == 1.33 and L.tma(600.).wl == 600.
    assert RT.tma().abcd.tolist() == ot.TMA([L], n0=n0).abcd.tolist() == L.tma(555., n0).abcd.tolist()
    assert type(RT.tma(wl=500).wl) is int


@pytest.mark.parametrize("name", ["biconvex/media/486", "trio/list/555", "double_gauss/656", "eye/near", "ideal/n2",
                                  "telescope"])
def test_consistency(name):
    with ot.global_options.no_warnings():
        tma, _ = st.analysis(ot, st.systems(ot)[name])
    A, B, C, D = tma.abcd.ravel()
    # a product of k unimodular-times-index-ratio factors: a few ulp per factor of the largest product term
    assert abs(A * D - B * C - tma.n1 / tma.n2) <= 1e-13 * max(abs(A * D), abs(B * C), 1.)
    v1, v2 = tma.vertex_points
    span = max(abs(v1), abs(v2), abs(tma.efl))
    for z in (v1 - 300., v1 - 40., v1 - 1.5):
        zb = tma.image_position(z)
        if v1 < zb < v2:
            continue  # (image inside the system: object_position refuses it)
        back = tma.object_position(zb)
        # two Moebius maps, each good to a few ulp of the quantities it subtracts (|z|, |zb|, efl)
        assert abs(back - z) <= 1e-11 * max(abs(z), abs(zb), span) * max(1., abs((z - v1) / tma.efl)), (z, zb, back)
        M = tma.matrix_at(z, zb)
        assert abs(M[0, 1]) <= 1e-12 * max(abs(z), abs(zb), span), (z, zb, M)
        assert abs(M[0, 0] - tma.image_magnification(z)) == 0.
        assert abs(tma.object_magnification(zb) - M[0, 0]) <= 1e-9 * abs(M[0, 0])
