"""Chromatic analysis without a device: the longdouble definition (tests/chromatic_cases.py) on hand-made storages whose answers
are known by inspection, the argument checks of `Raytracer.chromatic_analysis` and of the `ot_chromatic_*` entry points, which come
before any device call, the host-only parts of `ot.ChromaticAnalysis`, and one physical pin: the definition on rays the C oracle
traced through a dispersive single lens, against the paraxial image position per spectral line."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd import chromatic as chrom

import chromatic_cases as cc

NAN = np.nan
LD = cc.LD
F64 = lambda a: np.asarray(a).astype(np.float64)


# ---- hand-made storages: two sections, section 0 analysed ---------------------------------------------------------------------------
def through(point, starts, reach=2.0):
    """Rays from `starts` (n, 3) through `point`: p (n, 2, 3) with p[:, 1] = start + reach (point - start).  With dyadic numbers
    every difference is exact."""
    starts, point = np.asarray(starts, dtype=np.float64), np.asarray(point, dtype=np.float64)
    return np.stack([starts, starts + reach * (point - starts)], axis=1)


FA, FB = np.array([0.5, -0.25, 10.0]), np.array([0.75, 0.25, 12.0])
CROSS = np.array([[1.0, 0, 0], [-1.0, 0, 0], [0, 1.0, 0], [0, -1.0, 0]])


def two_bands():
    """Band 0 (486 nm) through FA, band 1 (656 nm) through FB, four rays each about a chief ray along z; ray 8 is dead and has no
    position; ray 9 (656 nm) runs through FB within the plane z = 12: it takes part in the focus and crosses no plane."""
    p = np.concatenate([through(FA, CROSS + [FA[0], FA[1], 0]), through(FB, CROSS + [FB[0], FB[1], 0]),
                        np.full((1, 2, 3), NAN), through(FB, [[-0.25, -1.75, 12.0]])])
    w = np.zeros((10, 2), dtype=np.float32)
    w[:4, 0], w[4:8, 0], w[9, 0] = 0.5, 0.25, 0.125
    wl = np.array([486.0] * 4 + [656.0] * 4 + [500.0, 656.0], dtype=np.float32)
    return p, w, wl


def test_oracle_recovers_two_chosen_foci_and_their_differences():
    p, w, wl = two_bands()
    out = cc.evaluate(p, w, wl, 0, 10, 0, "lines", reference=486.0)
    assert out["n_bands"] == 2 and out["reference_band"] == 0 and out["band_edges"] is None
    assert out["key"].tolist() == [0] * 4 + [1] * 4 + [cc.NO_BAND, 1]
    assert np.allclose(F64(out["focus"]), [FA, FB], rtol=0, atol=1e-15)
    assert out["z"] == 10.0
    assert np.allclose(F64(out["focal_shift"]), [0, 2], rtol=0, atol=1e-15) and abs(float(out["axial_colour"]) - 2) < 1e-15
    # the bundles are symmetric about chief rays along z: the centroid of a band is its focus' xy on every plane
    assert np.allclose(F64(out["centroid"]), [FA[:2], FB[:2]], rtol=0, atol=1e-15)
    assert np.allclose(F64(out["lateral_shift"]), [[0, 0], (FB - FA)[:2]], rtol=0, atol=1e-15)
    assert abs(float(out["lateral_colour"]) - np.hypot(0.25, 0.5)) < 1e-15
    # band 0 meets in a point there, band 1 is 2 mm before its focus: its rays are 1 / 6 of their start distance away
    assert F64(out["rms_radius"])[0] < 1e-15 and F64(out["rms_radius"])[1] == pytest.approx(1 / 6, rel=1e-15)
    assert F64(out["max_radius"])[1] == pytest.approx(1 / 6, rel=1e-15)
    assert F64(out["band_N"]).tolist() == [4, 4] and F64(out["band_power"]).tolist() == [2.0, 1.0]
    assert out["n_parallel"] == 1 and out["N"] == 8 and F64(out["wavelengths"]).tolist() == [486.0, 656.0]
    # the other reference, by default: the power-weighted mean of all used rays, (2 * 486 + 1.125 * 656) / 3.125 = 547.2: nearer to 486
    assert cc.evaluate(p, w, wl, 0, 10, 0, "lines")["reference_band"] == 0
    back = cc.evaluate(p, w, wl, 0, 10, 0, "lines", reference=700.0)
    assert back["reference_band"] == 1 and back["z"] == 12.0 and np.allclose(F64(back["focal_shift"]), [-2, 0], rtol=0, atol=1e-15)
    # a tie goes to the lower index
    assert cc.evaluate(p, w, wl, 0, 10, 0, "lines", reference=571.0)["reference_band"] == 0


def test_oracle_records_of_the_two_bands():
    p, w, wl = two_bands()
    key = [0] * 4 + [1] * 4 + [cc.NO_BAND, 1]
    val, mag = cc.records(p, w, wl, 0, 10, 0, key, 2, 10.0)
    v = F64(val)
    assert v[0].tolist() == [2, 4, 1, -0.5, 972, 0, 0, 0, 0, 0]
    assert v[1, :5].tolist() == [1, 4, 0.75, 0.25, 656] and v[1, 9] == 1
    assert v[1, 5] == pytest.approx(0.25 * 2 / 36, rel=1e-15) and v[1, 6] == pytest.approx(0.25 * 2 / 36, rel=1e-15) and abs(v[1, 7]) < 1e-17
    assert np.all(np.isfinite(v)) and np.all(np.isfinite(F64(mag))), "the dead ray's NaN position reached a sum"
    # a ray range: rays 4 .. 9 alone
    val, _ = cc.records(p, w, wl, 4, 6, 0, key[4:], 2, 10.0)
    assert F64(val)[0, :5].tolist() == [0] * 5 and F64(val)[1, 1] == 4 and np.all(np.isnan(F64(val)[0, 5:8]))
    # a centroid handed in is taken as it is
    val, _ = cc.records(p, w, wl, 0, 10, 0, key, 2, 10.0, centroid=[[0.5, 0.75], [0, 0]])
    assert F64(val)[0, 5:9].tolist() == [0, 2, 0, 1]


def test_oracle_focus_sums_add_up_to_the_bundle():
    p, w, wl = two_bands()
    key = np.array([0] * 4 + [1] * 4 + [cc.NO_BAND, 1])
    val, mag = cc.focus_sums(p, w, 0, 10, 0, key, 2, (0.25, 0, 1))
    one, _ = cc.focus_sums(p, w, 0, 10, 0, np.zeros(10, dtype=int), 1, (0.25, 0, 1))
    assert F64(val)[:, 1].tolist() == [4, 5] and F64(one)[0, 1] == 9
    assert np.allclose(F64(val.sum(axis=0)), F64(one[0]), rtol=1e-17, atol=1e-17)
    assert np.all(mag >= np.abs(val))
    assert np.allclose(F64(cc.foci(val[:1], (0.25, 0, 1))), [FA], rtol=0, atol=1e-15)


def test_oracle_empty_band_single_ray_and_collimated_band():
    """Edges 400 | 500 | 600 | 700 | 800: band 0 holds three collimated rays, band 1 nothing, band 2 one ray, band 3 the bundle
    through FB; 800 nm lies on the last edge and so in band 3, 399 nm in no band."""
    par = np.array([[[0.0, 0, 0], [0.0, 0, 1]], [[1.0, 0, 0], [1.0, 0, 1]], [[0.0, 2.0, 0], [0.0, 2.0, 1]]])
    p = np.concatenate([par, through(FA, [[1.0, 1.0, 0]]), through(FB, CROSS + [FB[0], FB[1], 0]), through(FA, [[2.0, 2.0, 0]])])
    w = np.ones((9, 2), dtype=np.float32)
    wl = np.array([400, 450, 499.9, 600, 700, 750, 800, 800, 399], dtype=np.float32)
    edges = np.array([400.0, 500, 600, 700, 800])
    out = cc.evaluate(p, w, wl, 0, 9, 0, edges, z=5.0)
    assert out["n_bands"] == 4 and out["key"].tolist() == [0, 0, 0, 2, 3, 3, 3, 3, cc.NO_BAND]
    f = F64(out["focus"])
    assert np.all(np.isnan(f[:3])) and np.allclose(f[3], FB, rtol=0, atol=1e-15), "collimated, empty and single-ray bands have no focus"
    assert F64(out["band_N"]).tolist() == [3, 0, 1, 4] and F64(out["band_power"]).tolist() == [3, 0, 1, 4]
    assert F64(out["rms_radius"])[2] == 0 and F64(out["rms_x"])[2] == 0 and F64(out["max_radius"])[2] == 0
    for name in ("wavelengths", "rms_x", "rms_y", "rms_radius", "cov_xy", "max_radius"):
        assert np.isnan(F64(out[name])[1]), name
    assert np.all(np.isnan(F64(out["centroid"])[1])) and float(out["axial_colour"]) == 0
    assert np.allclose(F64(out["centroid"])[0], [1 / 3, 2 / 3], rtol=1e-15)
    # the default plane is the reference band's focus z: a band without one cannot give it
    assert cc.evaluate(p, w, wl, 0, 9, 0, edges, reference=750.0)["z"] == pytest.approx(12.0, abs=1e-15)
    assert np.isnan(cc.evaluate(p, w, wl, 0, 9, 0, edges, reference=450.0)["z"])
    # an int: equal bands over 400 .. 800 of the used rays (the 399 nm ray takes part in the range: it is used)
    key, K, e = cc.band_keys(wl, np.ones(9, dtype=bool), 2)
    assert K == 2 and e.tolist() == [399, 599.5, 800] and key.tolist() == [0, 0, 0, 1, 1, 1, 1, 1, 0]
    key, K, e = cc.band_keys(np.full(5, 550, dtype=np.float32), np.ones(5, dtype=bool), 7)
    assert K == 1 and e.tolist() == [550, 550] and key.tolist() == [0] * 5


# ---- Raytracer.chromatic_analysis: arguments -----------------------------------------------------------------------------------------
def tracer():
    RT = ot.Raytracer(outline=[-1, 1, -1, 1, -1, 10])
    RT.add(ot.RaySource(ot.Point(), pos=[0, 0, 0]))
    return RT


@pytest.mark.parametrize("kwargs,error", [
    (dict(source_index=1.0), TypeError), (dict(source_index="0"), TypeError), (dict(source_index=True), TypeError),
    (dict(section=1.0), TypeError), (dict(section=-1), ValueError), (dict(section=1), ValueError),
    (dict(bands="bands"), ValueError), (dict(bands=2.0), TypeError), (dict(bands=True), TypeError), (dict(bands=None), TypeError),
    (dict(bands=0), ValueError), (dict(bands=33), ValueError), (dict(bands=[500.0]), ValueError),
    (dict(bands=list(range(400, 434))), ValueError), (dict(bands=[500, 400]), ValueError), (dict(bands=[400, 400]), ValueError),
    (dict(bands=[400, NAN]), ValueError), (dict(bands=[[400, 500]]), ValueError), (dict(bands=[400, "500"]), TypeError),
    (dict(z="1"), TypeError), (dict(z=NAN), ValueError), (dict(z=np.inf), ValueError), (dict(z=[1.0]), TypeError),
    (dict(reference="d"), TypeError), (dict(reference=NAN), ValueError), (dict(reference=-np.inf), ValueError),
])
def test_argument_errors_come_before_the_device(kwargs, error, monkeypatch):
    from optrace_amd import raytracer
    monkeypatch.setattr(raytracer, "require_device", lambda: pytest.fail("the device was asked for before the arguments were checked"))
    with pytest.raises(error):
        tracer().chromatic_analysis(**kwargs)


def test_band_limits_are_named_in_the_message():
    with pytest.raises(ValueError, match="32"):
        chrom.check_arguments(2, None, 33, None, None)
    with pytest.raises(ValueError, match="33"):
        chrom.check_arguments(2, None, np.arange(400.0, 435.0), None, None)
    bands, z, ref = chrom.check_arguments(2, 0, [400, 500, 600], 3, np.float32(550))
    assert bands.dtype == np.float64 and bands.tolist() == [400, 500, 600] and (z, ref) == (3.0, 550.0) and isinstance(z, float)
    assert chrom.check_arguments(2, None, "lines", None, None) == ("lines", None, None)
    assert chrom.check_arguments(5, 3, 32, None, None)[0] == 32


def test_good_arguments_reach_the_device_and_then_the_rays(monkeypatch):
    from optrace_amd import raytracer
    asked = []
    monkeypatch.setattr(raytracer, "require_device", lambda: asked.append(1))
    for kwargs in (dict(), dict(source_index=None, section=0, bands=4, z=1.0, reference=550), dict(bands=[400, 500.5, 700])):
        with pytest.raises(RuntimeError, match="No rays traced"):
            tracer().chromatic_analysis(**kwargs)
    assert len(asked) == 3


# ---- ot.ChromaticAnalysis ------------------------------------------------------------------------------------------------------------
def from_oracle(p, w, wl, count, bands, z, reference):
    """`ot.ChromaticAnalysis` from the oracle's records and foci rounded to float64, and the oracle's own figures."""
    out = cc.evaluate(p, w, wl, 0, count, 0, bands, z=z, reference=reference)
    val, _ = cc.records(p, w, wl, 0, count, 0, out["key"], out["n_bands"], out["z"])
    a = ot.ChromaticAnalysis(F64(val), F64(out["focus"]), float(out["z"]), out["reference_band"], 0, out["band_edges"], long_desc="by hand")
    return a, out, F64(val)


def test_derived_fields_against_a_direct_evaluation():
    rng = np.random.default_rng(5)
    n = 300
    starts = np.concatenate([rng.normal(size=(n, 2)) * [2.0, 1.0] + [0.3, -0.2], np.zeros((n, 1))], axis=1)
    wl = rng.choice(np.array([450, 550, 650, 700], dtype=np.float32), size=n, p=[0.4, 0.3, 0.299, 0.001])
    wl[:4] = [450, 550, 650, 700]
    target = np.array([0.1, 0.2, 20.0]) + ((wl[:, None] - 550) / 100) * [0.05, -0.02, 0.4] + rng.normal(size=(n, 3)) * 1e-3
    p = np.stack([starts, starts + 1.5 * (target - starts)], axis=1)
    w = rng.uniform(0.1, 1, size=(n, 2)).astype(np.float32)
    w[rng.uniform(size=n) < 0.1, 0] = 0
    p[w[:, 0] == 0] = NAN
    p[7, 1, 2] = p[7, 0, 2]  # (one ray in the plane z = 0)
    w[:8, 0] = 0.5
    wl[4:8] = [450, 550, 650, 650]
    p[:8] = np.where(np.isnan(p[:8]), 1.0, p[:8])
    p[7, 1, 2] = p[7, 0, 2]
    edges = np.array([400.0, 500, 600, 680, 690, 701])
    for bands, z, reference in (("lines", None, None), (edges, 19.5, 560.0), (3, None, 640.0)):
        a, out, rec = from_oracle(p, w, wl, n, bands, z, reference)
        K = out["n_bands"]
        assert a.n_bands == K == len(a.wavelengths) and a.reference_band == out["reference_band"] and a.z == out["z"]
        assert a.section == 0 and a.long_desc == "by hand" and a.records.shape == (K, 10)
        assert (a.band_edges is None) == (bands == "lines" if isinstance(bands, str) else False)
        assert a.N == int(out["N"]) and a.n_parallel == 1 == int(out["n_parallel"]) and a.band_N.dtype == np.int64
        assert np.array_equal(a.band_N, F64(out["band_N"])) and np.array_equal(a.band_power, rec[:, 0])
        close = lambda got, want, tol=1e-13: np.allclose(got, F64(want), rtol=tol, atol=1e-15, equal_nan=True)
        assert close(a.power, out["power"]) and close(a.wavelengths, out["wavelengths"]) and close(a.centroid, out["centroid"])
        many = a.band_N > 1
        for name in ("rms_x", "rms_y", "rms_radius", "cov_xy"):
            assert close(getattr(a, name)[many], out[name][many], 1e-12), name
            assert np.all(getattr(a, name)[a.band_N == 1] == 0) and np.all(np.isnan(getattr(a, name)[a.band_N == 0])), name
        assert close(a.max_radius, out["max_radius"]) and close(a.focus, out["focus"])
        assert close(a.focal_shift, out["focal_shift"]) and close(a.axial_colour, out["axial_colour"])
        assert close(a.lateral_shift, out["lateral_shift"], 1e-11) and close(a.lateral_colour, out["lateral_colour"], 1e-11)
        # the polychromatic spot from the band records against the sum over all rays
        assert close(a.centroid_all, out["centroid_all"]) and close(a.rms_radius_all, out["rms_radius_all"], 1e-12)
        assert a.rms_radius_all >= np.nanmin(a.rms_radius)
    a, out, _ = from_oracle(p, w, wl, n, edges, 19.5, 560.0)
    assert a.band_N[3] == 0 and a.band_N[4] >= 1 and np.array_equal(a.band_edges, edges)  # (an empty band and a thin one)


def test_result_object_is_locked_and_checks_its_shapes():
    rec = np.zeros((2, 10))
    rec[0] = [2, 4, 1, -0.5, 972, 0.5, 0.5, 0.1, 0.25, 0]
    rec[1, 5:8] = NAN
    a = ot.ChromaticAnalysis(rec, [[0, 0, 1], [NAN] * 3], 1.0, 0, 3, [400, 500, 600])
    assert a.N == 4 and a.power == 2 and a.band_N.tolist() == [4, 0] and a.centroid[0].tolist() == [0.5, -0.25]
    assert a.rms_x[0] == 0.5 and a.rms_radius[0] == np.sqrt(0.5) and a.cov_xy[0] == 0.05 and a.max_radius[0] == 0.5
    assert np.isnan(a.wavelengths[1]) and np.isnan(a.max_radius[1]) and np.isnan(a.focal_shift[1]) and a.focal_shift[0] == 0
    assert a.axial_colour == 0 and a.lateral_colour == 0 and a.centroid_all.tolist() == [0.5, -0.25] and a.rms_radius_all == np.sqrt(0.5)
    with pytest.raises(RuntimeError):
        a.power = 1.0
    with pytest.raises(ValueError):
        a.focus[0] = 1
    with pytest.raises(AttributeError):
        a.something_else = 1
    for bad in (dict(focus=[[0, 0, 1]]), dict(band_edges=[400, 500]), dict(reference_band=2), dict(reference_band=-2)):
        args = dict(records=rec, focus=[[0, 0, 1], [NAN] * 3], z=1.0, reference_band=0, section=3, band_edges=[400, 500, 600])
        with pytest.raises(ValueError):
            ot.ChromaticAnalysis(**{**args, **bad})
    with pytest.raises(ValueError):
        ot.ChromaticAnalysis(np.zeros((33, 10)), np.zeros((33, 3)), 0.0, 0, 0)
    # the empty result: what the caller fixed stays, every figure NaN
    e = chrom._empty(3, np.array([400.0, 500, 600]), None)
    assert e.N == 0 and e.power == 0 and e.n_bands == 2 and e.reference_band == -1 and np.isnan(e.z) and e.band_N.tolist() == [0, 0]
    for f in (e.focus, e.centroid, e.wavelengths, e.rms_radius, e.focal_shift, e.lateral_shift, e.centroid_all, e.max_radius):
        assert np.all(np.isnan(f))
    assert np.isnan(e.axial_colour) and np.isnan(e.lateral_colour) and np.isnan(e.rms_radius_all)
    e = chrom._empty(0, "lines", 2.5)
    assert e.n_bands == 1 and e.z == 2.5 and e.band_edges is None


def test_reference_band_and_band_foci():
    assert chrom.reference_band([486, 587, 656], [5, 5, 5], 600.0) == 1
    assert chrom.reference_band([486, 587, 656], [5, 0, 5], 600.0) == 2
    assert chrom.reference_band([500, 600], [1, 1], 550.0) == 0, "a tie goes to the lower index"
    assert chrom.reference_band([NAN, 600], [0, 1], 100.0) == 1 and chrom.reference_band([NAN, NAN], [0, 0], 500.0) == -1
    p, w, wl = two_bands()
    key = np.array([0] * 4 + [1] * 4 + [cc.NO_BAND, 2])
    val, _ = cc.focus_sums(p, w, 0, 10, 0, key, 4, (0, 0, 1))
    f = chrom.band_foci(F64(val), np.array([0.0, 0, 1]))
    assert np.allclose(f[:2], [FA, FB], rtol=0, atol=1e-14) and np.all(np.isnan(f[2:])), "a single ray and no ray have no focus"
    # the wavefront analysis' test, shared: a collimated bundle
    from optrace_amd import wavefront
    s = np.zeros(17)
    s[[0, 1, 8, 11]] = [3, 3, 3, 3]
    assert np.all(np.isnan(wavefront.closest_point(s, np.zeros(3))))
    with pytest.raises(RuntimeError, match="collimated"):
        wavefront.reference_sphere(s, np.zeros(3), None, None)


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_before_anything_else():
    lib = _capi.load_library()
    st = C.c_void_p()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)  # (never dereferenced: every call below returns from its checks)
    d3 = lambda *v: (C.c_double * 3)(*v)
    INVALID, UNSUPPORTED = -1, -3

    def rays(N=100, nt=3, p=a, w=a, wl=a):
        r = _capi.Rays()
        r.N, r.nt, r.p, r.w, r.wl = N, nt, p, w, wl
        return C.byref(r)

    def refused(code, text, status):
        assert status == code and text.encode() in lib.ot_last_error(), (status, lib.ot_last_error())

    focus = lambda *args: lib.ot_chromatic_focus(*args, st)
    ok = [rays(), 0, 10, 1, a, 3, d3(0, 0, 0), a, a]
    for i in (0, 4, 6, 7, 8):
        refused(INVALID, "ot_chromatic_focus: null argument", focus(*[None if j == i else x for j, x in enumerate(ok)]))
    for R in (rays(p=None), rays(w=None)):
        refused(INVALID, "ot_chromatic_focus: null argument", focus(R, *ok[1:]))
    for first, count in ((-1, 5), (0, -1), (0, 101), (91, 10), (101, 0)):
        refused(INVALID, "ot_chromatic_focus: ray range", focus(ok[0], first, count, *ok[3:]))
    for k in (-1, 2, 100):
        refused(INVALID, "ot_chromatic_focus: section", focus(*ok[:3], k, *ok[4:]))
    for org in (d3(NAN, 0, 0), d3(0, np.inf, 0), d3(0, 0, -np.inf)):
        refused(INVALID, "ot_chromatic_focus: origin", focus(*ok[:6], org, *ok[7:]))
    for K in (0, -1, 33):
        refused(UNSUPPORTED, "ot_chromatic_focus: n_bands outside 1 .. 32", focus(*ok[:5], K, *ok[6:]))
    assert focus(ok[0], 0, 0, *ok[3:]) == 0 and focus(ok[0], 100, 0, *ok[3:]) == 0
    refused(UNSUPPORTED, "ot_chromatic_focus", focus(ok[0], 0, 0, 1, a, 33, *ok[6:]))  # (the limits hold whatever the count is)

    plane = lambda *args: lib.ot_chromatic_plane(*args, st)
    ok = [rays(), 0, 10, 1, a, 3, 2.5, a, a]
    for i in (0, 4, 7, 8):
        refused(INVALID, "ot_chromatic_plane: null argument", plane(*[None if j == i else x for j, x in enumerate(ok)]))
    for R in (rays(p=None), rays(w=None), rays(wl=None)):
        refused(INVALID, "ot_chromatic_plane: null argument", plane(R, *ok[1:]))
    refused(INVALID, "ot_chromatic_plane: ray range", plane(ok[0], 95, 10, *ok[3:]))
    refused(INVALID, "ot_chromatic_plane: section", plane(*ok[:3], 2, *ok[4:]))
    for z in (NAN, np.inf, -np.inf):
        refused(INVALID, "ot_chromatic_plane: z not finite", plane(*ok[:6], z, *ok[7:]))
    for K in (0, -5, 33):
        refused(UNSUPPORTED, "ot_chromatic_plane: n_bands outside 1 .. 32", plane(*ok[:5], K, *ok[6:]))
    assert plane(ok[0], 0, 0, *ok[3:]) == 0 and plane(ok[0], 100, 0, 0, a, 32, 0.0, a, a) == 0


def test_workspace():
    """Doubles for the partial sums: 17 per workgroup of 256 rays and band, at most 1024 workgroups per band and piece of 2^28 rays;
    0 for arguments out of range."""
    ws = _capi.load_library().ot_chromatic_workspace
    assert ws(1, 1) == 17 and ws(256, 3) == 17 * 3 and ws(257, 3) == 17 * 3 * 2
    assert ws(256 * 1024, 5) == ws(10 ** 8, 5) == 17 * 5 * 1024 and ws(2 ** 28 + 1, 32) == 17 * 32 * 1025
    assert ws(0, 3) == 0
    for count, K in ((-1, 3), (10, 0), (10, -1), (10, 33)):
        assert ws(count, K) == 0


def test_constants_match_the_header():
    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "optrace_amd.h").read_text()
    value = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert value("OT_CHROM_M") == _capi.CHROM_M == cc.M == 10
    assert value("OT_CHROM_MAX_BANDS") == _capi.CHROM_MAX_BANDS == cc.MAX_BANDS == _capi.PSF_MAX_BANDS == 32
    assert value("OT_CHROM_BLOCKS") == _capi.CHROM_BLOCKS == 1024
    assert value("OT_WF_FOCUS_M") == _capi.WF_FOCUS_M == cc.FOCUS_M == 17
    assert _capi.CHROM_NO_BAND == cc.NO_BAND == 255
    assert value("OT_ABI_VERSION") == _capi.ABI_VERSION == 9
    for name in ("ot_chromatic_workspace", "ot_chromatic_focus", "ot_chromatic_plane"):
        assert name in _capi.SIGNATURES and re.search(rf"\b{name}\(", text)
    assert ot.ChromaticAnalysis is chrom.ChromaticAnalysis and callable(ot.Raytracer.chromatic_analysis)


# ---- one physical pin -------------------------------------------------------------------------------------------------------------------
HALF_ANGLE = 0.1  # degrees
DEVIATION = 2.99e-4  # mm: measured, the largest |focus z - paraxial image z| of the three lines
SPAN = 0.3335  # mm: z_C - z_F


def test_focus_per_line_follows_the_paraxial_image_position():
    """The single lens of the `c1_single_lens` scene, in a glass with dispersion (n_d = 1.5168, V = 64.17: the scene's own medium is
    a constant 1.5 and has no colour), traced by the C oracle: a point on the axis at z = -20 mm sends a cone of 0.1 degrees half
    angle, 96 rays on 8 rings per line F, d, C.  The definition's focus z per line against `RT.tma(wl).image_position(-20)`:
    z_F < z_d < z_C, and the largest deviation measured is 2.99e-4 mm (each line lies that much before its paraxial image: the
    bundle's residual spherical aberration, which falls to a quarter at half the angle), 0.09 % of z_C - z_F = 0.3335 mm.  Rays and
    definition are deterministic; the test allows twice the measured value for a longdouble that is narrower on another host."""
    from optrace_amd.scene import CompiledScene
    import oracle_bridge as ob
    import scenes
    with ot.global_options.no_warnings():
        RT = scenes.c1_single_lens(ot)
        RT.lenses[0].n = ot.RefractionIndex("Abbe", n=1.5168, V=64.17)
    RT._geometry_checks()
    assert not RT.geometry_error
    sc = CompiledScene(RT)
    lines = ot.presets.spectral_lines.FdC
    rings, spokes = 8, 12
    theta = np.deg2rad(HALF_ANGLE) * np.sqrt((np.arange(rings) + 0.5) / rings)
    phi = 2 * np.pi * (np.arange(spokes) + 0.5) / spokes
    T, P = np.meshgrid(theta, phi, indexing="ij")
    s = np.stack([np.sin(T) * np.cos(P), np.sin(T) * np.sin(P), np.cos(T)], axis=-1).reshape(-1, 3)
    s0 = np.tile(s, (3, 1))
    N = s0.shape[0]
    wl = np.repeat(np.array(lines, dtype=np.float32), s.shape[0])
    pol0 = np.cross(s0, [0.0, 1.0, 0.0])
    pol0 /= np.linalg.norm(pol0, axis=1)[:, None]
    rays = ob.HostRays(N, sc.nt, False)
    rays.set_initial(np.tile([0.0, 0.0, -20.0], (N, 1)), s0, pol0, np.full(N, 1.0 / N, dtype=np.float32), wl)
    _, status = ob.trace(sc.desc, rays, None)
    assert status == 0
    p, w, k = np.array(rays.p_list), np.array(rays.w_list), sc.nt - 2
    assert np.all(w[:, k] > 0)
    out = cc.evaluate(p, w, wl, 0, N, k, "lines")
    z = F64(out["focus"])[:, 2]
    paraxial = np.array([RT.tma(float(lam)).image_position(-20.0) for lam in lines])
    deviation = np.abs(z - paraxial)
    print(f"focus z {z}, paraxial {paraxial}, deviation {deviation}, z_C - z_F {z[2] - z[0]:.6f}")
    assert out["n_bands"] == 3 and out["reference_band"] == 1 and F64(out["wavelengths"]).tolist() == [float(np.float32(v)) for v in lines]
    assert z[0] < z[1] < z[2]
    assert z[2] - z[0] == pytest.approx(SPAN, abs=1e-4) and paraxial[2] - paraxial[0] == pytest.approx(SPAN, abs=1e-4)
    assert deviation.max() <= 2 * DEVIATION, f"deviation {deviation.max():.3e} mm"
    assert 0.5 * DEVIATION < deviation.max(), "the measured value stands in the docstring and in DESIGN.md"
    assert np.all(z < paraxial)
    # on the axis there is no lateral colour, and the focal shifts are the foci's differences
    assert float(out["lateral_colour"]) < 1e-12 and float(out["axial_colour"]) == pytest.approx(z[2] - z[0], rel=1e-12)
    assert np.allclose(F64(out["focal_shift"]), z - z[1], rtol=0, atol=1e-15)
