"""Raytracer.mtf_analysis without a device: the argument checks, the refusals of the `ot_mtf_*` entry points, the host arithmetic of
`ot.MTFAnalysis` on hand-made sums against direct longdouble sums over all rays, and closed-form pins of the oracle
(tests/mtf_cases.py)."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd import mtf

import field_cases as fc
import mtf_cases as mc

EPS, LD, NAN = mc.EPS, mc.LD, float("nan")
F64 = lambda a: np.asarray(a).astype(np.float64)
CPX = lambda re, im: F64(re) + 1j * F64(im)


# ---- hand-made storages ------------------------------------------------------------------------------------------------------------------
def storage(points, slopes, weights, z0=1.0, length=2.0):
    """Rays that cross the plane z0 at `points` (n, 2) with the slopes (n, 2), stored as one section from z0 - 1 on: p (n, 2, 3),
    w (n, 2), wl (n,)."""
    points, slopes = np.asarray(points, dtype=np.float64), np.asarray(slopes, dtype=np.float64)
    n = points.shape[0]
    p = np.zeros((n, 2, 3))
    p[:, 0, :2], p[:, 0, 2] = points - slopes, z0 - 1.0
    p[:, 1, :2], p[:, 1, 2] = points + (length - 1.0) * slopes, z0 - 1.0 + length
    return p, np.tile(np.asarray(weights, dtype=np.float32)[:, None], (1, 2)), np.full(n, 550.0, dtype=np.float32)


def oracle_analysis(p, w, wl, fields, key, K, origin, field, z, dz, freq, reference_band=0):
    """The records and the sums of the oracle, rounded to f64, through `ot.MTFAnalysis`.  -> (analysis, val, allow, records)"""
    rec, _ = fc.records(p, w, wl, fields, 0, key, 0, K, origin)
    rec = F64(rec)
    planes = z + np.asarray(dz, dtype=np.float64)
    t = fc.directions(field)
    val, allow, _ = mc.sums(p, w, fields, 0, key, 0, K, origin, fc.record_means(rec), t, planes - origin[2], freq)
    a = ot.MTFAnalysis(F64(val), rec, origin, z, planes, freq, reference_band, 0, 0, list(range(len(fields))), field)
    return a, val, allow, rec


def crossing(p, z):
    d = p[:, 1] - p[:, 0]
    return p[:, 0, :2] + ((z - p[:, 0, 2]) / d[:, 2])[:, None] * d[:, :2]


# ---- ot.MTFAnalysis: host arithmetic --------------------------------------------------------------------------------------------------
def test_bands_add_to_the_polychromatic_mtf_about_their_common_centroid():
    """Two fields, two bands whose centroids lie apart, three planes: the per-band OTF and the `*_all` figures against direct sums over
    the rays where they cross the plane.  Tolerance: the sums of the oracle are rounded to f64 once (eps), the host divides and
    turns each band by a phase of at most 2 pi nu |c_b - c_all| <= 2 pi 30 * 1 whose rounding is eps of that: 1e-12 covers both."""
    rng = np.random.default_rng(4)
    n = 60
    points = rng.normal(size=(2 * n, 2)) * 0.02
    slopes = rng.normal(size=(2 * n, 2)) * 0.05
    key = np.tile(np.arange(n) % 2, 2).astype(np.uint8)
    points[key == 1] += [0.3, -0.2]  # (lateral colour: band 1 lands elsewhere)
    weights = rng.uniform(0.2, 1.0, size=2 * n)
    p, w, wl = storage(points, slopes, weights)
    wl[key == 1] = 650.0
    fields, origin, field = [(0, n), (n, n)], np.array([0.01, -0.02, 0.5]), np.array([[0.0, 0.0], [3.0, 4.0]])
    freq, dz = np.array([0.0, 5.0, 30.0]), np.array([-0.1, 0.0, 0.2])
    a, _, _, _ = oracle_analysis(p, w, wl, fields, key, 2, origin, field, 1.0, dz, freq)
    assert a.otf_t.shape == a.mtf_s.shape == (2, 2, 3, 3) and a.otf_t_all.shape == a.mtf_s_all.shape == (2, 3, 3)
    assert a.centroid.shape == (2, 2, 3, 2) and a.sums.shape == (2, 2, 3, 3, 4) and a.focus_mtf_t.shape == (2, 2, 3)
    assert np.allclose(a.t, [[0, 1], [0.6, 0.8]]) and np.allclose(a.wavelengths, [550, 650]) and np.array_equal(a.planes, 1.0 + dz)
    worst = 0.0
    for f, (first, count) in enumerate(fields):
        t = a.t[f]
        for u, otf, otf_all in ((t, a.otf_t, a.otf_t_all), (np.array([-t[1], t[0]]), a.otf_s, a.otf_s_all)):
            for j, z in enumerate(a.planes):
                x = crossing(p[first:first + count], z)
                wt = w[first:first + count, 0]
                for b in range(2):
                    m = key[first:first + count] == b
                    re, im, c = mc.direct_otf(x[m], wt[m], u, freq)
                    worst = max(worst, np.max(np.abs(otf[f, b, j] - CPX(re, im))), np.max(np.abs(a.centroid[f, b, j] - F64(c))))
                re, im, _ = mc.direct_otf(x, wt, u, freq)
                worst = max(worst, np.max(np.abs(otf_all[f, j] - CPX(re, im))))
    print(f"per band and polychromatic OTF: off by at most {worst:.3e}")
    assert worst <= 1e-12
    assert np.array_equal(a.mtf_t_all, np.abs(a.otf_t_all)) and np.array_equal(a.mtf_s, np.abs(a.otf_s))
    # the bands apart blur the sum: below both bands' own MTF at the highest frequency, where their phases differ
    assert np.all(a.mtf_t_all[:, :, 0] == pytest.approx(1.0, abs=1e-15))


def test_a_cell_of_one_ray_and_a_cell_without_a_ray():
    """Field 0: band 0 holds one ray, band 1 none; field 1 holds no ray at all."""
    p, w, wl = storage([[0.1, 0.2], [0.0, 0.0]], [[0.01, 0.0], [0.0, 0.0]], [0.7, 0.0])
    key = np.zeros(2, dtype=np.uint8)
    origin = np.zeros(3)
    a, val, _, rec = oracle_analysis(p, w, wl, [(0, 1), (1, 1)], key, 2, origin, np.array([[0.0, 1.0], [0.0, 2.0]]), 1.0, [0.0, 0.5],
                                     np.array([0.0, 10.0, 40.0]))
    assert a.band_N.tolist() == [[1, 0], [0, 0]] and a.band_power[0, 0] == np.float32(0.7) and a.band_power[1].tolist() == [0, 0]
    assert np.all(a.otf_t[0, 0] == 1) and np.all(a.otf_s[0, 0] == 1) and np.all(a.mtf_t[0, 0] == 1) and np.all(a.mtf_s[0, 0] == 1)
    assert np.allclose(a.centroid[0, 0], [[0.1, 0.2], [0.105, 0.2]], rtol=0, atol=1e-15)
    assert np.all(a.otf_t_all[0] == 1) and np.all(a.mtf_s_all[0] == 1)  # (one band with rays: the field's figures are that band's)
    for cell in ((0, 1), (1, 0), (1, 1)):
        for name in ("otf_t", "otf_s", "mtf_t", "mtf_s", "centroid", "focus_mtf_t", "focus_mtf_s"):
            assert np.all(np.isnan(getattr(a, name)[cell])), (cell, name)
    assert np.all(np.isnan(a.otf_t_all[1])) and np.all(np.isnan(a.mtf_s_all[1])) and np.isnan(a.wavelengths[1])
    # a sum that is not exactly w for the single ray: the host still says 1
    s = F64(val)
    s[0, 0] *= 1 + 4 * EPS
    b = ot.MTFAnalysis(s, rec, origin, 1.0, [1.0, 1.5], [0.0, 10.0, 40.0], 0, 0, 0, [0, 1], [[0, 1], [0, 2]])
    assert np.all(b.otf_t[0, 0] == 1) and np.all(b.mtf_s[0, 0] == 1)


def test_through_focus_peak():
    """A known parabola over uneven planes: where its vertex lies (values of order 1 carry eps, the curvature times the spacing is
    above 0.1: 1e-13 allowed); a largest value on the first or last plane, or fewer than three planes: NaN."""
    planes = np.array([-0.3, -0.1, 0.05, 0.2, 0.5])
    curve = lambda z, top, at, c: top - c * (z - at) ** 2
    y = np.stack([curve(planes, 0.8, 0.0, 2.0), curve(planes, 0.6, -0.12, 1.0), curve(planes, 0.9, 0.7, 1.0), curve(planes, 0.9, -0.5, 1.0),
                  np.full(5, 0.25)])
    got = mtf.parabola_peak(planes, y)
    assert got[:2] == pytest.approx([0.0, -0.12], abs=1e-13) and np.isnan(got[2]) and np.isnan(got[3])
    assert np.isnan(got[4])  # (all equal: the first plane holds the largest value)
    assert np.all(np.isnan(mtf.parabola_peak(planes[:2], y[:, :2]))) and mtf.parabola_peak(planes[:3], y[:, :3]).shape == (5,)
    y[0, 3] = NAN
    assert np.isnan(mtf.parabola_peak(planes, y)[0])
    # through the result object: one field, one band, two frequencies with their peaks between different planes
    rec = np.zeros((1, 1, 18))
    rec[0, 0, :2] = [2.0, 5]
    sums = np.zeros((1, 1, 5, 2, 4))
    sums[0, 0, :, 0, 0], sums[0, 0, :, 1, 0] = 2 * curve(planes, 0.8, 0.0, 2.0), 2 * curve(planes, 0.6, -0.12, 1.0)
    sums[0, 0, :, 0, 3], sums[0, 0, :, 1, 3] = 2 * curve(planes, 0.9, 0.7, 1.0), -2 * curve(planes, 0.5, 0.1, 1.0)
    a = ot.MTFAnalysis(sums, rec, [0, 0, 0], 0.0, planes, [10.0, 20.0], 0, 0, 0, [0], [[0, 1]])
    assert a.focus_mtf_t[0, 0] == pytest.approx([0.0, -0.12], abs=1e-13)
    assert np.isnan(a.focus_mtf_s[0, 0, 0]) and a.focus_mtf_s[0, 0, 1] == pytest.approx(0.1, abs=1e-13)


def test_result_object_is_locked_and_checks_its_shapes():
    rec = np.zeros((2, 1, 18))
    rec[:, 0, :2] = [1.0, 3]
    good = dict(sums=np.zeros((2, 1, 2, 3, 4)), records=rec, origin=[0, 0, 0], z=0.0, planes=[0.0, 1.0], frequencies=[0.0, 1, 2],
                reference_band=0, reference_field=1, section=0, sources=[3, 1], field=[[0, 1], [1, 0]])
    a = ot.MTFAnalysis(**good)
    assert (a.n_fields, a.n_bands, a.n_planes, a.n_frequencies) == (2, 1, 2, 3) and a.sources.tolist() == [3, 1]
    with pytest.raises(RuntimeError, match="read-only"):
        a.z = 1.0
    for change, error in ((dict(sums=np.zeros((2, 1, 2, 3, 3))), ValueError), (dict(reference_band=1), ValueError),
                          (dict(reference_field=2), ValueError), (dict(band_edges=[400, 500, 600]), ValueError),
                          (dict(planes=np.zeros(66), sums=np.zeros((2, 1, 66, 3, 4))), ValueError),
                          (dict(frequencies=np.zeros(65), sums=np.zeros((2, 1, 2, 65, 4))), ValueError),
                          (dict(reference_band=0.0), TypeError)):
        with pytest.raises(error):
            ot.MTFAnalysis(**{**good, **change})


# ---- closed-form pins of the oracle ---------------------------------------------------------------------------------------------------
def comb(N, x):
    """|sin(x) / (N sin(x / N))|, 1 where x / N is a multiple of pi"""
    x = np.asarray(x, dtype=LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.abs(np.where(np.sin(x / N) == 0, 1, np.sin(x) / (N * np.sin(x / N)))).astype(np.float64)


@pytest.mark.parametrize("field", [(0.0, 1.0), (3.0, 4.0), (-1.0, 1.0)])
def test_rays_on_the_midpoints_of_equal_cells(field):
    """N parallel rays of equal weight crossing at the midpoints of N equal cells of a segment of half width h along t:
    mtf_t = |sin(2 pi nu h) / (N sin(2 pi nu h / N))|, mtf_s = 1, on every plane.  Tolerance: the positions are rounded to f64
    (eps |x|, a phase error of 2 pi nu eps |x|) on top of the oracle's allowance over the power."""
    N, h = 24, 0.05
    t = fc.directions([field])[0]
    along = h * (2 * np.arange(N) + 1 - N) / N
    p, w, wl = storage(np.array([0.4, -0.3]) + along[:, None] * t, np.zeros((N, 2)), np.full(N, 0.5))
    freq = np.array([0.0, 1.0, 7.5, 10.0, 33.0, 150.0])
    a, _, allow, _ = oracle_analysis(p, w, wl, [(0, N)], np.zeros(N, dtype=np.uint8), 1, np.array([0.0, 0.0, 0.0]), [field], 1.0,
                                     [-0.5, 0.0, 0.7], freq)
    want = comb(N, 2 * mc.PI * freq.astype(LD) * LD(h))
    tol = allow[0, 0] / (0.5 * N) + (2 * np.pi * freq * 8 * EPS)[None, :, None]
    off_t, off_s = np.abs(a.mtf_t[0, 0] - want[None, :]), np.abs(a.mtf_s[0, 0] - 1)
    print(f"field {field}: mtf_t off by {off_t.max():.3e}, mtf_s by {off_s.max():.3e}")
    assert np.all(off_t <= tol[:, :, 0]) and np.all(off_s <= tol[:, :, 1])
    assert a.mtf_t[0, 0, 0, 3] < 1e-12  # (nu h = 1 / 2: the first zero of the segment)


def test_a_cone_through_one_point():
    """Rays through one point of the plane z0 have MTF 1 there at every frequency; a plane dz further on they cross at the point
    plus dz times their slopes: slopes on the midpoints of equal cells along t give the MTF of the fan scaled by dz."""
    N, hm, dz = 16, 0.1, 0.25
    t = fc.directions([(3.0, 4.0)])[0]
    slope = hm * (2 * np.arange(N) + 1 - N) / N
    p, w, wl = storage(np.tile([0.25, 0.5], (N, 1)), slope[:, None] * t, np.full(N, 1.0), z0=2.0)
    freq = np.array([0.0, 3.0, 20.0, 100.0])
    a, _, allow, _ = oracle_analysis(p, w, wl, [(0, N)], np.zeros(N, dtype=np.uint8), 1, np.array([0.25, 0.5, 1.0]), [(3.0, 4.0)], 2.0,
                                     [0.0, dz], freq)
    tol = allow[0, 0] / N + (2 * np.pi * freq * 8 * EPS)[None, :, None]
    assert np.all(np.abs(a.mtf_t[0, 0, 0] - 1) <= tol[0, :, 0]) and np.all(np.abs(a.mtf_s[0, 0] - 1) <= tol[:, :, 1])
    want = comb(N, 2 * mc.PI * freq.astype(LD) * LD(hm) * LD(dz))
    print(f"cone: off the point's plane mtf_t {a.mtf_t[0, 0, 1]} against {want}")
    assert np.all(np.abs(a.mtf_t[0, 0, 1] - want) <= tol[1, :, 0]) and want[2] < 0.7


def test_small_phases_give_the_rms_size_of_the_field_analysis():
    """For 2 pi nu max|e| <= 0.01: (1 - mtf_t) / (2 pi^2 nu^2) is rms_t^2 of `FieldAnalysis` from the same storage up to the next
    order of the series, (2 pi nu max|e|)^2 / 12 relative; on top, 1 - mtf carries the rounding of the sums, 8 eps."""
    rng = np.random.default_rng(9)
    n = 200
    p, w, wl = storage(rng.uniform(-0.01, 0.01, size=(n, 2)), rng.uniform(-0.02, 0.02, size=(n, 2)), rng.uniform(0.5, 1.0, size=n))
    origin, field, z = np.array([0.0, 0.0, 0.5]), [(1.0, 2.0)], 1.1
    rec = F64(fc.records(p, w, wl, [(0, n)], 0, np.zeros(n, dtype=np.uint8), 0, 1, origin)[0])
    fa = ot.FieldAnalysis(rec, origin, z, 0, 0, 0, [0], field, [1.0])
    al_t, mu_t, al_s, mu_s = mc.line_terms(fc.lines(p, w, 0, n, 0, origin)[2], fc.record_means(rec)[0, 0], fa.t[0])
    zeta = z - origin[2]
    for (al, mu), rms, name in (((al_t, mu_t), fa.rms_t[0, 0], "mtf_t"), ((al_s, mu_s), fa.rms_s[0, 0], "mtf_s")):
        e_max = np.max(np.abs(al + zeta * mu))
        freq = np.array([0.25, 0.5, 1.0]) * 0.01 / (2 * np.pi * e_max)
        a = oracle_analysis(p, w, wl, [(0, n)], np.zeros(n, dtype=np.uint8), 1, origin, field, z, [0.0], freq)[0]
        got = (1 - getattr(a, name)[0, 0, 0]) / (2 * np.pi ** 2 * freq ** 2)
        rel = np.abs(got / rms ** 2 - 1)
        tol = (2 * np.pi * freq * e_max) ** 2 / 12 + 8 * EPS / (1 - getattr(a, name)[0, 0, 0])
        print(f"{name}: (1 - mtf) / (2 pi^2 nu^2) against rms^2: relative {rel}, allowed {tol}")
        assert np.all(rel <= tol)


# ---- Raytracer.mtf_analysis: arguments -------------------------------------------------------------------------------------------------
def tracer():
    RT = ot.Raytracer(outline=[-1, 1, -1, 1, -1, 10])
    RT.add(ot.RaySource(ot.Point(), pos=[0, 0, 0]))
    RT.add(ot.RaySource(ot.Point(), pos=[0, 0.5, 0]))
    return RT


@pytest.mark.parametrize("kwargs,error", [
    (dict(sources=1), TypeError), (dict(sources="01"), TypeError), (dict(sources=[]), ValueError), (dict(sources=[0.0]), TypeError),
    (dict(sources=[True]), TypeError), (dict(sources=[0, 2]), IndexError), (dict(sources=[-1]), IndexError), (dict(sources=[1, 1]), ValueError),
    (dict(sources=list(range(65))), ValueError),
    (dict(section=1.0), TypeError), (dict(section=-1), ValueError), (dict(section=1), ValueError),
    (dict(bands="bands"), ValueError), (dict(bands=2.0), TypeError), (dict(bands=None), TypeError), (dict(bands=0), ValueError),
    (dict(bands=33), ValueError), (dict(bands=[500.0]), ValueError), (dict(bands=[500, 400]), ValueError), (dict(bands=[400, NAN]), ValueError),
    (dict(z="1"), TypeError), (dict(z=NAN), ValueError), (dict(z=np.inf), ValueError),
    (dict(reference="d"), TypeError), (dict(reference=NAN), ValueError),
    (dict(reference_field=1.0), TypeError), (dict(reference_field=2), IndexError), (dict(reference_field=-1), IndexError),
    (dict(sources=[1], reference_field=1), IndexError), (dict(reference_field=True), TypeError),
    (dict(dz=0.0), TypeError), (dict(dz="0"), TypeError), (dict(dz=[]), ValueError), (dict(dz=[0.0, 0.0]), ValueError),
    (dict(dz=[0.1, 0.0]), ValueError), (dict(dz=[0.0, NAN]), ValueError), (dict(dz=[0.0, np.inf]), ValueError),
    (dict(dz=np.arange(66.0)), ValueError), (dict(dz=[[0.0, 1.0]]), ValueError), (dict(dz=["a"]), TypeError),
    (dict(frequencies=10.0), TypeError), (dict(frequencies="10"), TypeError), (dict(frequencies=[]), ValueError),
    (dict(frequencies=np.arange(65.0)), ValueError), (dict(frequencies=[1.0, -1.0]), ValueError), (dict(frequencies=[NAN]), ValueError),
    (dict(frequencies=[np.inf]), ValueError), (dict(frequencies=[[1.0]]), ValueError), (dict(frequencies=[1j]), TypeError),
])
def test_argument_errors_come_before_the_device(kwargs, error, monkeypatch):
    from optrace_amd import raytracer
    monkeypatch.setattr(raytracer, "require_device", lambda: pytest.fail("the device was asked for before the arguments were checked"))
    with pytest.raises(error):
        tracer().mtf_analysis(**kwargs)


def test_good_arguments_reach_the_device_and_then_the_rays(monkeypatch):
    from optrace_amd import raytracer
    asked = []
    monkeypatch.setattr(raytracer, "require_device", lambda: asked.append(1))
    for kwargs in (dict(), dict(sources=[1, 0], section=0, bands=4, z=1.0, reference=550, reference_field=1, dz=np.arange(65.0),
                               frequencies=np.arange(64.0)),
                   dict(sources=(1,), bands=[400, 500.5, 700], dz=(-1, 0, 1), frequencies=[0])):
        with pytest.raises(RuntimeError, match="No rays traced"):
            tracer().mtf_analysis(**kwargs)
    assert len(asked) == 3
    freq, dz = mtf.check_arguments(None, None)
    assert freq is None and dz.tolist() == [0.0]
    freq, dz = mtf.check_arguments((0, 5), np.array([-1, 2]))
    assert freq.dtype == dz.dtype == np.float64 and freq.tolist() == [0, 5] and dz.tolist() == [-1, 2]


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_before_anything_else():
    lib = _capi.load_library()
    st = C.c_void_p()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)  # (never dereferenced: every call below returns from its checks)
    dn = lambda *v: (C.c_double * len(v))(*v)
    ranges = lambda *v: (C.c_int64 * len(v))(*v)
    INVALID, UNSUPPORTED = -1, -3

    def rays(N=100, nt=3, p=a, w=a, wl=a):
        r = _capi.Rays()
        r.N, r.nt, r.p, r.w, r.wl = N, nt, p, w, wl
        return C.byref(r)

    def refused(code, text, status):
        assert status == code and text.encode() in lib.ot_last_error(), (status, lib.ot_last_error())

    sums = lambda *args: lib.ot_mtf_sums(*args, st)
    #     0       1                     2  3  4  5  6  7            8  9                10         11 12 13 14 15
    ok = [rays(), ranges(0, 10, 20, 5), 2, 1, a, 0, 3, dn(0, 0, 0), a, dn(0, 1, 0.6, 0.8), dn(0.5, 1), 2, a, 4, a, a]
    for i in (0, 1, 4, 7, 8, 9, 10, 12, 14, 15):
        refused(INVALID, "ot_mtf_sums: null argument", sums(*[None if j == i else x for j, x in enumerate(ok)]))
    for R in (rays(p=None), rays(w=None)):
        refused(INVALID, "ot_mtf_sums: null argument", sums(R, *ok[1:]))
    for pair in ((-1, 5), (0, -1), (0, 101), (91, 10), (101, 0)):
        refused(INVALID, "ot_mtf_sums: ray range", sums(ok[0], ranges(0, 10, *pair), *ok[2:]))
    for k in (-1, 2, 100):
        refused(INVALID, "ot_mtf_sums: section", sums(*ok[:3], k, *ok[4:]))
    refused(INVALID, "ot_mtf_sums: a field starts before key_first", sums(*ok[:5], 1, *ok[6:]))
    for org in (dn(NAN, 0, 0), dn(0, np.inf, 0), dn(0, 0, -np.inf)):
        refused(INVALID, "ot_mtf_sums: origin", sums(*ok[:7], org, *ok[8:]))
    for t in (dn(NAN, 1, 0, 1), dn(0, 1, 0, np.inf)):
        refused(INVALID, "ot_mtf_sums: t not finite", sums(*ok[:9], t, *ok[10:]))
    for zeta in (dn(NAN, 1), dn(0, -np.inf)):
        refused(INVALID, "ot_mtf_sums: zeta not finite", sums(*ok[:10], zeta, *ok[11:]))
    for K in (0, -1, 33):
        refused(UNSUPPORTED, "ot_mtf_sums: n_fields outside 1 .. 64, n_bands outside 1 .. 32", sums(*ok[:6], K, *ok[7:]))
    for F in (0, -1, 65):
        refused(UNSUPPORTED, "ot_mtf_sums: n_fields outside 1 .. 64", sums(*ok[:2], F, *ok[3:]))
    for Z in (0, -1, 66):
        refused(UNSUPPORTED, "n_planes outside 1 .. 65", sums(*ok[:11], Z, *ok[12:]))
    for Q in (0, -1, 65):
        refused(UNSUPPORTED, "n_freq outside 1 .. 64", sums(*ok[:13], Q, *ok[14:]))
    # no ray in any field: nothing to do, whatever key_first is
    assert sums(ok[0], ranges(0, 0, 100, 0), *ok[2:5], 50, *ok[6:]) == 0
    refused(UNSUPPORTED, "ot_mtf_sums", sums(ok[0], ranges(0, 0, 100, 0), 2, 1, a, 0, 33, *ok[7:]))  # (the limits hold whatever the counts are)


def test_workspace():
    """Doubles: per field a list of partials as long as the longest field's -- a workgroup per 256 rays, at most
    max(16, 1024 / (groups * tiles)) per field and piece of 2^28 rays --, and per workgroup, group of KB = min(K, 4) bands and tile of
    TILE = 8 / KB (plane, frequency) pairs, 3 for KB = 3, a partial of KB x 4 x TILE doubles; 0 for arguments out of range."""
    lib = _capi.load_library()

    def ws(counts, K, Z, Q):
        return lib.ot_mtf_workspace((C.c_int64 * (2 * len(counts)))(*[v for n in counts for v in (0, n)]), len(counts), K, Z, Q)

    assert ws([1], 1, 1, 1) == 32 and ws([256], 3, 1, 8) == 3 * 36 and ws([257], 3, 1, 9) == 2 * 3 * 36
    assert ws([257, 0, 1], 2, 3, 64) == 3 * 2 * 48 * 32 and ws([0], 3, 1, 1) == 36 and ws([300], 5, 1, 1) == 2 * 2 * 32
    assert ws([10 ** 8], 1, 1, 8) == 1024 * 32 and ws([10 ** 8], 3, 1, 8) == 341 * 3 * 36 and ws([10 ** 8], 3, 9, 64) == 16 * 192 * 36
    assert ws([2 ** 28 + 1, 5], 32, 65, 64) == 2 * 17 * 8 * 2080 * 32
    for counts, K, Z, Q in (([257, 0, 3000], 3, 3, 64), ([70000], 4, 2, 3), ([5000, 9000], 32, 65, 1), ([1], 2, 1, 1)):
        assert ws(counts, K, Z, Q) == mc.workspace(counts, K, Z, Q)
    for counts, K, Z, Q in (([-1], 3, 1, 1), ([10], 0, 1, 1), ([10], 33, 1, 1), ([1] * 65, 1, 1, 1), ([], 1, 1, 1), ([10], 1, 0, 1),
                            ([10], 1, 66, 1), ([10], 1, 1, 0), ([10], 1, 1, 65)):
        assert ws(counts, K, Z, Q) == 0
    assert lib.ot_mtf_workspace(None, 1, 1, 1, 1) == 0


def test_constants_match_the_header():
    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "optrace_amd.h").read_text()
    value = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert value("OT_MTF_MAX_FREQ") == _capi.MTF_MAX_FREQ == mc.MAX_FREQ == 64
    assert value("OT_MTF_MAX_PLANES") == _capi.MTF_MAX_PLANES == mc.MAX_PLANES == 65
    assert value("OT_MTF_BLOCKS") == _capi.MTF_BLOCKS == 1024 and value("OT_MTF_MIN_BLOCKS") == _capi.MTF_MIN_BLOCKS == 16
    assert value("OT_ABI_VERSION") == _capi.ABI_VERSION == 9
    for name in ("ot_mtf_workspace", "ot_mtf_sums"):
        assert name in _capi.SIGNATURES and re.search(rf"\b{name}\(", text)
    assert ot.MTFAnalysis is mtf.MTFAnalysis and callable(ot.Raytracer.mtf_analysis)
