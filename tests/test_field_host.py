"""Field analysis without a device: the longdouble definition (tests/field_cases.py) on hand-made storages whose answers are known
by inspection, the argument checks of `Raytracer.field_analysis` and of the `ot_field_*` entry points, which come before any device
call, the host-only figures of `ot.FieldAnalysis` against a direct evaluation over all rays, and physical pins: the definition on
rays the C oracle traced through a single lens at three field angles -- no astigmatism on the axis, astigmatism that grows with the
square of the field, and foci that curve towards the lens."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd import field as fld

import field_cases as fc

NAN = np.nan
LD, EPS = fc.LD, fc.EPS
F64 = lambda a: np.asarray(a).astype(np.float64)
GRID = np.array([[x, y, 0.0] for x in (-1.0, -0.5, 0.5, 1.0) for y in (-1.0, -0.5, 0.5, 1.0)])


# ---- hand-made storages: two sections, section 0 analysed ---------------------------------------------------------------------------
def line_foci(starts, centre, z_u, z_v, u=(1.0, 0.0), reach=2.0):
    """Rays from `starts` (n, 3), all at z = 0, whose component along the unit vector u passes through centre . u at z = z_u and
    whose component across it, along v = (-u_y, u_x), through centre . v at z = z_v: two line foci.  -> p (n, 2, 3)."""
    starts, u = np.asarray(starts, dtype=np.float64), np.asarray(u, dtype=np.float64)
    v = np.array([-u[1], u[0]])
    su, sv = starts[:, :2] @ u, starts[:, :2] @ v
    mu, mv = (np.dot(centre, u) - su) / z_u, (np.dot(centre, v) - sv) / z_v
    m = mu[:, None] * u + mv[:, None] * v
    d = np.concatenate([m, np.ones((starts.shape[0], 1))], axis=1)
    return np.stack([starts, starts + reach * d], axis=1)


DIAG = np.array([1.0, 1.0]) / np.sqrt(2.0)
FIELD = np.array([[0.0, 0.0], [0.0, 1.0], [1.0, 1.0], [0.0, 2.0], [0.0, 3.0], [3.0, 0.0]])


def six_fields():
    """Field 0, on the axis: every ray through (0, 0, 8).  Field 1, at (0, 1): every x through 0.25 at z = 8, every y through 0.5
    at z = 16: t = (0, 1), so the tangential focus is 16 and the sagittal one 8.  Field 2, on the diagonal: along t through z = 4,
    across it through z = 8.  Between field 1 and 2 two rays that belong to no field.  Field 3: no rays.  Field 4: one ray.  Field
    5: three collimated rays.  Field 1 also holds a dead ray without a position and a ray within the plane z = 0."""
    a = line_foci(GRID, [0.0, 0.0], 8.0, 8.0)
    b = line_foci(GRID, [0.25, 0.5], 8.0, 16.0)
    extra = np.array([[[NAN] * 3] * 2, [[0.5, 0.5, 0.0], [1.5, 0.25, 0.0]]])
    gap = np.full((2, 2, 3), 1e30)
    gap[:, 1] = -1e30
    c = line_foci(GRID, [0.5, 0.5], 4.0, 8.0, u=DIAG)
    one = line_foci([[0.5, 0.25, 0.0]], [0.0, 0.0], 8.0, 8.0)
    par = np.array([[[0.0, 0, 0], [0.0, 0, 1]], [[1.0, 0, 0], [1.0, 0, 1]], [[0.0, 2.0, 0], [0.0, 2.0, 1]]])
    p = np.concatenate([a, b, extra, gap, c, one, par])
    N = p.shape[0]
    w = np.full((N, 2), 0.5, dtype=np.float32)
    w[32, 0] = 0  # the dead ray
    wl = np.full(N, 550.0, dtype=np.float32)
    fields = [(0, 16), (16, 18), (36, 16), (52, 0), (52, 1), (53, 3)]
    key = np.zeros(N, dtype=np.uint8)
    key[34:36] = fc.NO_BAND
    return p, w, wl, fields, key


def analysis(p, w, wl, fields, key, K, origin, z, field, power=None, means=None, **kwargs):
    val, mag = fc.records(p, w, wl, fields, 0, key, 0, K, origin, means=means)
    F = len(fields)
    a = ot.FieldAnalysis(F64(val), origin, z, 0, 0, 0, list(range(F)), field, np.ones(F) if power is None else power, **kwargs)
    return a, val, mag


def test_oracle_recovers_the_chosen_line_foci():
    p, w, wl, fields, key = six_fields()
    origin = (0.25, -0.5, 1.0)
    a, val, mag = analysis(p, w, wl, fields, key, 1, origin, 8.0, FIELD)
    assert np.all(np.isfinite(F64(val)[[0, 1, 2, 4, 5], 0, :8])) and np.all(np.isfinite(F64(mag))), "a dead ray's NaN or 1e30 reached a sum"
    assert a.band_N[:, 0].tolist() == [16, 16, 16, 0, 1, 3] and a.n_parallel[:, 0].tolist() == [0, 1, 0, 0, 0, 0]
    assert a.band_power[:, 0].tolist() == [8, 8, 8, 0, 0.5, 1.5]
    assert np.allclose(a.t, [[0, 1], [0, 1], DIAG, [0, 1], [0, 1], [1, 0]], rtol=0, atol=1e-16)
    tol = dict(rtol=0, atol=1e-13)
    assert np.allclose(a.focus_t[:3, 0], [8, 16, 4], **tol) and np.allclose(a.focus_s[:3, 0], [8, 8, 8], **tol)
    assert np.allclose(a.astigmatism[:3, 0], [0, 8, -4], **tol)
    # the best RMS focus of two line foci z_u, z_v of starts equally wide: (1 / z_u + 1 / z_v) / (1 / z_u^2 + 1 / z_v^2)
    assert np.allclose(a.focus_rms[:3, 0], [8, 9.6, 4.8], **tol)
    for name in ("focus_t", "focus_s", "focus_rms", "astigmatism", "field_curvature_t", "field_curvature_s", "field_curvature_rms"):
        assert np.all(np.isnan(getattr(a, name)[3:, 0])), f"{name}: no ray, one ray and collimated rays have no focus"
    assert np.allclose(a.field_curvature_t[:3, 0], [0, 8, -4], **tol) and np.allclose(a.field_curvature_s[:3, 0], [0, 0, 0], **tol)
    # on the plane z = 8: field 0 is a point; field 1 is a line along y, half as long as the starts are wide
    assert a.rms_radius[0, 0] < 1e-14 and a.rms_s[1, 0] < 1e-14 and a.rms_t[2, 0] > 0.1 and a.rms_s[2, 0] < 1e-14
    half = np.sqrt(np.mean(GRID[:, 1] ** 2)) / 2
    assert a.rms_t[1, 0] == pytest.approx(half, rel=1e-14) and a.rms_radius[1, 0] == pytest.approx(half, rel=1e-14)
    # (field 2 runs on along t beyond its focus at z = 4: twice as far out at z = 8)
    assert np.allclose(a.centroid[:3, 0], [[0, 0], [0.25, 0.25], [1.0, 1.0]], **tol)
    assert a.rms_radius[4, 0] == 0 and a.rms_t[4, 0] == 0 and a.rms_s[4, 0] == 0 and np.isnan(a.rms_radius_best[4, 0])
    assert np.all(np.isnan(a.centroid[3])) and np.isnan(a.rms_radius[3, 0])
    assert a.rms_radius_best[0, 0] < 1e-14 and a.rms_radius_best[1, 0] < a.rms_radius[1, 0]
    # collimated rays keep their spot: (0, 0), (1, 0), (0, 2) about (1 / 3, 2 / 3)
    assert a.rms_radius[5, 0] == pytest.approx(np.sqrt((2 / 9 + 4 / 9 + 2 * 4 / 9 + 16 / 9) / 3), rel=1e-14)
    assert np.allclose(a.transmission, [8, 8, 8, 0, 0.5, 1.5]) and a.relative_illumination.tolist() == [1, 1, 1, 0, 0.0625, 0.1875]


def test_oracle_records_by_inspection():
    p, w, wl, fields, key = six_fields()
    val, _ = fc.records(p, w, wl, fields, 0, key, 0, 2, (0.0, 0.0, 0.0))
    v = F64(val)
    # field 0: a = start, m = -start / 8, symmetric starts: the first moments vanish, sum w x^2 = 0.5 * 8 * (1 + 0.25) * 2 / 2
    assert v[0, 0, :8].tolist() == [8, 16, 0, 0, 0, 0, 4400, 0] and v[0, 0, 8] == 5 and v[0, 0, 9] == 0 and v[0, 0, 10] == 5
    assert v[0, 0, 11] == -5 / 8 and v[0, 0, 14] == -5 / 8 and v[0, 0, 15] == 5 / 64 and v[0, 0, 12] == 0 == v[0, 0, 13]
    assert np.all(v[:, 1, :8] == 0) and np.all(np.isnan(v[:, 1, 8:])), "band 1 holds no ray"
    assert v[3, 0, :8].tolist() == [0] * 8 and np.all(np.isnan(v[3, 0, 8:]))
    assert v[1, 0, 7] == 1 and v[1, 0, 1] == 16
    assert v[4, 0, :2].tolist() == [0.5, 1] and np.all(v[4, 0, 8:] == 0)
    # means handed in are taken as they are
    means = np.zeros((6, 2, 4))
    means[0, 0] = [1, 0, 0, 0]
    val2, _ = fc.records(p, w, wl, fields, 0, key, 0, 2, (0.0, 0.0, 0.0), means=means)
    assert F64(val2)[0, 0, 8] == 5 + 8 and F64(val2)[0, 0, 10] == 5
    assert fc.record_means(v)[0, 0].tolist() == [0, 0, 0, 0] and np.all(np.isnan(fc.record_means(v)[3, 0]))


def random_fields(seed=5, n=200):
    """Three fields of n rays, two bands, aberrated bundles towards (0, 0.3 f, 20 + 0.2 f) with an astigmatic spread; some dead."""
    rng = np.random.default_rng(seed)
    ps, ws = [], []
    for f in range(3):
        starts = np.concatenate([rng.normal(size=(n, 2)) * [2.0, 1.5] + [0.1, 0.4 * f], np.zeros((n, 1))], axis=1)
        q = line_foci(starts, [0.0, 0.3 * f], 20.0 + 0.2 * f, 20.0 - 0.5 * f, u=(0.0, 1.0) if f < 2 else DIAG, reach=1.5)
        q[:, 1, :2] += rng.normal(size=(n, 2)) * 1e-3
        wt = rng.uniform(0.1, 1, size=(n, 2)).astype(np.float32)
        dead = rng.uniform(size=n) < 0.1
        wt[dead, 0], q[dead] = 0, NAN
        ps.append(q)
        ws.append(wt)
    p, w = np.concatenate(ps), np.concatenate(ws)
    wl = rng.choice(np.array([480.0, 640.0], dtype=np.float32), size=3 * n)
    key = (wl > 500).astype(np.uint8)
    return p, w, wl, [(0, n), (n, n), (2 * n, n)], key


def test_derived_figures_against_a_direct_evaluation():
    p, w, wl, fields, key = random_fields()
    origin, z = np.array([0.05, -0.1, 2.0]), 19.75
    field = np.array([[0.0, 0.0], [0.0, 0.4], [0.5, 0.5]])
    parax = np.array([[[0.0, 0.0]] * 2, [[0.0, 0.31], [0.0, 0.29]], [[0.4, 0.4], [0.45, 0.41]]])
    a, val, _ = analysis(p, w, wl, fields, key, 2, origin, z, field, power=[100.0, 50.0, 200.0], paraxial=parax, long_desc="by hand")
    assert a.records.shape == (3, 2, 18) and a.long_desc == "by hand" and a.z == z and a.n_fields == 3 and a.n_bands == 2
    close = lambda got, want, tol: np.allclose(got, np.float64(want), rtol=tol, atol=1e-15, equal_nan=True)
    for f, (first, count) in enumerate(fields):
        for b in range(2):
            d = fc.direct(p, w, first, count, 0, key[first:first + count] == b, origin, z, a.t[f])
            assert a.band_N[f, b] == d["band_N"] > 50 and close(a.band_power[f, b], d["band_power"], 1e-15)
            assert close(a.centroid[f, b], F64(d["centroid"]), 1e-12)
            for name, tol in (("focus_t", 1e-10), ("focus_s", 1e-10), ("focus_rms", 1e-10), ("rms_t", 1e-10), ("rms_s", 1e-10),
                              ("rms_radius", 1e-10), ("rms_radius_best", 1e-8)):
                assert close(getattr(a, name)[f, b], d[name], tol), f"{name} of field {f}, band {b}: {getattr(a, name)[f, b]} against {d[name]}"
            assert a.astigmatism[f, b] == a.focus_t[f, b] - a.focus_s[f, b]
            assert a.field_curvature_t[f, b] == a.focus_t[f, b] - a.focus_rms[0, b]
            assert a.field_curvature_s[f, b] == a.focus_s[f, b] - a.focus_rms[0, b] and a.field_curvature_rms[0, b] == 0
            assert a.rms_radius_best[f, b] <= a.rms_radius[f, b]
            assert a.rms_radius[f, b] == pytest.approx(np.hypot(a.rms_t[f, b], a.rms_s[f, b]), rel=1e-12)
    # the astigmatic spread put in: 0.2 f + 0.5 f between the line foci, to the noise on the directions
    assert np.allclose(a.astigmatism[:, 0], [0, 0.7, 1.4], atol=0.1) and np.allclose(a.astigmatism[:, 1], [0, 0.7, 1.4], atol=0.1)
    ww = np.where(np.isnan(w[:, 0]), 0, w[:, 0]).astype(LD)
    for b, lam in enumerate((480.0, 640.0)):
        assert a.wavelengths[b] == pytest.approx(lam, rel=1e-15)
    for f, (first, count) in enumerate(fields):
        used, inside, _ = fc.lines(p, w, first, count, 0, origin)
        total = float(ww[first:first + count][inside].sum())
        assert a.transmission[f] == pytest.approx(total / [100.0, 50.0, 200.0][f], rel=1e-14)
    assert np.allclose(a.relative_illumination, a.transmission / a.transmission[0], rtol=1e-15)
    # distortion against its definition; NaN where the paraxial image is on the axis
    assert np.all(np.isnan(a.distortion[0]))
    for f in (1, 2):
        for b in range(2):
            h = parax[f, b]
            want = (np.dot(a.centroid[f, b], h) / np.linalg.norm(h) - np.linalg.norm(h)) / np.linalg.norm(h)
            assert a.distortion[f, b] == pytest.approx(want, rel=1e-12)
    # another reference field
    b2 = ot.FieldAnalysis(a.records, origin, z, 1, 2, 0, [4, 2, 7], field, [100.0, 50.0, 200.0])
    assert b2.sources.tolist() == [4, 2, 7] and b2.reference_band == 1 and b2.relative_illumination[2] == 1
    assert np.array_equal(b2.field_curvature_t, b2.focus_t - b2.focus_rms[2][None, :]) and np.all(np.isnan(b2.paraxial))


def test_result_object_is_locked_and_checks_its_shapes():
    rec = np.zeros((2, 1, 18))
    rec[1, :, 8:] = NAN
    rec[0, 0] = [2, 4, 1, -0.5, 0, 0, 1100, 0, 1, 0, 1, -0.25, 0, 0, -0.125, 0.0625, 0, 0.015625]
    args = dict(records=rec, origin=[0, 0, 1], z=5.0, reference_band=0, reference_field=0, section=3, sources=[0, 1],
                field=[[0, 0], [0, 1]], power=[4, 4])
    a = ot.FieldAnalysis(**args)
    assert a.band_N.tolist() == [[4], [0]] and a.centroid[0, 0].tolist() == [0.5, -0.25] and a.wavelengths.tolist() == [550]
    assert a.focus_t[0, 0] == 1 + 0.125 / 0.015625 and a.focus_s[0, 0] == 1 + 0.25 / 0.0625 and a.astigmatism[0, 0] == 4
    assert a.transmission.tolist() == [0.5, 0] and a.relative_illumination.tolist() == [1, 0]
    with pytest.raises(RuntimeError):
        a.z = 1.0
    with pytest.raises(ValueError):
        a.focus_t[0] = 1
    with pytest.raises(AttributeError):
        a.something_else = 1
    for bad in (dict(band_edges=[400, 500, 600]), dict(reference_band=1), dict(reference_band=-2), dict(reference_field=2),
                dict(reference_field=-1), dict(sources=[0, 1, 2]), dict(field=[[0, 0]]), dict(power=[1])):
        with pytest.raises(ValueError):
            ot.FieldAnalysis(**{**args, **bad})
    with pytest.raises(ValueError):
        ot.FieldAnalysis(np.zeros((1, 33, 18)), [0, 0, 0], 0.0, 0, 0, 0, [0], [[0, 0]], [1])
    with pytest.raises(ValueError):
        ot.FieldAnalysis(np.zeros((65, 1, 18)), [0, 0, 0], 0.0, 0, 0, 0, list(range(65)), np.zeros((65, 2)), np.ones(65))
    # the empty result: what the caller fixed stays, every figure NaN
    e = fld._empty(3, np.array([400.0, 500, 600]), None, [0, 0, 1], 1, [3, 1], [[0, 0], [0, 1]], [1, 1])
    assert e.n_bands == 2 and e.n_fields == 2 and e.reference_band == -1 and e.reference_field == 1 and np.isnan(e.z)
    assert e.band_N.tolist() == [[0, 0], [0, 0]] and e.sources.tolist() == [3, 1] and e.transmission.tolist() == [0, 0]
    for f in (e.focus_t, e.focus_s, e.focus_rms, e.centroid, e.wavelengths, e.rms_radius, e.rms_radius_best, e.distortion, e.astigmatism):
        assert np.all(np.isnan(f))
    e = fld._empty(0, "lines", 2.5, [0, 0, 0], 0, [0], [[0, 0]], [1])
    assert e.n_bands == 1 and e.z == 2.5 and e.band_edges is None


def test_paraxial_images():
    M = lambda wl, zg, zb: np.array([[-2.0, 0.5], [0.0, -0.5]]) if wl < 600 else None
    out = fld.paraxial_images(M, [500.0, 650.0, NAN], [[0.0, 1.0, -20.0], [0.5, 0.0, -20.0]], [[0.0, 0.0], [0.0, 0.1]], 5.0)
    assert out.shape == (2, 3, 2) and out[0, 0].tolist() == [0, -2] and out[1, 0].tolist() == [-1, 0.05] and np.all(np.isnan(out[:, 1:]))
    assert np.all(np.isnan(fld.paraxial_images(None, [500.0], [[0.0, 1.0, -20.0]], [[0.0, 0.0]], 5.0)))
    assert np.all(np.isnan(fld.paraxial_images(M, [500.0], [[0.0, 1.0, -20.0]], [[NAN, NAN]], 5.0)))


# ---- Raytracer.field_analysis: arguments ----------------------------------------------------------------------------------------------
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
    (dict(paraxial="abcd"), ValueError), (dict(paraxial=1), ValueError),
])
def test_argument_errors_come_before_the_device(kwargs, error, monkeypatch):
    from optrace_amd import raytracer
    monkeypatch.setattr(raytracer, "require_device", lambda: pytest.fail("the device was asked for before the arguments were checked"))
    with pytest.raises(error):
        tracer().field_analysis(**kwargs)


def test_good_arguments_reach_the_device_and_then_the_rays(monkeypatch):
    from optrace_amd import raytracer
    asked = []
    monkeypatch.setattr(raytracer, "require_device", lambda: asked.append(1))
    for kwargs in (dict(), dict(sources=[1, 0], section=0, bands=4, z=1.0, reference=550, reference_field=1, paraxial=None),
                   dict(sources=(1,), bands=[400, 500.5, 700])):
        with pytest.raises(RuntimeError, match="No rays traced"):
            tracer().field_analysis(**kwargs)
    assert len(asked) == 3
    sources, bands, z, ref = fld.check_arguments(2, 3, np.array([2, 0]), 0, [400, 500], 3, np.float32(550), 1, "tma")
    assert sources == [2, 0] and bands.tolist() == [400, 500] and (z, ref) == (3.0, 550.0)
    assert fld.check_arguments(2, 3, None, None, "lines", None, None, 2, None)[0] == [0, 1, 2]
    with pytest.raises(RuntimeError, match="Ray Sources Missing"):
        fld.check_arguments(2, 0, None, None, "lines", None, None, 0, None)


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_before_anything_else():
    lib = _capi.load_library()
    st = C.c_void_p()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)  # (never dereferenced: every call below returns from its checks)
    d3 = lambda *v: (C.c_double * 3)(*v)
    ranges = lambda *v: (C.c_int64 * len(v))(*v)
    INVALID, UNSUPPORTED = -1, -3

    def rays(N=100, nt=3, p=a, w=a, wl=a):
        r = _capi.Rays()
        r.N, r.nt, r.p, r.w, r.wl = N, nt, p, w, wl
        return C.byref(r)

    def refused(code, text, status):
        assert status == code and text.encode() in lib.ot_last_error(), (status, lib.ot_last_error())

    sums = lambda *args: lib.ot_field_sums(*args, st)
    ok = [rays(), ranges(0, 10, 20, 5), 2, 1, a, 0, 3, d3(0, 0, 0), a, a]
    for i in (0, 1, 4, 7, 8, 9):
        refused(INVALID, "ot_field_sums: null argument", sums(*[None if j == i else x for j, x in enumerate(ok)]))
    for R in (rays(p=None), rays(w=None), rays(wl=None)):
        refused(INVALID, "ot_field_sums: null argument", sums(R, *ok[1:]))
    for pair in ((-1, 5), (0, -1), (0, 101), (91, 10), (101, 0)):
        refused(INVALID, "ot_field_sums: ray range", sums(ok[0], ranges(0, 10, *pair), *ok[2:]))
    for k in (-1, 2, 100):
        refused(INVALID, "ot_field_sums: section", sums(*ok[:3], k, *ok[4:]))
    refused(INVALID, "ot_field_sums: a field starts before key_first", sums(*ok[:5], 1, *ok[6:]))
    for org in (d3(NAN, 0, 0), d3(0, np.inf, 0), d3(0, 0, -np.inf)):
        refused(INVALID, "ot_field_sums: origin", sums(*ok[:7], org, *ok[8:]))
    for K in (0, -1, 33):
        refused(UNSUPPORTED, "ot_field_sums: n_fields outside 1 .. 64 or n_bands outside 1 .. 32", sums(*ok[:6], K, *ok[7:]))
    for F in (0, -1, 65):
        refused(UNSUPPORTED, "ot_field_sums: n_fields outside 1 .. 64", sums(*ok[:2], F, *ok[3:]))
    # no ray in any field: nothing to do, whatever key_first is
    assert sums(ok[0], ranges(0, 0, 100, 0), *ok[2:5], 50, *ok[6:]) == 0
    refused(UNSUPPORTED, "ot_field_sums", sums(ok[0], ranges(0, 0, 100, 0), 2, 1, a, 0, 33, *ok[7:]))  # (the limits hold whatever the counts are)


def test_workspace():
    """Doubles: per field a list of partials as long as the longest field's -- a workgroup per 256 rays, at most 1024 per field and
    piece of 2^28 rays --, 10 per band and workgroup, and the sums of both passes, 18 per cell; 0 for arguments out of range."""
    lib = _capi.load_library()
    ws = lambda counts, K: lib.ot_field_workspace((C.c_int64 * (2 * len(counts)))(*[v for n in counts for v in (0, n)]), len(counts), K)
    assert ws([1], 1) == 10 + 18 and ws([256], 3) == 3 * 28 and ws([257], 3) == 3 * (20 + 18)
    assert ws([257, 0, 1], 2) == 2 * (3 * 2 * 10 + 3 * 18)
    assert ws([256 * 1024], 5) == ws([10 ** 8], 5) == 5 * (1024 * 10 + 18) and ws([2 ** 28 + 1, 5], 32) == 32 * (2 * 1025 * 10 + 2 * 18)
    assert ws([0], 3) == 3 * 28
    for counts, K in (([-1], 3), ([10], 0), ([10], 33), ([1] * 65, 1), ([], 1)):
        assert ws(counts, K) == 0
    assert lib.ot_field_workspace(None, 1, 1) == 0


def test_constants_match_the_header():
    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "optrace_amd.h").read_text()
    value = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert value("OT_FIELD_M") == _capi.FIELD_M == fc.M == 18
    assert value("OT_FIELD_MAX_FIELDS") == _capi.FIELD_MAX_FIELDS == fc.MAX_FIELDS == 64
    assert value("OT_FIELD_BLOCKS") == _capi.FIELD_BLOCKS == 1024
    assert value("OT_CHROM_MAX_BANDS") == fc.MAX_BANDS == 32 and _capi.CHROM_NO_BAND == fc.NO_BAND == 255
    assert value("OT_ABI_VERSION") == _capi.ABI_VERSION == 9
    for name in ("ot_field_workspace", "ot_field_sums"):
        assert name in _capi.SIGNATURES and re.search(rf"\b{name}\(", text)
    assert ot.FieldAnalysis is fld.FieldAnalysis and callable(ot.Raytracer.field_analysis)


# ---- physical pins ----------------------------------------------------------------------------------------------------------------------
THETA = 2.0  # degrees


def traced_fields(theta_deg):
    """Collimated bundles at the field angles 0, theta and 2 theta about the x axis through the single lens of `c1_single_lens`,
    traced by the C oracle: per field 48 rays on 4 rings of 12 about the chief ray, which goes through the front vertex -- a set
    symmetric under a quarter turn about the chief direction.  -> (p, w, wl, fields, section, origin, field (3, 2))"""
    from optrace_amd.scene import CompiledScene
    import oracle_bridge as ob
    import scenes
    with ot.global_options.no_warnings():
        RT = scenes.c1_single_lens(ot)
    RT._geometry_checks()
    assert not RT.geometry_error
    sc = CompiledScene(RT)
    vertex = np.array([0.0, 0.0, float(RT.lenses[0].front.pos[2])])
    rings, spokes, radius = 4, 12, 0.05
    rho = radius * np.sqrt((np.arange(rings) + 0.5) / rings)
    phi = 2 * np.pi * (np.arange(spokes) + 0.5) / spokes
    Rr, P = np.meshgrid(rho, phi, indexing="ij")
    p0, s0, pol0 = [], [], []
    for mult in (0, 1, 2):
        th = np.deg2rad(mult * theta_deg)
        s = np.array([0.0, np.sin(th), np.cos(th)])
        e1, e2 = np.array([1.0, 0.0, 0.0]), np.cross(s, [1.0, 0.0, 0.0])
        off = (Rr * np.cos(P)).reshape(-1, 1) * e1 + (Rr * np.sin(P)).reshape(-1, 1) * e2
        p0.append(vertex - 5.0 * s + off)
        s0.append(np.tile(s, (off.shape[0], 1)))
        pol0.append(off / np.linalg.norm(off, axis=1)[:, None])  # (radial: the weights behind the lens share the set's symmetry)
    p0, s0, pol0 = np.concatenate(p0), np.concatenate(s0), np.concatenate(pol0)
    N, n = p0.shape[0], rings * spokes
    wl = np.full(N, 550.0, dtype=np.float32)
    rays = ob.HostRays(N, sc.nt, False)
    rays.set_initial(p0, s0, pol0, np.full(N, 1.0 / N, dtype=np.float32), wl)
    _, status = ob.trace(sc.desc, rays, None)
    assert status == 0
    p, w, k = np.array(rays.p_list), np.array(rays.w_list), sc.nt - 2
    assert np.all(w[:, k] > 0)
    from optrace_amd.scene import SectionTable
    origin = np.array(SectionTable(RT).origin(k, None), dtype=np.float64)
    tan = np.tan(np.deg2rad(theta_deg * np.arange(3)))
    return p, w, wl, [(0, n), (n, n), (2 * n, n)], k, origin, np.stack([np.zeros(3), tan], axis=1)


def foci_of(theta_deg):
    p, w, wl, fields, k, origin, field = traced_fields(theta_deg)
    key = np.zeros(p.shape[0], dtype=np.uint8)
    val, mag = fc.records(p, w, wl, fields, k, key, 0, 1, origin)
    a = ot.FieldAnalysis(F64(val), origin, float(origin[2]) + 8.0, 0, 0, k, [0, 1, 2], field, np.ones(3))
    return a, val, mag, p


RATIO_OFF_THETA, RATIO_OFF_HALF = 1.605e-2, 4.018e-3  # measured at THETA and at THETA / 2


def test_astigmatism_and_field_curvature_of_a_single_lens():
    """The biconvex lens of `c1_single_lens` (n = 1.5, R = +-8 mm), collimated bundles of 0.05 mm radius at 0, theta and 2 theta,
    theta = 2 degrees, traced by the C oracle; the definition in longdouble, the figures through `ot.FieldAnalysis`.
    1. On the axis the ray set is symmetric under a quarter turn, so the tangential and the sagittal focus coincide up to the
       rounding of the traced positions: a position carries a few eps of its magnitude (below 16 mm here; 32 eps allowed for the
       operations of two surfaces), which moves a line focus by that over the RMS slope about the mean, sqrt(V / W); the two foci
       may differ by twice that.
    2. Third order: astigmatism grows with the square of the field, astigmatism(2 theta) / astigmatism(theta) -> 4.  Measured
       |ratio - 4|: 1.605e-2 at theta = 2 degrees, 4.018e-3 at 1 degree -- a quarter at half the field, as the next order of the aberration
       would have it and rounding would not.  The test allows twice the value measured at theta.
    3. Both foci curve towards the lens, the tangential one more: focus_t < focus_s < the focus on the axis, at theta and more so
       at 2 theta."""
    a, val, mag, p = foci_of(THETA)
    v = F64(val)
    slope = np.sqrt((v[0, 0, 15] + v[0, 0, 17]) / 2 / v[0, 0, 0])
    tol = 2 * 32 * EPS * 16.0 / slope
    print(f"on the axis: focus_t - focus_s = {a.astigmatism[0, 0]:.3e}, allowed {tol:.3e}; foci t {a.focus_t[:, 0]}, s {a.focus_s[:, 0]}")
    assert abs(a.astigmatism[0, 0]) <= tol
    ratio = a.astigmatism[2, 0] / a.astigmatism[1, 0]
    half = foci_of(THETA / 2)[0]
    ratio_half = half.astigmatism[2, 0] / half.astigmatism[1, 0]
    print(f"astigmatism {a.astigmatism[:, 0]}, ratio - 4 = {ratio - 4:.3e}; at half the field {half.astigmatism[:, 0]}, {ratio_half - 4:.3e}")
    assert abs(ratio - 4) <= 2 * RATIO_OFF_THETA
    assert 0.5 * RATIO_OFF_THETA < abs(ratio - 4), "the measured value stands in the docstring and in DESIGN.md"
    assert abs(ratio_half - 4) < 0.5 * abs(ratio - 4), "the deviation from the third-order law shrinks with the field"
    assert abs(ratio_half - 4) == pytest.approx(RATIO_OFF_HALF, rel=0.5)
    ft, fs = a.focus_t[:, 0], a.focus_s[:, 0]
    assert ft[2] < ft[1] < ft[0] and fs[2] < fs[1] < fs[0] and ft[1] < fs[1] and ft[2] < fs[2]
    assert np.all(a.astigmatism[1:, 0] < 0) and np.all(a.field_curvature_t[1:, 0] < a.field_curvature_s[1:, 0])
