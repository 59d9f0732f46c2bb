"""Raytracer.huygens_field without a device: the argument checks of the method and of the `ot_psf_field_*` entry points, the
workspace formula, the result object on hand-made arrays, the NumPy restatement of the transfer function (step 4 of DESIGN.md
"Huygens PSF across the field") against `psf.diffraction_mtf`, and the diffraction-limit curve."""
import ctypes as C

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd import psf as hp
from optrace_amd import psf_field as pf

import psf_cases as pc
from wavefront_cases import EPS, LD

NAN, INF = float("nan"), float("inf")


# ---- Raytracer.huygens_field: arguments --------------------------------------------------------------------------------------------------
def tracer():
    RT = ot.Raytracer(outline=[-1, 1, -1, 1, -1, 10])
    RT.add(ot.RaySource(ot.Point(), pos=[0, 0, 0]))
    RT.add(ot.RaySource(ot.Point(), pos=[0, 0.5, 0]))
    return RT


@pytest.mark.parametrize("kwargs,error", [
    (dict(sources=1), TypeError), (dict(sources=[]), ValueError), (dict(sources=[0.0]), TypeError), (dict(sources=[0, 2]), IndexError),
    (dict(sources=[1, 1]), ValueError), (dict(sources=list(range(65))), ValueError),
    (dict(section=1.0), TypeError), (dict(section=-1), ValueError), (dict(section=1), ValueError),
    (dict(bands="bands"), ValueError), (dict(bands=2.0), TypeError), (dict(bands=0), ValueError), (dict(bands=33), ValueError),
    (dict(bands=[500, 400]), ValueError),
    (dict(n_px=64.0), TypeError), (dict(n_px=0), ValueError), (dict(n_px=1025), ValueError),
    (dict(size="1"), TypeError), (dict(size=0.0), ValueError), (dict(size=-1.0), ValueError), (dict(size=NAN), ValueError),
    (dict(size=INF), ValueError), (dict(size=[0.1, 0.1]), TypeError),
    (dict(dz="0"), TypeError), (dict(dz=NAN), ValueError), (dict(dz=[]), ValueError), (dict(dz=[0.0, INF]), ValueError),
    (dict(dz=[[0.0, 0.1]]), ValueError), (dict(dz=list(np.linspace(0, 1, 65))), ValueError),
    (dict(focus=1.0), TypeError), (dict(focus=[0, 0, 1.0]), ValueError), (dict(focus=[[0, 0, 1.0]]), ValueError),
    (dict(focus=[[0, 0, NAN], [0, 0, 1]]), ValueError), (dict(sources=[1], focus=[[0, 0, 1], [0, 0, 1]]), ValueError),
    (dict(radius="1"), TypeError), (dict(radius=0.0), ValueError), (dict(radius=NAN), ValueError), (dict(radius=[1.0]), ValueError),
    (dict(radius=[1.0, 0.0]), ValueError), (dict(radius=[1.0, INF]), ValueError),
    (dict(frequencies=10.0), TypeError), (dict(frequencies=[]), ValueError), (dict(frequencies=[[0.0, 1.0]]), ValueError),
    (dict(frequencies=[0.0, -1.0]), ValueError), (dict(frequencies=[0.0, NAN]), ValueError), (dict(frequencies=["a"]), TypeError),
    (dict(frequencies=list(range(65))), ValueError),
    (dict(n_px=8, size=0.1, frequencies=[0.0, 40.0, 40.001]), ValueError),  # (the sampling limit is 8 / 0.2 = 40 cycles / mm)
    (dict(reference="d"), TypeError), (dict(reference=NAN), ValueError),
    (dict(reference_field=1.0), TypeError), (dict(reference_field=2), IndexError), (dict(sources=[1], reference_field=1), IndexError),
])
def test_argument_errors_come_before_the_device(kwargs, error, monkeypatch):
    from optrace_amd import raytracer
    monkeypatch.setattr(raytracer, "require_device", lambda: pytest.fail("the device was asked for before the arguments were checked"))
    with pytest.raises(error):
        tracer().huygens_field(**kwargs)


def test_good_arguments_reach_the_device_and_then_the_rays(monkeypatch):
    from optrace_amd import raytracer
    asked = []
    monkeypatch.setattr(raytracer, "require_device", lambda: asked.append(1))
    for kwargs in (dict(), dict(sources=[1, 0], section=0, bands=4, n_px=1024, size=0.5, dz=[0.1, -0.1, 0.1], focus=[[0, 0, 5], [0, 1, 5.0]],
                                radius=-4, frequencies=[0, 1024.0], reference=550, reference_field=1),
                   dict(sources=(1,), bands=[400, 500.5, 700], focus=np.array([[0, 0, 1.0]]), radius=np.array([2.5]), n_px=1,
                        frequencies=np.array([3.0]), dz=np.zeros(64))):
        with pytest.raises(RuntimeError, match="No rays traced"):
            tracer().huygens_field(**kwargs)
    assert len(asked) == 3
    size, dz, focus, radius, freq = pf.check_arguments(3, 2, None, 8, np.float32(0.5), [0.2, 0.1], [[0, 0, 1], [1, 0, 1]], 3, (0, 8))
    assert size == 0.5 and dz.tolist() == [0.2, 0.1] and focus.dtype == np.float64 and radius.tolist() == [3, 3] and freq.tolist() == [0, 8]
    assert pf.check_arguments(3, 1, None, 8, None, 0.0, None, None, None)[2:] == (None, None, None)
    # without a size the limit is not known yet: the check waits for it
    assert pf.check_arguments(3, 1, None, 8, None, 0.0, None, None, [1e9])[4].tolist() == [1e9]
    with pytest.raises(ValueError, match="sampling limit"):
        pf.check_frequencies(np.array([0.0, 41.0]), 8, 0.1)
    pf.check_frequencies(np.array([0.0, 40.0]), 8, 0.1)


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_before_anything_else():
    """In the manner of `psf_cases.entry_point_argument_checks`: the OT_ERR_* code and the entry's name in `ot_last_error`, before a
    device is looked for and so without a launch: the addresses below are never dereferenced."""
    lib = _capi.load_library()
    st = C.c_void_p()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    INVALID, UNSUPPORTED = -1, -3
    i64s = lambda *v: (C.c_int64 * len(v))(*v)
    dbl = lambda *v: (C.c_double * len(v))(*v)

    def rays(N=100, nt=4, p=a, w=a, n=a, wl=a):
        r = _capi.Rays()
        r.N, r.nt, r.p, r.w, r.n, r.wl = N, nt, p, w, n, wl
        return C.byref(r)

    def refused(code, name, rc):
        assert rc == code, (name, rc, lib.ot_last_error())
        assert name.encode() in lib.ot_last_error(), lib.ot_last_error()

    swap = lambda ok, i, v: [v if j == i else x for j, x in enumerate(ok)]

    rays_ = lambda *args: lib.ot_psf_field_rays(*args, st)
    ok = [rays(), i64s(0, 10, 20, 5), 2, 2, a, 0, 30, 3, a, a, a, a]
    for i in (0, 1, 4, 8, 9, 10, 11):
        refused(INVALID, "ot_psf_field_rays: null argument", rays_(*swap(ok, i, None)))
    for missing in ("p", "w", "n", "wl"):
        refused(INVALID, "ot_psf_field_rays: null argument", rays_(rays(**{missing: None}), *ok[1:]))
    for F in (0, -1):
        refused(INVALID, "ot_psf_field_rays: n_fields or n_bands below 1", rays_(*swap(ok, 2, F)))
    refused(INVALID, "ot_psf_field_rays: n_fields or n_bands below 1", rays_(*swap(ok, 7, 0)))
    refused(UNSUPPORTED, "ot_psf_field_rays: n_fields above 64 or n_bands above 32", rays_(*swap(ok, 2, 65)))
    refused(UNSUPPORTED, "ot_psf_field_rays: n_fields above 64 or n_bands above 32", rays_(*swap(ok, 7, 33)))
    for k in (-1, 3, 100):
        refused(INVALID, "ot_psf_field_rays: section", rays_(*swap(ok, 3, k)))
    for key_first, span in ((-1, 30), (0, -1), (80, 30)):
        refused(INVALID, "ot_psf_field_rays: ray range", rays_(*ok[:5], key_first, span, *ok[7:]))
    for pair in ((-1, 5), (0, -1), (95, 10)):
        refused(INVALID, "ot_psf_field_rays: ray range", rays_(*swap(ok, 1, i64s(0, 10, *pair))))
    refused(INVALID, "ot_psf_field_rays: a field outside the span", rays_(*swap(ok, 6, 24)))
    refused(INVALID, "ot_psf_field_rays: a field outside the span", rays_(*swap(ok, 5, 1)))
    assert rays_(*swap(ok, 1, i64s(0, 0, 0, 0))[:6], 0, *ok[7:]) == 0

    sum_ = lambda *args: lib.ot_psf_field_sum(*args, st)
    ok = [10, a, 2, 2, i64s(0, 3, 3, 9, 10), dbl(5.0, -4.0), 8, 0.1, 2, dbl(0.0, 0.1), a, a, a, a]
    for i in (1, 4, 5, 9, 10, 11, 12, 13):
        refused(INVALID, "ot_psf_field_sum: null argument", sum_(*swap(ok, i, None)))
    refused(INVALID, "ot_psf_field_sum", sum_(*swap(ok, 0, -1)))
    for i, low, high, text in ((2, 0, 65, "n_fields"), (3, 0, 33, "n_bands"), (6, 0, 1025, "n_px"), (8, 0, 65, "n_planes")):
        refused(INVALID, f"ot_psf_field_sum: {text} below 1", sum_(*swap(ok, i, low)))
        refused(UNSUPPORTED, f"ot_psf_field_sum: {text} above {high - 1}", sum_(*swap(ok, i, high)))
    refused(UNSUPPORTED, "ot_psf_field_sum: n_px above 1024", sum_(0, *swap(ok, 6, 1025)[1:]))  # (the limits hold whatever n is)
    for starts in (i64s(1, 3, 3, 9, 10), i64s(0, 3, 3, 9, 11)):
        refused(INVALID, "ot_psf_field_sum: starts do not run from 0 to n", sum_(*swap(ok, 4, starts)))
    refused(INVALID, "ot_psf_field_sum: starts not ascending", sum_(*swap(ok, 4, i64s(0, 4, 3, 9, 10))))
    for size in (0.0, -1.0, INF, NAN):
        refused(INVALID, "ot_psf_field_sum: size", sum_(*swap(ok, 7, size)))
    for dz in (dbl(0.0, INF), dbl(NAN, 0.0)):
        refused(INVALID, "ot_psf_field_sum: dz", sum_(*swap(ok, 9, dz)))
    for radius in (dbl(5.0, 0.0), dbl(NAN, 1.0), dbl(1.0, INF)):
        refused(INVALID, "ot_psf_field_sum: radius", sum_(*swap(ok, 5, radius)))
    big = [65, a, 64, 32, i64s(*([0] * 2048 + [65])), dbl(*([1.0] * 64)), 1024, 0.1, 64, dbl(*([0.0] * 64)), a, a, a, a]
    refused(UNSUPPORTED, "ot_psf_field_sum: workspace and field", sum_(*big))
    many = [9 * 10 ** 6, a, 64, 1, i64s(*range(0, 9 * 10 ** 6 + 1, 140625)), dbl(*([1.0] * 64)), 8, 0.1, 1, dbl(0.0), a, a, a, a]
    assert _capi.psf_field_chunks(9 * 10 ** 6, 64, 1, 8, 1) == 64 * 1024 + 63 > _capi.PSFF_MAX_CHUNKS
    refused(UNSUPPORTED, "ot_psf_field_sum: more than 65535 chunks", sum_(*many))  # (the grid's second dimension)
    assert sum_(0, a, 2, 2, i64s(0, 0, 0, 0, 0), *ok[5:]) == 0

    comb = lambda *args: lib.ot_psf_field_combine(*args, st)
    ok = [2, 3, 2, 8, a, a, a, a, a, a, a]
    for i in range(4, 11):
        refused(INVALID, "ot_psf_field_combine: null argument", comb(*swap(ok, i, None)))
    for i, low, high, text in ((0, 0, 65, "n_fields"), (1, 0, 33, "n_bands"), (2, 0, 65, "n_planes"), (3, 0, 1025, "n_px")):
        refused(INVALID, f"ot_psf_field_combine: {text} below 1", comb(*swap(ok, i, low)))
        refused(UNSUPPORTED, f"ot_psf_field_combine: {text} above {high - 1}", comb(*swap(ok, i, high)))

    otf = lambda *args: lib.ot_psf_field_otf(*args, st)
    ok = [2, 2, 8, 0.1, a, a, dbl(0, 1, 0.6, 0.8), 3, dbl(0.0, 10.0, 40.0), a]
    for i in (4, 5, 6, 8, 9):
        refused(INVALID, "ot_psf_field_otf: null argument", otf(*swap(ok, i, None)))
    for i, low, high, text in ((0, 0, 65, "n_fields"), (1, 0, 65, "n_planes"), (2, 0, 1025, "n_px")):
        refused(INVALID, f"ot_psf_field_otf: {text} below 1", otf(*swap(ok, i, low)))
        refused(UNSUPPORTED, f"ot_psf_field_otf: {text} above {high - 1}", otf(*swap(ok, i, high)))
    refused(INVALID, "ot_psf_field_otf: n_freq below 1", otf(*swap(ok, 7, 0)))
    refused(UNSUPPORTED, "ot_psf_field_otf: n_freq above 64", otf(*swap(ok, 7, 65)))
    for size in (0.0, NAN, INF):
        refused(INVALID, "ot_psf_field_otf: size", otf(*swap(ok, 3, size)))
    refused(INVALID, "ot_psf_field_otf: direction", otf(*swap(ok, 6, dbl(0, 1, NAN, 0.8))))
    for freq in (dbl(0.0, -1.0, 2.0), dbl(0.0, NAN, 2.0), dbl(0.0, INF, 2.0)):
        refused(INVALID, "ot_psf_field_otf: frequency not finite or below zero", otf(*swap(ok, 8, freq)))
    refused(INVALID, "ot_psf_field_otf: frequency above the sampling limit", otf(*swap(ok, 8, dbl(0.0, 10.0, 40.001))))


def test_workspace():
    """The Python mirror is the library's bound; with one field it is that of `ot_psf_stack`; the table is four words per cell and two."""
    lib = _capi.load_library()
    for n, F, K, n_px, Z in ((1, 1, 1, 1, 1), (63, 2, 3, 2, 2), (257, 3, 2, 33, 1), (70001, 2, 1, 8, 1), (10 ** 6, 5, 3, 64, 21),
                             (10 ** 6, 5, 3, 128, 5), (5, 64, 32, 1024, 64), (0, 1, 1, 1, 1)):
        assert lib.ot_psf_field_workspace(n, F, K, n_px, Z) == _capi.psf_field_ws(n, F, K, n_px, Z) > 0, (n, F, K, n_px, Z)
        assert _capi.psf_field_ws(n, 1, K, n_px, Z) == _capi.psf_stack_ws(n, K, n_px, Z) == lib.ot_psf_stack_workspace(n, K, n_px, Z)
    for bad in ((-1, 1, 1, 8, 1), (10, 0, 1, 8, 1), (10, 65, 1, 8, 1), (10, 1, 0, 8, 1), (10, 1, 33, 8, 1), (10, 1, 1, 0, 1),
                (10, 1, 1, 1025, 1), (10, 1, 1, 8, 0), (10, 1, 1, 8, 65)):
        assert lib.ot_psf_field_workspace(*bad) == 0
    assert _capi.psf_field_table(6) == 26 and _capi.PSFF_MAX_FREQ == 64
    with pytest.raises(RuntimeError, match="fewer fields, planes, bands or image points"):
        pf.check_cap(65, 3, 1, 1024, 64)
    pf.check_cap(10 ** 6, 5, 3, 64, 21)
    with pytest.raises(RuntimeError, match="chunks of records"):
        pf.check_cap(9 * 10 ** 6, 64, 1, 8, 1)
    # the bound holds for every number of fields with records up to F: five fields of 140 records take two chunks each
    assert _capi.psf_field_chunks(700, 7, 1, 8, 1) == 5 * 2 + 6 and _capi.psf_field_chunks(700, 1, 1, 8, 1) == 6


# ---- the result object -----------------------------------------------------------------------------------------------------------------
def hand_made(F=3, K=2, Z=3, n_px=4, M=5, dead=1):
    """Arguments of `HuygensField` with field `dead` without a ray."""
    rng = np.random.default_rng(3)
    N = rng.integers(1, 100, (F, K))
    I = rng.uniform(0.1, 1, (F, Z, n_px, n_px))
    strehl = np.array([[0.3, 0.8, 0.8], [0.1, 0.2, 0.3], [0.9, 0.2, 0.9]])[:F, :Z]
    a = dict(sources=[4, 2, 7][:F], field=[[0, 0], [3.0, 4.0], [0, -2.0]][:F], section=2, reference_band=1, reference_field=0,
             band_edges=None, wavelengths=[486.0, 656.0][:K], dz=[-0.1, 0.0, 0.1][:Z], size=0.05, focus=rng.uniform(0, 1, (F, 3)),
             radius=np.full(F, -40.0), band_N=N, band_power=N / 100.0, n_missed=np.ones((F, K)), n_no_sphere=np.zeros((F, K)),
             band_weight=np.full((F, K), 1.0 / K), cutoff=np.full((F, K), 100.0), intensity=I, band_strehl=rng.uniform(0, 1, (F, Z, K)),
             strehl=strehl, noise_floor=np.full(F, 1e-3), frequencies=np.linspace(0, 40, M),
             otf_t=rng.uniform(0, 1, (F, Z, M)) + 1j, otf_s=rng.uniform(0, 1, (F, Z, M)), mtf_t=rng.uniform(0, 1, (F, Z, M)),
             mtf_s=rng.uniform(0, 1, (F, Z, M)))
    if dead is not None:
        a["band_N"][dead] = 0
        a["band_power"][dead] = 0
        for key in ("band_weight", "cutoff", "intensity", "band_strehl", "strehl", "noise_floor", "otf_t", "otf_s", "mtf_t", "mtf_s",
                    "focus", "radius"):
            a[key] = np.array(a[key], dtype=np.complex128 if key.startswith("otf") else np.float64)
            a[key][dead] = NAN
    return a


def test_result_object():
    a = hand_made()
    hf = ot.HuygensField(**a, long_desc="by hand")
    assert isinstance(hf, pf.HuygensField) and hf._tracked is False
    with pytest.raises(RuntimeError, match="read-only"):
        hf.size = 1.0  # locked
    assert (hf.n_fields, hf.n_bands, hf.n_px) == (3, 2, 4) and hf.sources.tolist() == [4, 2, 7]
    assert hf.field.shape == (3, 2) and hf.t.tolist() == [[0, 1], [0.6, 0.8], [0, -1]] and hf.focus.shape == (3, 3) and hf.radius.shape == (3,)
    assert hf.band_N.dtype == np.int64 and hf.n_missed.dtype == np.int64 and hf.n_no_sphere.shape == (3, 2)
    for arr, shape in ((hf.band_power, (3, 2)), (hf.band_weight, (3, 2)), (hf.cutoff, (3, 2)), (hf.intensity, (3, 3, 4, 4)),
                       (hf.band_strehl, (3, 3, 2)), (hf.strehl, (3, 3)), (hf.peak, (3, 3)), (hf.noise_floor, (3,)), (hf.best_focus, (3,)),
                       (hf.frequencies, (5,)), (hf.otf_t, (3, 3, 5)), (hf.otf_s, (3, 3, 5)), (hf.mtf_t, (3, 3, 5)), (hf.mtf_s, (3, 3, 5)),
                       (hf.wavelengths, (2,)), (hf.dz, (3,))):
        assert arr.shape == shape
    assert hf.otf_t.dtype == np.complex128 and hf.otf_t[0, 0, 0].imag == 1
    # best focus: the first maximum; peak: the largest value of a plane; the field without a ray: NaN
    assert hf.best_focus[0] == 0.0 and hf.best_focus[2] == -0.1 and np.isnan(hf.best_focus[1])
    holes = hand_made()
    holes["strehl"][0] = [NAN, 0.4, 0.4]  # (a plane without a value is passed over)
    assert ot.HuygensField(**holes).best_focus[0] == 0.0
    assert np.array_equal(hf.peak[[0, 2]], a["intensity"][[0, 2]].max(axis=(2, 3))) and np.all(np.isnan(hf.peak[1]))

    p = hf.psf(2, 1)
    assert isinstance(p, ot.HuygensPSF) and p.N == a["band_N"][2].sum() and p.power == pytest.approx(a["band_power"][2].sum())
    assert p.n_missed == 2 and p.section == 2 and np.array_equal(p.focus, hf.focus[2]) and p.radius == -40 and p.size == 0.05 and p.dz == 0.0
    assert np.array_equal(p.intensity, hf.intensity[2, 1]) and p.strehl == hf.strehl[2, 1] and p.noise_floor == 1e-3 and p.peak == hf.peak[2, 1]
    assert p.wavelength == pytest.approx((a["band_power"][2] * [486, 656]).sum() / a["band_power"][2].sum()) and p.long_desc == "by hand"
    assert hf.psf(0).dz == -0.1
    img = hf.to_image(2, 1)
    assert isinstance(img, ot.GrayscaleImage) and img.shape[:2] == (4, 4) and list(img.s) == [0.05, 0.05]
    pc.check_empty(hf.psf(1, 2), 4)
    with pytest.raises(RuntimeError, match="No usable ray"):
        hf.to_image(1)
    for bad in ((3, 0), (-1, 0), (0, 3), (0, -1)):
        with pytest.raises(ValueError):
            hf.psf(*bad)
    with pytest.raises(TypeError):
        hf.psf(0.0)

    g = hf.grid()
    assert len(g) == 1 and len(g[0]) == 3 and all(isinstance(q, ot.HuygensPSF) for q in g[0])
    assert [q.N for q in g[0]] == a["band_N"].sum(axis=1).tolist() and np.array_equal(g[0][2].intensity, hf.intensity[2, 0])
    assert np.array_equal(hf.grid(plane=2)[0][0].intensity, hf.intensity[0, 2])
    g = hf.grid(1, shape=(3, 1))
    assert len(g) == 3 and all(len(row) == 1 for row in g) and np.array_equal(g[2][0].intensity, hf.intensity[2, 1])
    six = ot.HuygensField(**hand_made(F=3, dead=None) | dict(sources=[0, 1, 2]))
    assert np.array_equal(six.grid(shape=[1, 3])[0][1].intensity, six.intensity[1, 0])
    for shape in ((2, 2), (3,), (1, 3, 1), (0, 3), (1.5, 2), (4, 1)):
        with pytest.raises(ValueError):
            hf.grid(shape=shape)
    with pytest.raises(TypeError):
        hf.grid(shape=3)
    with pytest.raises(ValueError):
        hf.grid(plane=3)

    # what does not fit is refused
    for key, val in (("sources", []), ("sources", list(range(65))), ("band_edges", [400, 500]), ("reference_band", 2), ("reference_field", 3),
                     ("intensity", np.zeros((3, 3, 4, 5))), ("intensity", np.zeros((3, 2, 4, 4))), ("band_N", np.zeros((3, 33)))):
        with pytest.raises(ValueError):
            ot.HuygensField(**{**a, key: val})


def test_empty_result():
    """The rule of `psf._empty_stack`: what the caller fixed stays; edges keep their bands, else one band without a ray."""
    dz = np.array([0.0, 0.1])
    e = pf._empty(3, np.array([400.0, 500, 600]), 6, 0.1, dz, None, None, np.array([0.0, 5.0]), 1, [3, 1], [[0, 0], [0, 1]])
    assert e.n_bands == 2 and e.n_fields == 2 and e.reference_band == -1 and e.reference_field == 1 and e.section == 3 and e.size == 0.1
    assert e.band_N.tolist() == [[0, 0], [0, 0]] and e.band_power.tolist() == [[0, 0], [0, 0]] and e.n_missed.sum() == 0 and e.n_no_sphere.sum() == 0
    assert e.sources.tolist() == [3, 1] and e.band_edges.tolist() == [400, 500, 600] and e.frequencies.tolist() == [0, 5] and e.dz.tolist() == [0, 0.1]
    assert e.intensity.shape == (2, 2, 6, 6) and e.otf_t.shape == (2, 2, 2) and e.mtf_s.shape == (2, 2, 2)
    for arr in (e.intensity, e.strehl, e.band_strehl, e.band_weight, e.cutoff, e.noise_floor, e.peak, e.best_focus, e.focus, e.radius,
                e.wavelengths, e.otf_t, e.otf_s, e.mtf_t, e.mtf_s):
        assert np.all(np.isnan(arr))
    pc.check_empty(e.psf(1, 1), 6)
    assert np.all(np.isnan(e.diffraction_limit([0.0, 1.0], 0, 1)))
    e = pf._empty(0, "lines", 4, None, np.zeros(1), np.array([[1.0, 2, 3]]), np.array([-5.0]), None, 0, [0], [[0, 0]],
                  n_missed=np.array([[7]]), n_no_sphere=np.array([[2]]))
    assert e.n_bands == 1 and e.band_edges is None and np.isnan(e.size) and e.frequencies.shape == (17,) and np.all(np.isnan(e.frequencies))
    assert e.focus.tolist() == [[1, 2, 3]] and e.radius.tolist() == [-5] and e.n_missed.tolist() == [[7]] and e.n_no_sphere.tolist() == [[2]]
    e = pf._empty(0, 4, 8, 0.2, np.zeros(1), None, None, None, 0, [0], [[0, 0]])
    assert e.n_bands == 1 and np.array_equal(e.frequencies, np.linspace(0, 20, 17))


# ---- the transfer function -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def perfect():
    """The perfect-wave intensity of `psf_cases.perfect_wave` by `psf_cases.truth`: NA 0.1 at 550 nm, 16 x 16 points over 0.06 mm."""
    n_px, size = 16, 0.06
    rec = pc.perfect_wave(12, 0.1, 550.0, -50.0)
    re, im, _, A, A2, _ = pc.truth(rec, -50.0, n_px, size, 0.0)
    inten = np.asarray((re * re + im * im) / (A * A), dtype=np.float64)[:-1].reshape(n_px, n_px)
    return inten, float(A2 / (A * A)), n_px, size


def otf_bound(J, n_px, size, nu):
    """(n_px^2 + 6 pi nu size + 16) eps sum |J|: the additions and the sine-cosine kernels, and three roundings of a phase of at
    most nu size turns."""
    return (n_px * n_px + 6 * np.pi * np.asarray(nu) * size + 16) * EPS * np.abs(J).sum()


def test_restated_transfer_function_is_diffraction_mtf_along_the_axes(perfect):
    """With t = (0, 1): t . x = y and s . x = -x.  `diffraction_mtf` sums the rows first (its line spread) and takes the phase from
    the pixel's coordinate alone, the restatement adds pixel by pixel in the device's order: both lie within the bound of the exact
    transform, so their moduli differ by twice the bound over |OTF(0)|, and by as much again for the quotient."""
    inten, floor, n_px, size = perfect
    m = hp.diffraction_mtf(inten, floor, size, n_f=17)
    otf_t, otf_s, mtf_t, mtf_s = pf.transfer(inten, floor, size, (0.0, 1.0), m.f)
    J = inten - floor
    tol = 4 * otf_bound(J, n_px, size, m.f) / abs(J.sum())
    print("largest difference", np.abs(mtf_t - m.mtf_y).max(), np.abs(mtf_s - m.mtf_x).max(), "allowed", tol.min())
    assert np.all(np.abs(mtf_t - m.mtf_y) <= tol) and np.all(np.abs(mtf_s - m.mtf_x) <= tol)
    assert mtf_t[0] == 1 and mtf_s[0] == 1 and otf_t[0].imag == 0 and otf_t[0].real == otf_s[0].real
    # a quarter turn of t swaps the two, up to the sign of the odd part
    o_t, o_s, m_t, m_s = pf.transfer(inten, floor, size, (1.0, 0.0), m.f)
    assert np.all(np.abs(m_t - m.mtf_x) <= tol) and np.all(np.abs(m_s - m.mtf_y) <= tol)
    # the restatement against the exact transform in longdouble, for an oblique direction too
    for t in ((0.0, 1.0), (0.6, 0.8)):
        got = pf.transfer(inten, floor, size, t, m.f)
        want = exact_transfer(inten, floor, size, t, m.f)
        for k in (0, 1):
            err = np.maximum(np.abs(got[k].real - want[k].real), np.abs(got[k].imag - want[k].imag))
            assert np.all(err <= otf_bound(J, n_px, size, m.f)), (t, k, err)


def exact_transfer(inten, floor, size, t, nu):
    """sum_p J_p exp(-2 pi i nu (d . x_p)) along d = t and d = s in longdouble, from the float64 J, pixel centres as the definition
    has them.  -> (otf_t, otf_s) as pairs of longdouble arrays in a structured result with .real and .imag"""
    n_px = inten.shape[0]
    a = (np.arange(n_px, dtype=LD) + LD(0.5) - LD(n_px) / 2) * LD(size) / LD(n_px)
    x, y = np.meshgrid(a, a)
    J = (np.asarray(inten, dtype=np.float64) - floor).astype(LD)
    tx, ty = LD(t[0]), LD(t[1])
    out = []
    for u in (tx * x + ty * y, tx * y - ty * x):
        ph = 2 * pc.PI * np.asarray(nu, dtype=LD)[:, None, None] * u[None]
        out.append(type("Z", (), dict(real=(J * np.cos(ph)).sum(axis=(1, 2)), imag=-(J * np.sin(ph)).sum(axis=(1, 2)))))
    return out


def test_diffraction_limit():
    a = hand_made(dead=1)
    a["cutoff"][0] = [100.0, 250.0]
    hf = ot.HuygensField(**a)
    nu = np.array([0.0, 25.0, 50.0, 99.999, 100.0, 100.001, 1e6])
    got = hf.diffraction_limit(nu, 0, 0)
    x = nu[:4] / 100.0
    assert got[0] == 1.0 and np.all(got[4:] == 0.0) and got.shape == (7,)
    assert np.allclose(got[:4], 2 / np.pi * (np.arccos(x) - x * np.sqrt(1 - x * x)), rtol=0, atol=4 * EPS)
    assert np.all(np.diff(got[:5]) < 0) and hf.diffraction_limit(125.0, 0, 1) == pytest.approx(2 / np.pi * (np.pi / 3 - 0.5 * np.sqrt(0.75)), abs=4 * EPS)
    assert np.all(np.isnan(hf.diffraction_limit(nu, 1, 0)))  # the field without a ray
    for bad in ((3, 0), (0, 2), (-1, 0)):
        with pytest.raises(ValueError):
            hf.diffraction_limit(nu, *bad)


def test_constants_match_the_header():
    import pathlib
    import re
    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "optrace_amd.h").read_text()
    assert int(re.search(r"#define OT_PSFF_MAX_FREQ (\d+)", text).group(1)) == _capi.PSFF_MAX_FREQ
    assert re.search(r"#define OT_PSF_FIELD_TABLE\(cells\) \(4 \* \(int64_t\)\(cells\) \+ 2\)", text)
    assert re.search(r"#define OT_ABI_VERSION 9\b", text)
