"""Ray fans without a device: the argument checks of `Raytracer.ray_fans` and of the `ot_fans_*` entry points, which come before any
device call, `ot.RayFans` built from hand-made records and bins, the longdouble definition (tests/fans_cases.py) on a ten-ray
example worked by hand, and the header's constants."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd import fans

import fans_cases as fc

NAN = np.nan
F64 = lambda a: np.asarray(a).astype(np.float64)


# ---- the arguments -------------------------------------------------------------------------------------------------------------------
def tracer():
    RT = ot.Raytracer(outline=[-1, 1, -1, 1, -1, 10])
    RT.add(ot.RaySource(ot.Point(), pos=[0, 0, 0]))
    return RT


@pytest.mark.parametrize("kwargs,error", [
    (dict(source_index=1.0), TypeError), (dict(source_index="0"), TypeError),
    (dict(section=1.0), TypeError), (dict(section=-1), ValueError), (dict(section=1), ValueError),
    (dict(bands="bands"), ValueError), (dict(bands=2.0), TypeError), (dict(bands=None), TypeError), (dict(bands=0), ValueError),
    (dict(bands=33), ValueError), (dict(bands=[500.0]), ValueError), (dict(bands=[500, 400]), ValueError),
    (dict(bands=[400, NAN]), ValueError), (dict(bands=[[400, 500]]), ValueError),
    (dict(focus=1.0), TypeError), (dict(focus=[0, 0]), ValueError), (dict(focus=[0, 0, NAN]), ValueError),
    (dict(focus=["a", "b", "c"]), TypeError), (dict(radius="1"), TypeError), (dict(radius=0.0), ValueError),
    (dict(radius=np.inf), ValueError),
    (dict(n_bins=32.0), TypeError), (dict(n_bins=None), TypeError), (dict(n_bins=0), ValueError), (dict(n_bins=257), ValueError),
    (dict(slab="0.1"), TypeError), (dict(slab=None), TypeError), (dict(slab=0.0), ValueError), (dict(slab=-0.1), ValueError),
    (dict(slab=np.nextafter(1.0, 2.0)), ValueError), (dict(slab=NAN), ValueError), (dict(slab=np.inf), ValueError),
    (dict(pupil_radius="1"), TypeError), (dict(pupil_radius=0.0), ValueError), (dict(pupil_radius=-1.0), ValueError),
    (dict(pupil_radius=NAN), ValueError),
])
def test_argument_errors_come_before_the_device(kwargs, error, monkeypatch):
    from optrace_amd import raytracer
    monkeypatch.setattr(raytracer, "require_device", lambda: pytest.fail("the device was asked for before the arguments were checked"))
    with pytest.raises(error):
        tracer().ray_fans(**kwargs)


def test_check_arguments_returns_what_the_analysis_takes():
    bands, focus, radius, slab, pr = fans.check_arguments(3, 1, [400, 500, 600], (0, 1, 2), 5, 256, 1, np.float32(0.5))
    assert bands.dtype == np.float64 and bands.tolist() == [400, 500, 600] and focus.dtype == np.float64 and focus.tolist() == [0, 1, 2]
    assert (radius, slab, pr) == (5.0, 1.0, 0.5) and all(isinstance(v, float) for v in (radius, slab, pr))
    assert fans.check_arguments(2, None, "lines", None, None, 1, 0.1, None) == ("lines", None, None, 0.1, None)
    assert fans.check_arguments(2, 0, 32, None, -3.0, 32, 1e-300, None)[:3:2] == (32, -3.0)
    with pytest.raises(ValueError, match="256"):
        fans.check_arguments(2, None, "lines", None, None, 257, 0.1, None)
    with pytest.raises(ValueError, match="slab"):
        fans.check_arguments(2, None, "lines", None, None, 32, 1.5, None)


def test_good_arguments_reach_the_device_and_then_the_rays(monkeypatch):
    from optrace_amd import raytracer
    asked = []
    monkeypatch.setattr(raytracer, "require_device", lambda: asked.append(1))
    for kwargs in (dict(), dict(source_index=None, section=0, bands=4, focus=[0, 0, 5], radius=-2, n_bins=256, slab=1.0, pupil_radius=0.5),
                   dict(bands=[400, 500.5, 700], n_bins=1)):
        with pytest.raises(RuntimeError, match="No rays traced"):
            tracer().ray_fans(**kwargs)
    assert len(asked) == 3


# ---- ten rays by hand -------------------------------------------------------------------------------------------------------------------
# Two sections of which section 0 is analysed; every ray starts in the plane z = 0 and ends in the plane z = 10 of the focus
# (0, 0, 10), so t = 1 and (ex, ey) are the xy of its end; ray 9 ends in z = 0 and runs parallel to that plane.  The pupil has its
# centre in (0, 0) and the radius 1: (u, v) are the unit-disc coordinates.  slab 0.1, four bins: [-1, -.5) [-.5, 0) [0, .5) [.5, 1].
#           u       v       w    opl    ex     ey     key                         tangential (|u| <= .1)    sagittal (|v| <= .1)
RAYS = [(0.0,    -1.0,    1.0, 50.0,  0.0,  -0.5,    0),                        # bin 0                   -
        (0.0,    -0.5,    1.0, 50.25, 0.0,  -0.125,  0),                        # bin 1                   -
        (0.0,     0.0,    2.0, 50.5,  0.75,  0.0,    0),                        # bin 2                   bin 2
        (0.0,     0.5,    1.0, 50.25, 0.0,   0.125,  0),                        # bin 3                   -
        (0.0,     1.0,    1.0, 50.0,  0.0,   0.5,    0),                        # bin 3 (the last edge)   -
        (-0.75,   0.0,    0.5, 51.0, -0.5,   0.0,    1),                        # -                       bin 0
        (0.75,    0.0625, 0.5, 51.0,  0.5,   0.25,   1),                        # -                       bin 3
        (0.5,     0.5,    1.0, 52.0,  1.0,   1.0,    1),                        # in neither cut
        (0.0625,  0.25,   1.0, 49.0,  2.0,  -1.0,    255),                      # in no band
        (0.0,     0.25,   1.0, 48.0,  3.0,   3.0,    0)]                        # parallel: no weight after the transverse step
REC = np.array([[6, 5, 301.5, 1.5, 0, 3000, 50, 50.5, 0.25, 0.75, 0.53125, 0, 0.3125],
                [2, 3, 103, 1, 1.125, 1200, 51, 52, 0.5, 0.75, 0.3984375, 0.5, 1.31640625]])
BINS = np.zeros((2, 2, 4, 6))
BINS[0, 0] = [[1, 1, -1, 0, -0.5, -0.25], [1, 1, -0.5, 0, -0.125, 0], [2, 1, 0, 1.5, 0, 0.5], [2, 2, 1.5, 0, 0.625, -0.25]]
BINS[0, 1, 2] = [2, 1, 0, 1.5, 0, 0.5]
BINS[1, 1, 0] = [0.5, 1, -0.375, -0.25, 0, -0.25]
BINS[1, 1, 3] = [0.5, 1, 0.375, 0.25, 0.125, -0.25]
MOM = np.array([9.5, 10, 0, 0, 0, 0, 0, 0, 0, 1, 1.0])  # (the slots the fans read: 0, 3, 4 and 10)


def ten_rays():
    r = np.array(RAYS)
    u, v, w, opl, ex, ey = r[:, :6].T
    p = np.zeros((10, 2, 3))
    p[:, 0, :2] = [0.25, -0.5]
    p[:, 1] = np.stack([ex, ey, np.full(10, 10.0)], axis=1)
    p[9, 1, 2] = 0.0
    wl = np.where(r[:, 6] == 0, 500.0, 600.0).astype(np.float32)
    return p, u, v, w.astype(np.float32), opl, wl, r[:, 6].astype(np.uint8)


def test_the_truth_on_ten_rays_worked_by_hand():
    p, u, v, w, opl, wl, key = ten_rays()
    t = fc.transverse(p, w, 0, 10, 0, (0.0, 0.0, 10.0))
    assert t["n_parallel"] == 1 and t["w"].tolist() == [1, 1, 2, 1, 1, 0.5, 0.5, 1, 1, 0]
    want = np.array(RAYS)[:, 4:6]
    assert np.array_equal(F64(t["ex"])[:9], want[:9, 0]) and np.array_equal(F64(t["ey"])[:9], want[:9, 1])
    assert np.isnan(F64(t["ex"])[9]) and np.isnan(F64(t["ey"])[9]) and np.all(F64(t["b_ex"])[:9] >= 0)
    # a focus off the axis and a plane the rays reach half way: ex = p_x + (p1_x - p_x) / 2 - f_x
    h = fc.transverse(p, w, 0, 10, 0, (1.0, 2.0, 5.0))
    assert np.array_equal(F64(h["ex"])[:9], 0.25 + (want[:9, 0] - 0.25) / 2 - 1) and np.array_equal(F64(h["ey"])[:9], -0.5 + (want[:9, 1] + 0.5) / 2 - 2)
    # a ray range and dead rays with NaN positions
    q = p.copy()
    q[:3] = NAN
    part = fc.transverse(q, np.where(np.arange(10) < 3, 0, w)[2:], 2, 8, 0, (0.0, 0.0, 10.0))
    assert np.isnan(F64(part["ex"])[0]) and np.array_equal(F64(part["ex"])[1:7], want[3:9, 0]) and part["n_parallel"] == 1

    val, mag = fc.band_records(opl, F64(t["ex"]), F64(t["ey"]), t["w"], wl, key, 2)
    assert np.array_equal(F64(val), REC), F64(val) - REC
    assert np.all(mag[:, fc.SUMS1 + fc.SUMS2] >= np.abs(val[:, fc.SUMS1 + fc.SUMS2]))
    assert fc.record_means(REC).tolist() == [[50.25, 0.25, 0], [51.5, 0.5, 0.5625]]
    # means handed in are taken as they are; a band without a ray
    val3, _ = fc.band_records(opl, F64(t["ex"]), F64(t["ey"]), t["w"], wl, key, 3, means=[[50, 0, 0], [51.5, 0.5, 0.5625], [0, 0, 0]])
    assert F64(val3)[0, 8:].tolist() == [0.625, 1.125, 0.53125, 0, 0.5625] and np.array_equal(F64(val3)[1], REC[1])
    assert F64(val3)[2, :9].tolist() == [0] * 9 and np.all(np.isnan(F64(val3)[2, 9:12])) and val3[2, 12] == 0

    sel, x, y = fc.unit_disc(u, v, t["w"], MOM, None)
    assert sel.tolist() == [True] * 9 + [False] and np.array_equal(x[:9], u[:9]) and np.array_equal(y[:9], v[:9])
    assert fc.bin_index([-1, -0.5, -2.0 ** -52, 0, 0.5, 1, np.nextafter(1, 2), np.nextafter(-1, -2)], 4).tolist() == [0, 1, 1, 2, 3, 3, 3, 0]
    bins, bmag, passed = fc.fan_bins(u, v, opl, F64(t["ex"]), F64(t["ey"]), t["w"], key, 2, MOM, None, REC, 4, 0.1)
    assert np.array_equal(F64(bins), BINS), F64(bins) - BINS
    assert passed.tolist() == [5, 3] and np.all(bmag >= np.abs(bins))
    # a pupil radius of 0.75 given: the unit disc shrinks, rays 0 and 4 (|y| = 4 / 3) and ray 6 (x = 1, y > 0) fall out, ray 5 moves to x = -1
    sel, x, y = fc.unit_disc(u, v, t["w"], MOM, 0.75)
    assert sel.tolist() == [False, True, True, True, False, True, False, True, True, False] and x[5] == -1
    # and a pupil whose centre the record gives: the coordinates are taken about it
    mom = MOM.copy()
    mom[3], mom[4] = 9.5 * 0.5, 9.5 * -0.25
    _, x, y = fc.unit_disc(u, v, t["w"], mom, None)
    assert x[2] == -0.5 and y[2] == 0.25


def test_ray_fans_from_the_hand_made_records():
    edges = [400, 550, 700]
    a = ot.RayFans(REC, BINS, 0, [0, 0, 10], 10.0, (0, 0), 1.0, 0.1, n_missed=2, n_parallel=1, n_out_of_band=1, band_edges=edges,
                   long_desc="by hand")
    assert (a.n_bands, a.n_bins, a.section, a.radius, a.pupil_radius, a.slab) == (2, 4, 0, 10.0, 1.0, 0.1) and a.long_desc == "by hand"
    assert (a.N, a.power, a.n_missed, a.n_parallel, a.n_out_of_band) == (8, 8.0, 2, 1, 1)
    assert a.band_N.tolist() == [5, 3] and a.band_N.dtype == np.int64 and a.band_power.tolist() == [6, 2] and a.band_edges.tolist() == edges
    assert a.focus.tolist() == [0, 0, 10] and a.pupil_centre.tolist() == [0, 0]
    assert a.wavelengths.tolist() == [500, 600] and a.opl_mean.tolist() == [50.25, 51.5]
    assert a.opd_min.tolist() == [-0.25, -0.5] and a.opd_max.tolist() == [0.25, 0.5] and a.opd_pv.tolist() == [0.5, 1]
    assert np.array_equal(a.opd_rms, np.sqrt([0.25 / 6, 0.25])) and np.array_equal(a.opd_rms_waves, a.opd_rms / (np.array([500, 600]) * 1e-6))
    assert a.centroid.tolist() == [[0.25, 0], [0.5, 0.5625]]
    assert np.array_equal(a.rms_x, np.sqrt([0.125, 0.375])) and np.array_equal(a.rms_y, np.sqrt([0.53125 / 6, 0.3984375 / 2]))
    assert np.array_equal(a.rms_radius, np.sqrt(a.rms_x ** 2 + a.rms_y ** 2)) and np.array_equal(a.max_radius, np.sqrt([0.3125, 1.31640625]))
    # the fans: means per bin, NaN where no ray fell
    assert a.count.dtype == np.int64 and a.count[0].tolist() == [[1, 1, 1, 2], [0, 0, 1, 0]] and a.count[1].tolist() == [[0] * 4, [1, 0, 0, 1]]
    assert np.array_equal(a.weight, BINS[..., 0]) and a.weight.shape == a.pupil.shape == a.ex.shape == a.ey.shape == a.opd.shape == (2, 2, 4)
    y, ey, opd = a.tangential(0)
    assert y.tolist() == [-1, -0.5, 0, 0.75] and ey.tolist() == [-0.5, -0.125, 0, 0.3125] and opd.tolist() == [-0.25, 0, 0.25, -0.125]
    x, ex, opd = a.sagittal(1)
    assert np.array_equal(x, [-0.75, NAN, NAN, 0.75], equal_nan=True) and np.array_equal(ex, [-0.5, NAN, NAN, 0.5], equal_nan=True)
    assert np.array_equal(opd, [-0.5, NAN, NAN, -0.5], equal_nan=True) and a.ey[1, 1, 3] == 0.25
    assert np.all(np.isnan(a.tangential(1)[0])) and a.sagittal()[1][2] == 0.75
    for name in ("pupil", "ex", "ey", "opd"):
        assert np.array_equal(np.isnan(getattr(a, name)), a.count == 0), name
    # ... and they are the truth's figures
    f = fc.figures(REC, BINS)
    for name, want in f.items():
        assert np.allclose(getattr(a, name), F64(want), rtol=1e-15, atol=0, equal_nan=True), name
    assert np.array_equal(a.records, REC) and np.array_equal(a.bins, BINS)


def test_result_object_is_locked_and_checks_its_shapes():
    rec = REC.copy()
    rec[1] = 0
    rec[1, 9:12] = NAN
    one = REC[:1].copy()
    one[0, :2] = [0.5, 1]
    a = ot.RayFans(rec, BINS, 2, [0, 0, 1], -3.0, (0.5, 0.5), 2.0, 0.25)
    assert a.band_N.tolist() == [5, 0] and a.band_edges is None and a.radius == -3.0
    for name in ("wavelengths", "opl_mean", "opd_rms", "opd_min", "opd_max", "opd_pv", "opd_rms_waves", "rms_x", "rms_y", "rms_radius",
                 "max_radius"):
        assert np.isnan(getattr(a, name)[1]) and np.isfinite(getattr(a, name)[0]), name
    assert np.all(np.isnan(a.centroid[1]))
    s = ot.RayFans(one, BINS[:1], 0, [0, 0, 1], 1.0, (0, 0), 1.0, 0.1)
    assert s.opd_rms[0] == 0 and s.rms_x[0] == 0 and s.rms_y[0] == 0 and s.rms_radius[0] == 0, "a band of one ray"
    with pytest.raises(RuntimeError):
        a.power = 1.0
    with pytest.raises(ValueError):
        a.ex[0, 0, 0] = 1
    with pytest.raises(AttributeError):
        a.something_else = 1
    args = dict(records=rec, bins=BINS, section=2, focus=[0, 0, 1], radius=1.0, pupil_centre=(0, 0), pupil_radius=1.0, slab=0.1)
    for bad in (dict(records=rec[:, :12]), dict(records=rec.ravel()), dict(records=np.zeros((33, 13)), bins=np.zeros((33, 2, 4, 6))),
                dict(records=np.zeros((0, 13)), bins=np.zeros((0, 2, 4, 6))), dict(bins=BINS[:1]), dict(bins=BINS[:, :1]),
                dict(bins=BINS[..., :5]), dict(bins=BINS.reshape(2, 2, 24)), dict(bins=np.zeros((2, 2, 257, 6))),
                dict(bins=np.zeros((2, 2, 0, 6))), dict(band_edges=[400, 500]), dict(focus=[0, 0]), dict(pupil_centre=(0, 0, 0))):
        with pytest.raises(ValueError):
            ot.RayFans(**{**args, **bad})
    # the empty result: what the caller fixed stays, every figure NaN, no ray in any bin
    e = fans._empty(3, np.array([400.0, 500, 600]), None, None, 8, 0.2, None, 4, 5, 6)
    assert e.N == 0 and e.power == 0 and e.n_bands == 2 and e.n_bins == 8 and e.band_N.tolist() == [0, 0] and e.slab == 0.2
    assert (e.n_missed, e.n_parallel, e.n_out_of_band) == (4, 5, 6) and e.band_edges.tolist() == [400, 500, 600] and e.section == 3
    for f in (e.focus, e.radius, e.pupil_centre, e.pupil_radius, e.wavelengths, e.opl_mean, e.opd_rms, e.opd_pv, e.opd_rms_waves,
              e.centroid, e.rms_radius, e.max_radius, e.pupil, e.ex, e.ey, e.opd):
        assert np.all(np.isnan(f))
    assert np.all(e.count == 0) and np.all(e.weight == 0) and e.count.shape == (2, 2, 8)
    e = fans._empty(0, "lines", np.array([0.0, 0, 5]), 2.5, 1, 0.1, 0.5)
    assert e.n_bands == 1 and e.band_edges is None and e.focus.tolist() == [0, 0, 5] and e.radius == 2.5 and e.pupil_radius == 0.5
    assert fans._empty(0, 7, None, None, 1, 0.1, None).n_bands == 1


# ---- the entry points ------------------------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_before_anything_else():
    lib = _capi.load_library()
    st = C.c_void_p()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)  # (never dereferenced: every call below returns from its checks)
    d3 = lambda *v: (C.c_double * 3)(*v)
    INVALID, UNSUPPORTED = -1, -3

    def rays(N=100, nt=3, p=a, w=a):
        r = _capi.Rays()
        r.N, r.nt, r.p, r.w = N, nt, p, w
        return C.byref(r)

    def refused(code, text, status):
        assert status == code and text.encode() in lib.ot_last_error(), (status, lib.ot_last_error())

    without = lambda ok, i: [None if j == i else x for j, x in enumerate(ok)]
    tr = lambda *args: lib.ot_fans_transverse(*args, st)
    ok = [rays(), 0, 10, 1, d3(0, 0, 0), a, a, a, a]
    for i in (0, 4, 5, 6, 7, 8):
        refused(INVALID, "ot_fans_transverse: null argument", tr(*without(ok, i)))
    for R in (rays(p=None), rays(w=None)):
        refused(INVALID, "ot_fans_transverse: null argument", tr(R, *ok[1:]))
    for first, count in ((-1, 5), (0, -1), (0, 101), (91, 10), (101, 0)):
        refused(INVALID, "ot_fans_transverse: ray range", tr(ok[0], first, count, *ok[3:]))
    for k in (-1, 2, 100):
        refused(INVALID, "ot_fans_transverse: section", tr(*ok[:3], k, *ok[4:]))
    for f in (d3(NAN, 0, 0), d3(0, np.inf, 0), d3(0, 0, -np.inf)):
        refused(INVALID, "ot_fans_transverse: focus not finite", tr(*ok[:4], f, *ok[5:]))
    assert tr(ok[0], 0, 0, *ok[3:]) == 0 and tr(ok[0], 100, 0, *ok[3:]) == 0

    bands = lambda *args: lib.ot_fans_bands(*args, st)
    ok = [10, a, a, a, a, a, a, 3, a, a]
    for i in (1, 2, 3, 4, 5, 6, 8, 9):
        refused(INVALID, "ot_fans_bands: null argument", bands(*without(ok, i)))
    refused(INVALID, "ot_fans_bands", bands(-1, *ok[1:]))
    for K in (0, -1, 33):
        refused(UNSUPPORTED, "ot_fans_bands: n_bands outside 1 .. 32", bands(*ok[:7], K, *ok[8:]))
    refused(UNSUPPORTED, "ot_fans_bands", bands(0, *ok[1:7], 33, *ok[8:]))  # (the limits hold whatever the count is)
    assert bands(0, *ok[1:]) == 0 and bands(0, *ok[1:7], 32, *ok[8:]) == 0

    bins = lambda *args: lib.ot_fans_bins(*args, st)
    ok = [10, a, a, a, a, a, a, a, a, NAN, a, 3, 32, 0.1, a]
    for i in (1, 2, 3, 4, 5, 6, 7, 8, 10, 14):
        refused(INVALID, "ot_fans_bins: null argument", bins(*without(ok, i)))
    refused(INVALID, "ot_fans_bins", bins(-1, *ok[1:]))
    for K in (0, -1, 33):
        refused(UNSUPPORTED, "ot_fans_bins: n_bands outside 1 .. 32", bins(*ok[:11], K, *ok[12:]))
    for nb in (0, -1, 257):
        refused(UNSUPPORTED, "ot_fans_bins: n_bins outside 1 .. 256", bins(*ok[:12], nb, *ok[13:]))
    for slab in (0.0, -0.1, float(np.nextafter(1.0, 2.0)), NAN, np.inf):
        refused(INVALID, "ot_fans_bins: slab", bins(*ok[:13], slab, a))
    for pr in (0.0, -1.0, np.inf):
        refused(INVALID, "ot_fans_bins: pupil radius", bins(*ok[:9], pr, *ok[10:]))
    assert bins(0, *ok[1:]) == 0 and bins(0, *ok[1:9], 2.0, a, 32, 256, 1.0, a) == 0


def test_workspace():
    """Doubles for the partial sums: 8 per workgroup of 256 rays and band, at most 1024 workgroups per band and piece of 2^28 rays;
    0 for arguments out of range."""
    ws = _capi.load_library().ot_fans_workspace
    assert ws(1, 1) == 8 and ws(256, 3) == 8 * 3 and ws(257, 3) == 8 * 3 * 2
    assert ws(256 * 1024, 5) == ws(10 ** 8, 5) == 8 * 5 * 1024 and ws(2 ** 28 + 1, 32) == 8 * 32 * 1025
    assert ws(0, 3) == 0
    for count, K in ((-1, 3), (10, 0), (10, -1), (10, 33)):
        assert ws(count, K) == 0


def test_constants_match_the_header():
    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "optrace_amd.h").read_text()
    value = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert value("OT_FAN_M") == _capi.FAN_M == fc.M == 13
    assert value("OT_FAN_BIN_M") == _capi.FAN_BIN_M == fc.BIN_M == 6
    assert value("OT_FAN_MAX_BINS") == _capi.FAN_MAX_BINS == fc.MAX_BINS == 256
    assert value("OT_CHROM_MAX_BANDS") == fc.MAX_BANDS == 32 and _capi.CHROM_NO_BAND == fc.NO_BAND == 255
    assert value("OT_ABI_VERSION") == _capi.ABI_VERSION == 9
    for name in ("ot_fans_workspace", "ot_fans_transverse", "ot_fans_bands", "ot_fans_bins"):
        assert name in _capi.SIGNATURES and re.search(rf"\b{name}\(", text)
    assert ot.RayFans is fans.RayFans and callable(ot.Raytracer.ray_fans)
