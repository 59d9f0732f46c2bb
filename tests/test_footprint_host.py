"""Beam footprints without a device: the longdouble definition (tests/footprint_cases.py) on hand-made storages whose answers are
known by inspection, the argument checks of `Raytracer.footprints` and of the `ot_footprint_*` entry points, which come before any
device call, and the host-only parts of `ot.Footprints`."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd import footprint as fp

import footprint_cases as fc

NAN = np.nan


def storage(pos, weights):
    """pos (N, nt, 3), weights (N, nt) -> (p f64, w f32)"""
    return np.array(pos, dtype=np.float64), np.array(weights, dtype=np.float32)


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def three_rays():
    """Three rays, three sections; ray 2 dies at section 1 (its weight there is 0, its position NaN)."""
    p, w = storage([[[0, 0, 0], [1, 2, 5], [1, 2, 9]],
                    [[0, 0, 0], [3, 2, 5], [3, 2, 9]],
                    [[0, 0, 0], [NAN, NAN, NAN], [NAN, NAN, NAN]]],
                   [[1, 1, 0], [2, 0.5, 0], [4, 0, 0]])
    return p, w, [[0, 0], [2, 2], [0, 0]]


def test_oracle_three_rays_one_dying():
    p, w, axis = three_rays()
    val, mag = fc.records(p, w, 0, 3, axis)
    v = val.astype(np.float64)
    # section 0: all three alive at the origin; arriving = alive
    assert list(v[0, :4]) == [7, 3, 7, 3] and list(v[0, 4:7]) == [0, 0, 0] and list(v[0, 7:13]) == [0] * 6
    assert list(v[0, 13:]) == [0, 0, 0, 0]
    # section 1: rays 0 and 1 alive with weights 1 and 0.5, all three arrived with 7 W
    assert list(v[1, :4]) == [1.5, 2, 7, 3]
    assert list(v[1, 4:7]) == [1 * 1 + 0.5 * 3, 1.5 * 2, 1.5 * 5]
    assert list(v[1, 7:13]) == [1, 3, 2, 2, 5, 5]
    cx = 2.5 / 1.5  # centroid x; y = 2
    assert v[1, 13] == pytest.approx(1 * (1 - cx) ** 2 + 0.5 * (3 - cx) ** 2, rel=1e-15) and v[1, 14] == 0 and v[1, 15] == 0
    assert v[1, 16] == 1  # both rays are 1 away from the axis (2, 2)
    assert list(mag[1, [0, 2, 4, 5, 6]].astype(np.float64)) == [1.5, 7, 2.5, 3, 7.5]
    # the last section: nobody alive, two arrived
    assert list(v[2, :4]) == [0, 0, 1.5, 2] and np.all(np.isnan(v[2, 7:13])) and list(v[2, 13:]) == [0, 0, 0, 0]
    assert np.all(np.isfinite(val[:, fc.SUMS].astype(np.float64))), "the dead ray's NaN position reached a sum"


def test_oracle_ray_range_and_given_centroid():
    p, w, axis = three_rays()
    val, _ = fc.records(p, w, 1, 2, axis)  # rays 1 and 2 only
    v = val.astype(np.float64)
    assert list(v[0, :4]) == [6, 2, 6, 2] and list(v[1, :4]) == [0.5, 1, 6, 2]
    assert list(v[1, 4:7]) == [1.5, 1.0, 2.5] and list(v[1, 13:]) == [0, 0, 0, 1]
    # a centroid handed in is taken as it is
    val, _ = fc.records(p, w, 0, 3, axis, centroid=[[0, 0], [2, 1], [0, 0]])
    assert list(val[1, 13:16].astype(np.float64)) == [1 * 1 + 0.5 * 1, 1.5, 1 * (-1) * 1 + 0.5 * 1 * 1]


def test_oracle_empty_section_single_ray_and_dead_nan():
    # section 1: no living ray at all; section 2 (behind it) of course none either; a single living ray in section 0
    p, w = storage([[[1, -2, 0.5], [NAN, 7, 7], [NAN, NAN, NAN]],
                    [[NAN, NAN, NAN], [NAN, NAN, NAN], [NAN, NAN, NAN]]],
                   [[3, 0, 0], [0, 0, 0]])
    val, mag = fc.records(p, w, 0, 2, [[1, 1], [0, 0], [0, 0]])
    v = val.astype(np.float64)
    assert list(v[0, :7]) == [3, 1, 3, 1, 3, -6, 1.5] and list(v[0, 7:13]) == [1, 1, -2, -2, 0.5, 0.5]
    assert list(v[0, 13:]) == [0, 0, 0, 9]  # one ray: it is its own centroid; 3 below the axis
    assert list(v[1, :4]) == [0, 0, 3, 1] and np.all(np.isnan(v[1, 7:13])) and list(v[1, 13:]) == [0, 0, 0, 0]
    assert list(v[2, :4]) == [0, 0, 0, 0] and np.all(np.isnan(v[2, 7:13]))
    assert not np.any(np.isnan(mag.astype(np.float64)))


def test_oracle_cells():
    p, w = storage([[[-1, -1, 0]], [[1, 1, 0]], [[0, 0, 0]], [[0.999, -0.5, 0]], [[NAN, 0, 0]]], [[1], [2], [4], [8], [0]])
    p, w = np.repeat(p, 2, axis=1), np.repeat(w, 2, axis=1)  # two sections, the same in both
    rec = fc.records(p, w, 0, 5, [[0, 0], [0, 0]])[0].astype(np.float64)
    assert rec[0, 16] == 2
    got, cnt = fc.maps(p, w, 0, 5, [[0, 0], [0, 0]], rec, 4)
    R = np.sqrt(2.0)
    want = np.zeros((4, 4))
    for x, y, wt in ((-1, -1, 1), (1, 1, 2), (0, 0, 4), (0.999, -0.5, 8)):
        want[min(int((y + R) / (2 * R) * 4), 3), min(int((x + R) / (2 * R) * 4), 3)] += wt
    assert np.array_equal(got[0].astype(np.float64), want) and cnt[0].sum() == 4 and want[2, 2] == 4 and want[0, 0] == 1
    # R = 0: everything in cell 0, 0
    rec[1, 16] = 0
    assert fc.maps(p, w, 0, 5, [[0, 0], [0, 0]], rec, 4)[0][1, 0, 0] == 15


# ---- Raytracer.footprints: arguments ----------------------------------------------------------------------------------------------
def tracer():
    RT = ot.Raytracer(outline=[-1, 1, -1, 1, -1, 10])
    RT.add(ot.RaySource(ot.Point(), pos=[0, 0, 0]))
    return RT


@pytest.mark.parametrize("kwargs,error", [
    (dict(source_index=1.0), TypeError), (dict(source_index="0"), TypeError), (dict(source_index=True), TypeError),
    (dict(n_px=64.0), TypeError), (dict(n_px="64"), TypeError), (dict(n_px=True), TypeError), (dict(n_px=[64]), TypeError),
    (dict(n_px=0), ValueError), (dict(n_px=-3), ValueError), (dict(n_px=1025), ValueError),
])
def test_argument_errors_come_before_the_device(kwargs, error, monkeypatch):
    from optrace_amd import raytracer
    monkeypatch.setattr(raytracer, "require_device", lambda: pytest.fail("the device was asked for before the arguments were checked"))
    with pytest.raises(error):
        tracer().footprints(**kwargs)


def test_good_arguments_reach_the_device_and_then_the_rays(monkeypatch):
    from optrace_amd import raytracer
    asked = []
    monkeypatch.setattr(raytracer, "require_device", lambda: asked.append(1))
    for kwargs in (dict(), dict(source_index=0, n_px=1), dict(n_px=1024)):
        with pytest.raises(RuntimeError, match="No rays traced"):
            tracer().footprints(**kwargs)
    assert len(asked) == 3
    RT = ot.Raytracer(outline=[-1, 1, -1, 1, -1, 10])
    with pytest.raises(RuntimeError, match="Ray Sources Missing"):
        RT.footprints()


def test_no_device_is_a_backend_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("device present")
    with pytest.raises(ot.BackendError):
        tracer().footprints(n_px=8)


# ---- ot.Footprints --------------------------------------------------------------------------------------------------------------
def hand_records():
    """Four sections: 3 rays of 7 W at the source; 2 of 1.5 W behind a surface; 1 of 0.5 W behind the next; the empty end."""
    rec = np.zeros((4, 17))
    rec[0] = [7, 3, 7, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
    rec[1] = [1.5, 2, 7, 3, 2.5, 3, 7.5, 1, 3, 2, 2, 5, 5, 1.5 * 4, 1.5 * 9, 1.5 * 2, 4]
    rec[2] = [0.5, 1, 1.5, 2, 1.5, 1, 4.5, 3, 3, 2, 2, 9, 9, 1e-30, 1e-31, 1e-32, 1]
    rec[3] = [0, 0, 0.5, 1, 0, 0, 0, NAN, NAN, NAN, NAN, NAN, NAN, 0, 0, 0, 0]
    return rec


def hand_built(maps=None):
    return ot.Footprints(hand_records(), ["RS0", "L0 front", "L0 back", "end"], [[0, 0], [2, 2], [3, 1], [0, 0]],
                         [NAN, 4.0, 0.5, NAN], maps, long_desc="by hand")


def test_derived_fields():
    f = hand_built()
    assert f.labels == ("RS0", "L0 front", "L0 back", "end") and f.long_desc == "by hand"
    assert f.N.tolist() == [3, 2, 1, 0] and f.N_in.tolist() == [3, 3, 2, 1] and f.N.dtype == np.int64
    assert f.power.tolist() == [7, 1.5, 0.5, 0] and f.power_in.tolist() == [7, 7, 1.5, 0.5]
    assert f.loss.tolist() == [0, 5.5, 1.0, 0.5]
    assert f.transmission.tolist() == [1, 1.5 / 7, 0.5 / 1.5, 0]
    assert f.total_transmission == 0.5 / 7
    assert f.centroid[:3].tolist() == [[0, 0, 0], [2.5 / 1.5, 2, 5], [3, 2, 9]] and np.all(np.isnan(f.centroid[3]))
    assert f.extent[1].tolist() == [1, 3, 2, 2, 5, 5] and np.all(np.isnan(f.extent[3])) and f.extent.shape == (4, 6)
    assert f.rms_x[1] == 2 and f.rms_y[1] == 3 and f.cov_xy[1] == 2 and f.rms_radius[1] == np.sqrt(13)
    # one ray: exactly 0, whatever the second pass left in the record
    assert f.rms_x[2] == 0 and f.rms_y[2] == 0 and f.cov_xy[2] == 0 and f.rms_radius[2] == 0
    for a in (f.rms_x, f.rms_y, f.rms_radius, f.cov_xy, f.max_radius, f.fill):
        assert np.isnan(a[3])
    assert f.max_radius[:3].tolist() == [0, 2, 1]
    assert np.isnan(f.surface_radius[0]) and f.surface_radius[1:3].tolist() == [4, 0.5] and f.fill[1:3].tolist() == [0.5, 2]
    assert np.isnan(f.fill[0]) and f.records.shape == (4, 17)
    # nothing arrives: the transmission is no number; nothing emitted: neither the total
    rec = hand_records()
    rec[:, :4] = 0
    g = ot.Footprints(rec, list("abcd"), np.zeros((4, 2)), np.full(4, NAN))
    assert np.all(np.isnan(g.transmission)) and np.isnan(g.total_transmission) and g.N.tolist() == [0] * 4
    assert np.all(np.isnan(g.centroid)) and np.all(np.isnan(g.max_radius))


def test_result_object_is_locked_and_checks_its_shapes():
    f = hand_built()
    with pytest.raises(RuntimeError):
        f.power = 1.0
    with pytest.raises(ValueError):
        f.power[0] = 1
    with pytest.raises(AttributeError):
        f.something_else = 1
    with pytest.raises(ValueError):
        ot.Footprints(hand_records(), ["a", "b"], np.zeros((4, 2)), np.zeros(4))
    with pytest.raises(ValueError):
        ot.Footprints(hand_records()[:1], ["a"], np.zeros((1, 2)), np.zeros(1))
    with pytest.raises(ValueError):
        hand_built(np.zeros((4, 3, 2)))
    with pytest.raises(ValueError):
        hand_built(np.zeros((3, 2, 2)))


def test_image():
    with pytest.raises(ValueError, match="No maps"):
        hand_built().image(1)
    maps = np.arange(16, dtype=np.float64).reshape(4, 2, 2)
    f = hand_built(maps)
    for bad in (4, -5, 100):
        with pytest.raises(IndexError):
            f.image(bad)
    with pytest.raises(TypeError):
        f.image(1.0)
    img = f.image(1)
    assert isinstance(img, ot.ScalarImage) and np.array_equal(img.data, maps[1])
    assert list(img.extent) == [0, 4, 0, 4]  # axis (2, 2) +- max_radius 2
    assert list(f.image(2).extent) == [2, 4, 0, 2] and np.array_equal(f.image(-1).data, maps[3])
    assert "L0 front" in img.long_desc
    assert all(np.isfinite(f.image(i).extent).all() for i in (0, 3))  # (a point, no ray: a cell of some size)


def test_surface_radius():
    assert fp.surface_radius(ot.CircularSurface(r=2.5)) == 2.5
    assert fp.surface_radius(ot.RingSurface(r=3.0, ri=1.0)) == 3.0
    assert fp.surface_radius(ot.RectangularSurface(dim=[6, 8])) == 5.0
    assert fp.surface_radius(ot.SlitSurface(dim=[6, 8], dimi=[0.1, 0.2])) == 5.0
    assert fp.surface_radius(ot.SphericalSurface(r=1.5, R=10)) == 1.5


# ---- the entry points ------------------------------------------------------------------------------------------------------------
def test_entry_points_check_their_arguments_before_anything_else():
    """`ot_footprint_moments`, `ot_footprint_maps` (include/optrace_amd.h): a null argument, a ray range outside the storage and
    nt < 2 are refused with OT_ERR_INVALID, n_px outside 1 .. 1024 with OT_ERR_UNSUPPORTED, both before a device is looked for and
    with the entry point's name in the message; count = 0 is no work and no error."""
    lib = _capi.load_library()
    st = C.c_void_p()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)  # (never dereferenced: every call below returns from its checks)
    INVALID, UNSUPPORTED = -1, -3

    def rays(N=100, nt=3, p=a, w=a):
        r = _capi.Rays()
        r.N, r.nt, r.p, r.w = N, nt, p, w
        return C.byref(r)

    moments = lambda R, first, count, axis, ws, rec: lib.ot_footprint_moments(R, first, count, axis, ws, rec, st)
    for k in range(3):
        args = [a, a, a]
        args[k] = None
        assert moments(rays(), 0, 10, *args) == INVALID and b"ot_footprint_moments: null argument" in lib.ot_last_error()
    for R in (None, rays(p=None), rays(w=None)):
        assert moments(R, 0, 10, a, a, a) == INVALID and b"ot_footprint_moments: null argument" in lib.ot_last_error()
    for first, count in ((-1, 5), (0, -1), (0, 101), (91, 10), (101, 0)):
        assert moments(rays(), first, count, a, a, a) == INVALID and b"ot_footprint_moments: ray range" in lib.ot_last_error()
    for nt in (1, 0, -2):
        assert moments(rays(nt=nt), 0, 10, a, a, a) == INVALID and b"ot_footprint_moments: fewer than 2" in lib.ot_last_error()
    assert moments(rays(nt=65536), 0, 10, a, a, a) == UNSUPPORTED and b"ot_footprint_moments" in lib.ot_last_error()
    assert moments(rays(), 0, 0, a, a, a) == 0 and moments(rays(), 100, 0, a, a, a) == 0

    maps = lambda R, first, count, axis, rec, n_px, out: lib.ot_footprint_maps(R, first, count, axis, rec, n_px, out, st)
    for k in range(3):
        args = [a, a, 16, a]
        args[k + (k == 2)] = None
        assert maps(rays(), 0, 10, *args) == INVALID and b"ot_footprint_maps: null argument" in lib.ot_last_error()
    assert maps(None, 0, 10, a, a, 16, a) == INVALID and b"ot_footprint_maps: null argument" in lib.ot_last_error()
    assert maps(rays(), 95, 10, a, a, 16, a) == INVALID and b"ot_footprint_maps: ray range" in lib.ot_last_error()
    assert maps(rays(nt=1), 0, 10, a, a, 16, a) == INVALID and b"ot_footprint_maps: fewer than 2" in lib.ot_last_error()
    for n_px in (0, -1, 1025):
        assert maps(rays(), 0, 10, a, a, n_px, a) == UNSUPPORTED and b"ot_footprint_maps: n_px outside" in lib.ot_last_error()
    assert maps(rays(), 0, 0, a, a, 1025, a) == UNSUPPORTED  # (the limits hold whatever the count is)
    assert maps(rays(), 0, 0, a, a, 1024, a) == 0 and maps(rays(), 0, 0, a, a, 1, a) == 0


def test_workspace():
    """Doubles for the partial sums: 13 per workgroup of 256 rays and section, at most 1024 workgroups per section and piece of
    2^28 rays; 0 for arguments out of range."""
    ws = _capi.load_library().ot_footprint_workspace
    assert ws(1, 2) == 13 * 2 and ws(256, 3) == 13 * 3 and ws(257, 3) == 13 * 3 * 2
    assert ws(256 * 1024, 5) == ws(10 ** 8, 5) == 13 * 5 * 1024 and ws(2 ** 28 + 1, 2) == 13 * 2 * 1025
    assert ws(0, 3) == 0
    for count, nt in ((-1, 3), (10, 1), (10, 0), (10, -1), (10, 65536)):
        assert ws(count, nt) == 0


def test_constants_match_the_header():
    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "optrace_amd.h").read_text()
    value = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert value("OT_FP_M") == _capi.FP_M == fc.M == 17
    assert value("OT_FP_MAX_PX") == _capi.FP_MAX_PX == 1024
    assert value("OT_ABI_VERSION") == 9
    for name in ("ot_footprint_workspace", "ot_footprint_moments", "ot_footprint_maps"):
        assert name in _capi.SIGNATURES and re.search(rf"\b{name}\(", text)
