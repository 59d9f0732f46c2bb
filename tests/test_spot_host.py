"""Spot analysis without a device: argument checks of `Raytracer.spot_analysis` and of the `ot_spot_*` entry points, which come
before any device call, and the host-only methods of `ot.SpotAnalysis`."""
import ctypes as C

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi


def tracer():
    RT = ot.Raytracer(outline=[-1, 1, -1, 1, -1, 10])
    RT.add(ot.RaySource(ot.Point(), pos=[0, 0, 0]))
    RT.add(ot.Detector(ot.RectangularSurface(dim=[1, 1]), pos=[0, 0, 5]))
    return RT


@pytest.mark.parametrize("kwargs,error", [
    (dict(n_radii=1.5), TypeError), (dict(n_radii="3"), TypeError), (dict(n_radii=True), TypeError),
    (dict(n_radii=0), ValueError), (dict(n_radii=-4), ValueError), (dict(n_radii=65537), ValueError),
    (dict(frequencies=3.0), TypeError), (dict(frequencies="12"), TypeError), (dict(frequencies=[1j, 2]), TypeError),
    (dict(frequencies=np.zeros((2, 3))), ValueError), (dict(frequencies=[[1.0, 2.0]]), ValueError),
    (dict(frequencies=[0.0, np.nan]), ValueError), (dict(frequencies=[0.0, np.inf]), ValueError),
    (dict(frequencies=np.zeros(4097)), ValueError),
])
def test_argument_errors_come_before_the_device(kwargs, error):
    """(no rays traced, and on a machine without a device none could be: the argument is what the call complains about)"""
    with pytest.raises(error):
        tracer().spot_analysis(**kwargs)


def test_no_device_is_a_backend_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("device present")
    for kwargs in (dict(), dict(n_radii=65536, frequencies=np.zeros(4096)), dict(frequencies=[]), dict(n_radii=1, frequencies=(0, 1))):
        with pytest.raises(ot.BackendError):
            tracer().spot_analysis(**kwargs)


def test_entry_points_check_their_arguments_before_anything_else():
    """`ot_spot_moments`, `ot_spot_radial`, `ot_spot_otf` (include/optrace_amd.h): null arguments are refused with OT_ERR_INVALID,
    radial bins and frequencies beyond the limits with OT_ERR_UNSUPPORTED, both before a device is looked for and with the entry
    point's name in the message; n = 0 is no work and no error.  Only `fill` may be null (a dense list)."""
    lib = _capi.load_library()
    st = C.c_void_p()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)  # (never dereferenced: every call below returns from its checks)
    INVALID, UNSUPPORTED = -1, -3

    moments = lambda n, x, y, w, ws, mom: lib.ot_spot_moments(n, None, x, y, w, ws, mom, st)
    good = [a] * 5
    for k in range(5):
        args = list(good)
        args[k] = None
        assert moments(10, *args) == INVALID and b"ot_spot_moments: null argument" in lib.ot_last_error()
    assert moments(-1, *good) == INVALID and b"ot_spot_moments" in lib.ot_last_error()
    assert moments(0, *good) == 0

    radial = lambda n, x, y, w, mom, n_radii, hist: lib.ot_spot_radial(n, None, x, y, w, mom, n_radii, hist, st)
    for k in range(5):
        args = [a, a, a, a, 32, a]
        args[k + (k == 4)] = None
        assert radial(10, *args) == INVALID and b"ot_spot_radial: null argument" in lib.ot_last_error()
    assert radial(10, a, a, a, a, 0, a) == INVALID and b"ot_spot_radial" in lib.ot_last_error()
    assert radial(10, a, a, a, a, 65537, a) == UNSUPPORTED and b"ot_spot_radial: more than 65536" in lib.ot_last_error()
    assert radial(0, a, a, a, a, 65537, a) == UNSUPPORTED  # (the limits hold whatever n is)
    assert radial(0, a, a, a, a, 65536, a) == 0

    otf = lambda n, x, y, w, mom, freq, K, ws, out: lib.ot_spot_otf(n, None, x, y, w, mom, freq, K, ws, out, st)
    for k in range(7):
        args = [a, a, a, a, a, 17, a, a]
        args[k + (k >= 5)] = None
        assert otf(10, *args) == INVALID and b"ot_spot_otf: null argument" in lib.ot_last_error()
    assert otf(10, a, a, a, a, a, 0, a, a) == INVALID and b"ot_spot_otf" in lib.ot_last_error()
    assert otf(10, a, a, a, a, a, 4097, a, a) == UNSUPPORTED and b"ot_spot_otf: more than 4096" in lib.ot_last_error()
    assert otf(0, a, a, a, a, a, 4096, a, a) == 0
    # the workspace the binding asks for is the header's OT_SPOT_WS(K)
    assert _capi.spot_ws(0) == 32 * 2048 + 256 * 8 and _capi.spot_ws(4096) == 32 * 2048 + 256 * 4104


def hand_built(ee, max_radius=4.0, N=10):
    K = 3
    return ot.SpotAnalysis(N, 2.5, (1.0, -2.0), 0.3, 0.4, 0.01, max_radius, [0, 2, -3, -1], ee, [0, 1, 2],
                           np.array([1, 0.5j, -0.25]), np.ones(K), long_desc="by hand")


def test_result_object():
    sa = hand_built([0, 0.1, 0.4, 0.8, 1.0])
    assert sa.N == 10 and sa.power == 2.5 and sa.rms_radius == 0.5 and sa.long_desc == "by hand"
    assert np.array_equal(sa.ee_radii, [0, 1, 2, 3, 4])
    assert np.array_equal(sa.mtf_x, [1, 0.5, 0.25]) and sa.otf_x.dtype == np.complex128
    with pytest.raises(RuntimeError):  # locked like other result objects
        sa.power = 1.0
    with pytest.raises(ValueError):
        sa.ee[0] = 1
    with pytest.raises(AttributeError):
        sa.something_else = 1


def test_encircled_energy_and_its_inverse():
    sa = hand_built([0, 0.1, 0.4, 0.8, 1.0])
    # interior interpolation, the edges themselves, beyond the last radius
    assert sa.encircled_energy(0) == 0 and sa.encircled_energy(2) == 0.4
    assert sa.encircled_energy(1.5) == pytest.approx(0.25, rel=1e-15) and sa.encircled_energy(3.5) == pytest.approx(0.9, rel=1e-15)
    assert sa.encircled_energy(4) == 1 and sa.encircled_energy(4.001) == 1 and sa.encircled_energy(1e9) == 1
    assert np.allclose(sa.encircled_energy(np.array([0.5, 2.5])), [0.05, 0.6], rtol=1e-15)
    assert sa.radius_of(0.4) == 2 and sa.radius_of(1.0) == 4 and sa.radius_of(1) == 4
    assert sa.radius_of(0.25) == pytest.approx(1.5, rel=1e-15) and sa.radius_of(0.05) == pytest.approx(0.5, rel=1e-15)
    assert np.allclose(sa.radius_of(np.array([0.6, 0.9])), [2.5, 3.5], rtol=1e-15)
    for r in (0.3, 1.7, 3.99):
        assert sa.radius_of(sa.encircled_energy(r)) == pytest.approx(r, rel=1e-14)
    for bad in (0, -0.1, 1.0000001, np.nan):
        with pytest.raises(ValueError):
            sa.radius_of(bad)
    # steps: a flat stretch is entered at its left edge, and left behind from its right edge
    step = hand_built([0, 0, 0.5, 0.5, 1.0])
    assert step.radius_of(0.5) == 2 and step.radius_of(0.25) == pytest.approx(1.5) and step.radius_of(0.75) == pytest.approx(3.5)
    assert step.radius_of(1.0) == 4 and step.encircled_energy(2.5) == 0.5
    # a single hit: every radius is 0 and holds everything
    one = hand_built([0, 1, 1, 1], max_radius=0.0, N=1)
    assert np.array_equal(one.ee_radii, np.zeros(4))
    assert one.radius_of(1.0) == 0 and one.radius_of(0.3) == 0 and one.encircled_energy(0) == 1 and one.encircled_energy(2) == 1
    # no hit
    none = hand_built(np.zeros(5), max_radius=np.nan, N=0)
    assert none.encircled_energy(1.0) == 0 and np.isnan(none.radius_of(0.5))
