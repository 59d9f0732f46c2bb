"""Wavefront analysis without a device: argument checks of `Raytracer.wavefront_analysis` and of the `ot_wavefront_*` entry points,
which come before any device call, the host function `zernike`, and the host-only side of `ot.WavefrontAnalysis`."""
import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd import wavefront as wf

import wavefront_cases as wc
from wavefront_cases import check_empty


def tracer():
    """Two tracing surfaces: nt = 4, sections 0 .. 2."""
    RT = ot.Raytracer(outline=[-5, 5, -5, 5, -1, 30])
    RT.add(ot.RaySource(ot.Point(), pos=[0, 0, 0]))
    RT.add(ot.Lens(ot.SphericalSurface(r=3, R=10), ot.SphericalSurface(r=3, R=-10), n=ot.RefractionIndex("Constant", n=1.5),
                   pos=[0, 0, 10], d=1))
    return RT


@pytest.mark.parametrize("kwargs,error", [
    (dict(n_zernike=1.5), TypeError), (dict(n_zernike="3"), TypeError), (dict(n_zernike=True), TypeError),
    (dict(n_zernike=0), ValueError), (dict(n_zernike=-2), ValueError), (dict(n_zernike=37), ValueError),
    (dict(n_grid=8.0), TypeError), (dict(n_grid=None), TypeError), (dict(n_grid=0), ValueError), (dict(n_grid=1025), ValueError),
    (dict(section=1.0), TypeError), (dict(section="1"), TypeError), (dict(section=-1), ValueError), (dict(section=3), ValueError),
    (dict(focus=3.0), TypeError), (dict(focus="abc"), TypeError), (dict(focus=[0, 1]), ValueError),
    (dict(focus=np.zeros((3, 1))), ValueError), (dict(focus=[0, np.nan, 1]), ValueError), (dict(focus=[0, np.inf, 1]), ValueError),
    (dict(focus=[1j, 0, 0]), TypeError),
    (dict(radius="1"), TypeError), (dict(radius=[1.0]), TypeError), (dict(radius=0), ValueError), (dict(radius=0.0), ValueError),
    (dict(radius=np.nan), ValueError), (dict(radius=-np.inf), ValueError),
    (dict(pupil_radius="1"), TypeError), (dict(pupil_radius=0.0), ValueError), (dict(pupil_radius=-0.5), ValueError),
    (dict(pupil_radius=np.nan), ValueError), (dict(pupil_radius=np.inf), ValueError),
    (dict(source_index=0.0), TypeError),
])
def test_argument_errors_come_before_the_device(kwargs, error):
    """(no rays traced, and on a machine without a device none could be: the argument is what the call complains about)"""
    with pytest.raises(error):
        tracer().wavefront_analysis(**kwargs)


def test_no_device_is_a_backend_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("device present")
    for kwargs in (dict(), dict(section=0), dict(section=2, focus=(0, 0, 20), radius=-3, pupil_radius=0.5, n_zernike=36, n_grid=1024),
                   dict(source_index=None, focus=np.array([0, 0, 20])), dict(n_zernike=1, n_grid=1)):
        with pytest.raises(ot.BackendError):
            tracer().wavefront_analysis(**kwargs)


def test_entry_points_check_their_arguments_before_anything_else():
    wc.entry_point_argument_checks(_capi.load_library())
    # the constants of the binding are the header's
    assert (_capi.WF_FOCUS_M, _capi.WF_M, _capi.WF_MAX_J, _capi.WF_MAX_GRID, _capi.WF_WS) == (17, 11, 36, 1024, 40 * 2048)


def disc_rule(n_rho=12, n_theta=40):
    """Gauss-Legendre in t = rho^2 over [0, 1] times a uniform rule in theta: exact for polynomials of degree below 2 n_rho in t
    and for trigonometric orders below n_theta, so for every product Z_i Z_j with i, j <= 36 (degree 7 in t, order 14).
    -> x, y, weights that sum to pi."""
    node, weight = np.polynomial.legendre.leggauss(n_rho)
    t, wt = (node + 1) / 2, weight / 2
    theta = np.arange(n_theta) * (2 * np.pi / n_theta)
    rho = np.sqrt(t)[:, None]
    return rho * np.cos(theta), rho * np.sin(theta), np.repeat(wt[:, None], n_theta, axis=1) * (np.pi / n_theta)


def test_zernike_polynomials_are_orthonormal_on_the_disc():
    x, y, wq = disc_rule()
    assert wq.sum() == pytest.approx(np.pi, rel=1e-15)
    Z = np.array([wf.zernike(j, x, y) for j in range(1, 37)])
    gram = np.einsum("iab,jab,ab->ij", Z, Z, wq)
    err = np.abs(gram - np.pi * np.eye(36)).max()
    print("largest deviation from pi * identity", err)
    assert err < 1e-12


def test_zernike_closed_forms_and_order():
    rng = np.random.default_rng(5)
    rho, theta = np.sqrt(rng.uniform(0, 1, 200)), rng.uniform(-np.pi, np.pi, 200)
    x, y = rho * np.cos(theta), rho * np.sin(theta)
    tol = dict(rtol=0, atol=1e-13)
    np.testing.assert_allclose(wf.zernike(1, x, y), np.ones(200), **tol)
    np.testing.assert_allclose(wf.zernike(4, x, y), np.sqrt(3) * (2 * rho ** 2 - 1), **tol)
    np.testing.assert_allclose(wf.zernike(11, x, y), np.sqrt(5) * (6 * rho ** 4 - 6 * rho ** 2 + 1), **tol)
    # even j carries the cosine term
    np.testing.assert_allclose(wf.zernike(2, x, y), 2 * x, **tol)
    np.testing.assert_allclose(wf.zernike(3, x, y), 2 * y, **tol)
    np.testing.assert_allclose(wf.zernike(6, x, y), np.sqrt(6) * rho ** 2 * np.cos(2 * theta), **tol)
    np.testing.assert_allclose(wf.zernike(5, x, y), np.sqrt(6) * rho ** 2 * np.sin(2 * theta), **tol)
    np.testing.assert_allclose(wf.zernike(7, x, y), np.sqrt(8) * (3 * rho ** 3 - 2 * rho) * np.sin(theta), **tol)
    np.testing.assert_allclose(wf.zernike(8, x, y), np.sqrt(8) * (3 * rho ** 3 - 2 * rho) * np.cos(theta), **tol)
    np.testing.assert_allclose(wf.zernike(22, x, y), np.sqrt(7) * (20 * rho ** 6 - 30 * rho ** 4 + 12 * rho ** 2 - 1), **tol)
    assert [wf.noll_indices(j) for j in (1, 2, 3, 4, 10, 11, 15, 22, 28, 29, 36)] == [
        (0, 0), (1, 1), (1, -1), (2, 0), (3, 3), (4, 0), (4, -4), (6, 0), (6, 6), (7, -1), (7, 7)]
    # the centre of the disc is a point like any other; scalars come back as scalars
    assert wf.zernike(4, 0.0, 0.0) == pytest.approx(-np.sqrt(3), rel=1e-15) and wf.zernike(7, 0.0, 0.0) == 0
    for bad, error in ((0, ValueError), (37, ValueError), (1.0, TypeError)):
        with pytest.raises(error):
            wf.zernike(bad, x, y)
    # the longdouble restatement the GPU tests use is the same function
    for j in (1, 5, 16, 29, 36):
        np.testing.assert_allclose(wc.zernike_ld(j, x.astype(np.longdouble), y.astype(np.longdouble)).astype(np.float64), wf.zernike(j, x, y), **tol)
        assert np.all(wc.zernike_abs(j, x, y) >= np.abs(wf.zernike(j, x, y)) - 1e-13)


def hand_built(rms=25e-6, wavelength=500.0):
    return ot.WavefrontAnalysis(10, 2.5, 1, 2, (0, 0, 20), -9.0, wavelength, 31.5, rms, -1e-4, 3e-4, (0.01, -0.02), 0.25,
                                np.arange(6.0), np.full((4, 4), 1e-5), np.ones((4, 4)), long_desc="by hand")


def test_result_object():
    wa = hand_built()
    assert wa.N == 10 and wa.power == 2.5 and wa.n_missed == 1 and wa.section == 2 and wa.radius == -9 and wa.long_desc == "by hand"
    assert isinstance(wa.N, int) and isinstance(wa.rms, float) and wa.focus.dtype == np.float64
    assert wa.pv == pytest.approx(4e-4, rel=1e-15) and wa.opd_min == -1e-4 and wa.opd_max == 3e-4
    assert wa.zernike.shape == (6,) and wa.opd_map.shape == wa.weight_map.shape == (4, 4)
    # 25 nm RMS at 500 nm: a twentieth of a wave
    assert wa.rms_waves == pytest.approx(0.05, rel=1e-14) and wa.pv_waves == pytest.approx(0.8, rel=1e-14)
    assert wa.strehl == pytest.approx(np.exp(-(2 * np.pi * 0.05) ** 2), rel=1e-14)
    assert hand_built(rms=0.0).strehl == 1
    with pytest.raises(RuntimeError):  # locked like other result objects
        wa.rms = 1.0
    for arr in (wa.focus, wa.pupil_centre, wa.zernike, wa.opd_map, wa.weight_map):
        assert not arr.flags.writeable
        with pytest.raises(ValueError):
            arr[0] = 1
    with pytest.raises(AttributeError):
        wa.something_else = 1
    assert ot.WavefrontAnalysis._tracked is False


def test_empty_result():
    wa = wf._empty(2, None, None, 15, 8, long_desc="nothing")
    check_empty(wa, 15, 8)
    assert wa.section == 2 and wa.n_missed == 0 and np.all(np.isnan(wa.focus)) and np.isnan(wa.radius)
    kept = wf._empty(0, np.array([0.0, 0.0, 1.0]), 2.0, 3, 1, n_missed=7)  # what the caller fixed stays
    check_empty(kept, 3, 1)
    assert np.array_equal(kept.focus, [0, 0, 1]) and kept.radius == 2 and kept.n_missed == 7


def test_reference_sphere_from_sums():
    """The host half of the default sphere: rays through one point from a ring of starts meet there."""
    focus_true, origin = np.array([0.3, -0.2, 40.0]), np.array([0.0, 0.0, 10.0])
    ang = np.linspace(0, 2 * np.pi, 12, endpoint=False)
    p = np.stack([2 * np.cos(ang), 2 * np.sin(ang), np.full(12, 10.0)], axis=1)
    far = focus_true + 0.5 * (focus_true - p)  # the sections end behind the focus
    w = np.ones((12, 2), dtype=np.float32)
    val, _, n = wc.focus_sums(np.stack([p, far], axis=1), w, 0, 0, 12, origin)
    assert n == 12
    c, R = wf.reference_sphere(val.astype(np.float64), origin, None, None)
    np.testing.assert_allclose(c, focus_true, rtol=0, atol=1e-12)
    assert R == pytest.approx(np.linalg.norm(focus_true - [0, 0, 10]), rel=1e-13)  # converging: positive
    # the same lines run backwards diverge from the point: negative radius
    val, _, _ = wc.focus_sums(np.stack([far, far + (far - p)], axis=1), w, 0, 0, 12, origin)
    c, R = wf.reference_sphere(val.astype(np.float64), origin, None, None)
    np.testing.assert_allclose(c, focus_true, rtol=0, atol=1e-11)
    assert R < 0
    # what the caller gives stays; parallel rays have no closest point
    c, R = wf.reference_sphere(val.astype(np.float64), origin, np.array([0.0, 0.0, 1.0]), 3.0)
    assert np.array_equal(c, [0, 0, 1]) and R == 3
    par = np.stack([p, p + [0, 0, 5.0]], axis=1)
    val, _, _ = wc.focus_sums(par, w, 0, 0, 12, origin)
    with pytest.raises(RuntimeError):
        wf.reference_sphere(val.astype(np.float64), origin, None, None)
    # the packed normal equations unfold into a symmetric matrix
    G, g = wf.unpack_normal_equations(np.arange(9.0), 3)
    assert np.array_equal(G, [[0, 1, 2], [1, 3, 4], [2, 4, 5]]) and np.array_equal(g, [6, 7, 8])
