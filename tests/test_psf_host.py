"""Huygens PSF without a device: argument checks of `Raytracer.huygens_psf` and of the `ot_psf_*` entry points, which come before
any device call, the host-only side of `ot.HuygensPSF`, and the physics of the definition on the longdouble truth alone."""
import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd import psf as hp

import psf_cases as pc
from test_wavefront_host import tracer


@pytest.mark.parametrize("kwargs,error", [
    (dict(n_px=8.0), TypeError), (dict(n_px="8"), TypeError), (dict(n_px=None), TypeError), (dict(n_px=True), TypeError),
    (dict(n_px=0), ValueError), (dict(n_px=-4), ValueError), (dict(n_px=1025), ValueError),
    (dict(size="1"), TypeError), (dict(size=[0.1]), TypeError), (dict(size=0), ValueError), (dict(size=0.0), ValueError),
    (dict(size=-0.1), ValueError), (dict(size=np.nan), ValueError), (dict(size=np.inf), ValueError),
    (dict(dz="0"), TypeError), (dict(dz=None), TypeError), (dict(dz=np.nan), ValueError), (dict(dz=-np.inf), ValueError),
    (dict(section=1.0), TypeError), (dict(section="1"), TypeError), (dict(section=-1), ValueError), (dict(section=3), ValueError),
    (dict(focus=3.0), TypeError), (dict(focus="abc"), TypeError), (dict(focus=[0, 1]), ValueError),
    (dict(focus=np.zeros((3, 1))), ValueError), (dict(focus=[0, np.nan, 1]), ValueError), (dict(focus=[0, np.inf, 1]), ValueError),
    (dict(focus=[1j, 0, 0]), TypeError),
    (dict(radius="1"), TypeError), (dict(radius=[1.0]), TypeError), (dict(radius=0), ValueError), (dict(radius=0.0), ValueError),
    (dict(radius=np.nan), ValueError), (dict(radius=-np.inf), ValueError),
    (dict(source_index=0.0), TypeError),
])
def test_argument_errors_come_before_the_device(kwargs, error):
    """(no rays traced, and on a machine without a device none could be: the argument is what the call complains about)"""
    with pytest.raises(error):
        tracer().huygens_psf(**kwargs)


def test_no_device_is_a_backend_error():
    import torch
    if torch.cuda.is_available():
        pytest.skip("device present")
    for kwargs in (dict(), dict(section=0), dict(section=2, focus=(0, 0, 20), radius=-3, n_px=1024, size=0.5, dz=-0.01),
                   dict(source_index=None, focus=np.array([0, 0, 20])), dict(n_px=1)):
        with pytest.raises(ot.BackendError):
            tracer().huygens_psf(**kwargs)


def test_entry_points_check_their_arguments_before_anything_else():
    pc.entry_point_argument_checks(_capi.load_library())
    assert (_capi.PSF_MAX_PX, _capi.PSF_REC) == (1024, 6)
    # the chunks follow from (n, n_px) alone: about 1024 workgroups, 128 rays per chunk at least
    assert _capi.psf_ws(1, 1) == 6 and _capi.psf_ws(257, 2) == 3 * 12 and _capi.psf_ws(70001, 8) == 547 * 132
    assert _capi.psf_ws(10 ** 6, 128) == 60 * (2 * 16385 + 2) and _capi.psf_ws(10 ** 6, 1024) == 2 * (1024 * 1024 + 1) + 2


def hand_built(**kwargs):
    inten = np.array([[0.01, 0.02, 0.01], [0.03, 0.64, 0.02], [0.0, 0.04, 0.01]])
    return ot.HuygensPSF(1000, 2.5, 1, 2, (0, 0, 20), -9.0, 550.0, 0.03, 0.01, inten, 0.8, 1e-3, long_desc="by hand", **kwargs)


def test_result_object_and_image():
    psf = hand_built()
    assert psf.N == 1000 and psf.power == 2.5 and psf.n_missed == 1 and psf.section == 2 and psf.radius == -9 and psf.long_desc == "by hand"
    assert isinstance(psf.N, int) and isinstance(psf.strehl, float) and psf.focus.dtype == np.float64
    assert psf.size == 0.03 and psf.dz == 0.01 and psf.wavelength == 550 and psf.strehl == 0.8 and psf.noise_floor == 1e-3
    assert psf.peak == 0.64 and psf.intensity.shape == (3, 3)
    with pytest.raises(RuntimeError):  # locked like other result objects
        psf.strehl = 1.0
    for arr in (psf.focus, psf.intensity):
        assert not arr.flags.writeable
        with pytest.raises(ValueError):
            arr[0] = 1
    with pytest.raises(AttributeError):
        psf.something_else = 1
    assert ot.HuygensPSF._tracked is False
    img = psf.to_image()
    assert isinstance(img, ot.GrayscaleImage) and img.shape == (3, 3)
    np.testing.assert_allclose(img.extent, [-0.015, 0.015, -0.015, 0.015], rtol=0, atol=1e-18)
    assert img.s == pytest.approx([0.03, 0.03], rel=1e-15)
    d = img.data
    assert d.min() >= 0 and d.max() <= 1 and d[1, 1] == pytest.approx(1, abs=1e-15) and np.argmax(d) == 4
    assert d[2, 0] == 0 and d[0, 1] > d[0, 0] > 0
    # `convolve` removes the gamma of a GrayscaleImage: what it then works on is intensity / peak
    from optrace_amd.image import srgb_to_srgb_linear
    np.testing.assert_allclose(srgb_to_srgb_linear(d), psf.intensity / psf.peak, rtol=0, atol=1e-15)


def test_empty_result():
    psf = hp._empty(2, None, None, 5, None, 0.0, long_desc="nothing")
    pc.check_empty(psf, 5)
    assert psf.section == 2 and psf.n_missed == 0 and np.all(np.isnan(psf.focus)) and np.isnan(psf.radius) and np.isnan(psf.size)
    assert psf.dz == 0
    kept = hp._empty(0, np.array([0.0, 0.0, 1.0]), 2.0, 1, 0.25, -0.5, n_missed=7)  # what the caller fixed stays
    pc.check_empty(kept, 1)
    assert np.array_equal(kept.focus, [0, 0, 1]) and kept.radius == 2 and kept.size == 0.25 and kept.dz == -0.5 and kept.n_missed == 7
    with pytest.raises(RuntimeError):
        kept.to_image()


def test_default_size_and_figures():
    mom = np.zeros(11)
    mom[0], mom[5], mom[10] = 2.0, 2 * 500.0, 0.05  # mean wavelength 500 nm, pupil radius 0.05: NA 0.05 in air
    assert hp.default_size(mom) == pytest.approx(10 * 500e-6 / 0.05, rel=1e-15)  # 0.1 mm, 8.2 Airy diameters of 1.22 lambda / NA
    mom[10] = 0
    assert not np.isfinite(hp.default_size(mom))
    field = np.array([[[3.0, 0.0]], [[4.0, 1.0]]])
    inten, strehl, floor = hp.figures(field, np.array([6.0, 8.0, 10.0, 2.0]))
    assert np.array_equal(inten, [[0.25, 0.01]]) and strehl == 1 and floor == 0.02


def bessel_j1(x):
    """J1(x) = (1 / pi) int_0^pi cos(t - x sin t) dt; the midpoint rule on a periodic integrand converges geometrically."""
    t = (np.arange(256) + 0.5) * np.pi / 256
    return np.cos(t[None] - np.asarray(x, dtype=np.float64)[:, None] * np.sin(t)[None]).mean(axis=1)


AIRY_DEVIATION = 2 * 2.8e-5  # twice the truth's own largest deviation from Airy, measured on the CPU: 2.73e-5 of the peak


def test_perfect_wave_gives_the_airy_pattern():
    """A perfect spherical wave of NA 0.05 at 550 nm, 20172 rays on a stratified disc, R = 100 mm, 33 x 33 points over 0.04 mm:
    the longdouble sum along the central row against (2 J1(x) / x)^2, x = 2 pi NA r / lambda.  The sum differs from Airy's
    integral by the rule's discretisation (the rings), by the missing obliquity factor and by sin against tan of the aperture
    angle, O(NA^2) = 2.5e-3 of the pattern's slope; the deviation measured on the CPU is 2.73e-5 of the peak, and twice
    that (rounded up) is allowed."""
    na, wl, n_px, size = 0.05, 550.0, 33, 0.04
    rec = pc.perfect_wave(82, na, wl, 100.0)
    assert rec.shape == (6, 20172)
    row = 16 * n_px + np.arange(n_px)
    re, im, bound, A, A2, b_tau = pc.truth(rec, 100.0, n_px, size, 0.0, points=np.append(row, n_px * n_px))
    inten = ((re * re + im * im) / (A * A)).astype(np.float64)
    assert inten[-1] == pytest.approx(1, abs=1e-12), "Strehl ratio of a perfect wave"
    assert inten[16] == inten[-1], "with an odd n_px the middle pixel lies on the axis"
    assert float(A2 / (A * A)) == pytest.approx(1 / 20172, rel=1e-12), "noise floor of equal weights: 1 / N"
    r = (np.arange(n_px) + 0.5 - n_px / 2) * size / n_px
    x = 2 * np.pi * na * np.abs(r) / (wl * 1e-6)
    with np.errstate(invalid="ignore", divide="ignore"):
        airy = np.where(x > 0, (2 * bessel_j1(x) / x) ** 2, 1.0)
    dev = np.abs(inten[:-1] - airy).max()
    print("largest deviation from Airy", dev, "phase bound", b_tau)
    assert dev <= AIRY_DEVIATION
    # the first minimum: 0.61 lambda / NA from the axis, within one pixel
    right = inten[16:-1]
    first_min = int(np.argmax((right[1:-1] < right[:-2]) & (right[1:-1] < right[2:]))) + 1
    assert abs(first_min * size / n_px - 0.61 * wl * 1e-6 / na) <= size / n_px
    assert right[first_min] < 1e-2
