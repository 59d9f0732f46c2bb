"""What the device does with the preset catalogue, against the reference (tests/golden/presets.npz, trace_legrand_eye.npz,
trace_presets_achromat.npz; generator: tests/golden/generate_golden_presets.py with tests/scenes_presets.py): index
evaluation of all 45 media, tracing through preset glasses and the LeGrand eye, wavelength sampling from the new light
spectra, convolution with the preset PSFs.  Tolerances are those of the tests that pin the same kernels on synthetic
parameters (test_gpu_parity.py, test_gpu_spectrum_sampling.py, test_gpu_convolve.py)."""
import numpy as np
import pytest

import optrace_amd as ot
import scenes_presets as sp
from helpers import load, assert_close
from test_gpu_spectrum_sampling import WL0, WL1, normal_cdf, truncated_mean, truncated_std

pytestmark = pytest.mark.gpu

#: models whose device formula rounds like the reference's (test_gpu_parity.py::test_refraction_index): 4e-16, others 1e-13
EXACT_MODELS = ("Constant", "Abbe", "Data", "Sellmeier1", "Sellmeier3")


@pytest.fixture(scope="module")
def ref():
    return load("presets.npz")


def index_tolerance(model: str) -> float:
    return 4e-16 if model in EXACT_MODELS else 1e-13


# ---- index -------------------------------------------------------------------------------------------------------------
def test_refraction_index_of_all_media(ref):
    mod = ot.presets.refraction_index
    names = [str(n) for n in ref["media/names"]]
    assert len(names) == 45
    failures = []
    for j, name in enumerate(names):
        m = getattr(mod, name)
        assert m.spectrum_type == str(ref["media/type"][j])
        try:
            assert_close(m(ref["wl"]), ref["media/n"][j], rtol=index_tolerance(m.spectrum_type), what=f"{name} ({m.spectrum_type})")
        except AssertionError as err:
            failures.append(str(err))
    assert not failures, "\n".join(failures)


def test_abbe_number_of_all_media(ref):
    """V = (n_d - 1) / (n_F - n_C): an index error of tol * n is amplified by n_d / (n_F - n_C) in the quotient.  That factor is
    V * n_d / (n_d - 1), from the fixture's V and its index next to the d line."""
    mod = ot.presets.refraction_index
    failures = []
    for j, name in enumerate(str(n) for n in ref["media/names"]):
        m, V = getattr(mod, name), float(ref["media/abbe"][j])
        mine = m.abbe_number()
        assert type(mine) is float
        if not np.isfinite(V):
            assert mine == V and not m.is_dispersive(), name
            continue
        n_d = float(np.interp(ot.presets.spectral_lines.d, ref["wl"], ref["media/n"][j]))
        rtol = index_tolerance(m.spectrum_type) * V * n_d / (n_d - 1)
        if abs(mine - V) > rtol * abs(V):
            failures.append(f"{name} ({m.spectrum_type}): {mine!r} vs {V!r}, relative {abs(mine - V) / V:.3g} > {rtol:.3g}")
        assert m.is_dispersive(), name
    assert not failures, "\n".join(failures)


# ---- tracing -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(sp.SCENES))
def test_trace_matches_reference(name):
    """The assertions of test_gpu_parity.py::test_trace_matches_reference on scenes built from presets only."""
    g = load(f"trace_{name}.npz")
    with ot.global_options.no_warnings():
        RT = sp.SCENES[name][0](ot)
        assert int(g["N"]) == sp.SCENES[name][1]
        RT.trace(int(g["N"]), _initial_rays=(g["p0"], g["s0"], g["pol0"], g["w0"], g["wl"]), _N_list=g["N_list"])
    assert not RT.geometry_error
    r = RT.rays
    assert r.p_list.shape == g["p_list"].shape
    assert r.p_list.flags.f_contiguous and r.p_list.dtype == np.float64
    assert r.w_list.dtype == np.float32 and r.wl_list.dtype == np.float32 and r.n_list.dtype == np.float64
    assert np.array_equal(RT._msgs, g["msgs"]), f"counters differ:\n{RT._msgs}\n{g['msgs']}"
    assert np.array_equal(r.w_list > 0, g["w_list"] > 0), "alive masks per section must be bit-exact"
    assert_close(r.p_list, g["p_list"], rtol=1e-11, atol=1e-11, what="p_list")
    assert_close(r.n_list, g["n_list"], rtol=1e-13, what="n_list")
    assert_close(r.w_list, g["w_list"], rtol=2e-7, atol=1e-30, what="w_list")
    assert_close(r.s0_list, g["s_final"], rtol=1e-10, atol=1e-12, what="s_final")
    assert r.pol_list.dtype == np.float32
    assert_close(r.pol_list, g["pol_list"], rtol=1e-5, atol=2e-7, what="pol_list")


# ---- sampling ----------------------------------------------------------------------------------------------------------
# Gaussian components (relative amplitude of the normalised curve, mu, sigma) of the sRGB primary spectra, cut to the visible range
_R = [(75.1660756583 * 0.951190393, 639.854491, 30.0), (75.1660756583 * 0.951190393 * 0.0500907584, 418.905848, 80.6220465)]
_G = [(83.4999222966, 539.13108974, 33.31164968)]
_B = [(47.99521746361 * 1.16364585503, 454.833119, 20.1460206),
      (47.99521746361 * 1.16364585503 * 0.184484176, 459.658190, 71.0927568)]
MIXTURES = {"srgb_r": _R, "srgb_g": _G, "srgb_b": _B, "srgb_w": _R + _G + _B}


def mixture_mean_std(components) -> tuple:
    """Mean and standard deviation of a sum of Gaussians cut to [WL0, WL1], from the closed forms of the cut Gaussian."""
    mass = np.array([a * (normal_cdf(WL1, mu, sig) - normal_cdf(WL0, mu, sig)) for a, mu, sig in components])
    means = np.array([truncated_mean(mu, sig, WL0, WL1) for _, mu, sig in components])
    stds = np.array([truncated_std(mu, sig, WL0, WL1) for _, mu, sig in components])
    mean = np.sum(mass * means) / mass.sum()
    return mean, np.sqrt(np.sum(mass * (stds ** 2 + means ** 2)) / mass.sum() - mean ** 2)


@pytest.mark.parametrize("name", sp.NEW_LIGHT)
def test_random_wavelengths_of_new_light_spectra(name):
    """Means and standard deviations of 100 000 wavelengths against the closed forms, within the bounds of
    test_gpu_spectrum_sampling.py for line and Function spectra (0.005 nm)."""
    spec = getattr(ot.presets.light_spectrum, name)
    wl = spec.random_wavelengths(100_000)
    assert wl.shape == (100_000,)
    if spec.spectrum_type == "Lines":
        lines, vals = np.array(spec.lines, dtype=np.float64), np.array(spec.line_vals, dtype=np.float64)
        assert np.all(np.any(np.abs(wl[:, None] - lines) < 1000 * np.finfo(np.float32).eps, axis=1)), "only the lines occur"
        mean = np.sum(lines * vals) / vals.sum()
        std = np.sqrt(np.sum((lines - mean) ** 2 * vals / vals.sum()))
    elif name == "e":
        assert spec.spectrum_type == "Function"
        mean, std = (WL0 + WL1) / 2, (WL1 - WL0) / np.sqrt(12)
    else:
        assert spec.spectrum_type == "Function"
        mean, std = mixture_mean_std(MIXTURES[name])
    assert wl.min() >= WL0 and wl.max() <= WL1
    assert np.mean(wl) == pytest.approx(mean, abs=0.005)
    assert np.std(wl) == pytest.approx(std, abs=0.005)


# ---- convolution -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", sp.CONVOLVE_CASES)
def test_convolve_with_preset_psf_matches_reference(ref, case):
    """Image and PSF have the same pixel pitch (the reference's area resize is the identity there); tolerances of
    test_gpu_convolve.py::test_convolve_matches_reference."""
    psf = sp.psf(ot, case)
    with ot.global_options.no_warnings():
        res = ot.convolve(sp.sparse_image(ot, psf), psf)
    assert isinstance(res, ot.GrayscaleImage)
    d = res.data
    assert tuple(d.shape) == tuple(ref[f"convolve/{case}/shape"])
    np.testing.assert_allclose(res.extent, ref[f"convolve/{case}/extent"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(d[::4, ::4], ref[f"convolve/{case}/grid4"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(d.sum(), ref[f"convolve/{case}/sum"], rtol=1e-9)


@pytest.mark.parametrize("case", ["glare", "halo"])
def test_convolve_with_wide_psf_is_mirror_symmetric(case):
    """The 801 px PSFs against a 96 x 64 RGB image: they are much finer than the image, so they go through the area resize
    and have no reference value.  They are symmetric, so a mirrored image has to give the mirrored result."""
    psf = sp.psf(ot, case)
    assert psf.shape == (801, 801)
    data = sp.mirror_image()
    sides = [2 * psf.s[0] * 96 / 64, 2 * psf.s[1]]   # PSF half as high as the image
    with ot.global_options.no_warnings():
        res = ot.convolve(ot.RGBImage(data, sides), psf)
        d = res.data
        assert isinstance(res, ot.RGBImage) and d.ndim == 3 and d.shape[2] == 3
        assert d.shape[0] > 64 and d.shape[1] > 96 and np.isfinite(d).all()
        assert d.min() >= 0 and d.max() <= 1
        for axis in (0, 1):
            flipped = ot.convolve(ot.RGBImage(np.flip(data, axis=axis), sides), psf).data
            np.testing.assert_allclose(flipped, np.flip(d, axis=axis), rtol=0, atol=1e-12)
