"""ot.color without a GPU: its names, constants and re-exports, the host functions (observers, xyz_from_spectrum, dominant
and complementary wavelength) and the host figures of the spectrum classes against tests/golden/color.npz (generator:
tests/golden/generate_golden_color.py), that the device functions refuse to run without a device, and the fixture itself.

Tolerances: rtol 1e-9 with atol 1e-12, NaN positions equal.  For the wavelengths 1e-9 of about 500 nm is 5e-7 nm; the
generator asserts that one ulp of the input moves no recorded wavelength by more than 1e-7 nm (D65 itself, which sits on
the whitepoint, is recorded for xyz() and color() only)."""
import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import spectrum, image
from helpers import load, assert_close
import color_cases as cc

CONSTANTS = ["WP_D65_XY", "WP_D65_XYZ", "WP_D65_LUV", "WP_D65_UV", "SRGB_R_XY", "SRGB_G_XY", "SRGB_B_XY", "SRGB_R_UV",
             "SRGB_G_UV", "SRGB_B_UV", "SRGB_PRIMARY_POWER_FACTORS"]
ILLUMINANTS = ["a", "c", "d50", "d55", "d65", "d75", "e", "f2", "f7", "f11", "led_b1", "led_b2", "led_b3", "led_b4", "led_b5",
               "led_bh1", "led_rgb1", "led_v1", "led_v2"]
HOST = ["wavelengths", "blackbody", "normalized_blackbody", "x_observer", "y_observer", "z_observer", "xyz_from_spectrum",
        "dominant_wavelength", "complementary_wavelength", "srgb_to_srgb_linear", "srgb_linear_to_srgb",
        "power_from_srgb_linear", "srgb_r_primary", "srgb_g_primary", "srgb_b_primary"]
DEVICE = ["xyz_to_xyY", "xyY_to_xyz", "xyz_to_luv", "luv_to_xyz", "luv_to_u_v_l", "luv_saturation", "luv_chroma", "luv_hue",
          "srgb_linear_to_xyz", "srgb_to_xyz", "xyz_to_srgb_linear", "xyz_to_srgb", "outside_srgb_gamut", "get_chroma_scale",
          "log_srgb", "spectral_colormap"]
TOL = dict(rtol=1e-9, atol=1e-12)


@pytest.fixture(scope="module")
def g():
    return load("color.npz")


def test_names_constants_and_reexports(g):
    color = ot.color
    for name in CONSTANTS + ["SRGB_RENDERING_INTENTS"] + HOST + DEVICE + [f"{n}_illuminant" for n in ILLUMINANTS]:
        assert hasattr(color, name), name
    assert not hasattr(color, "random_wavelengths_from_srgb")  # drawn inside the generation kernel: DESIGN.md section 8
    for name in CONSTANTS:
        assert np.array_equal(np.array(getattr(color, name), dtype=np.float64), g[f"const/{name}"]), name
    assert list(color.SRGB_RENDERING_INTENTS) == [str(s) for s in g["const/SRGB_RENDERING_INTENTS"]]
    for name in ("wavelengths", "blackbody", "normalized_blackbody", "d65_illuminant"):
        assert getattr(color, name) is getattr(spectrum, name), name
    for name in ("srgb_to_srgb_linear", "srgb_linear_to_srgb", "power_from_srgb_linear", "srgb_r_primary", "srgb_g_primary",
                 "srgb_b_primary", "SRGB_PRIMARY_POWER_FACTORS"):
        assert getattr(color, name) is getattr(image, name), name
    wl = np.array([300.0, 455.5, 560.0, 781.0, 900.0])
    for name in ILLUMINANTS:  # all of them are spectrum.illuminant(name) of the CIE name
        cie = name.upper().replace("_", "-")
        assert np.array_equal(getattr(color, f"{name}_illuminant")(wl), spectrum.illuminant(cie)(wl)), name
    assert np.array_equal(color.e_illuminant(wl), np.full(5, 100.0))


def test_observers_and_xyz_from_spectrum(g):
    wl = g["observers/wl"]
    assert wl.tobytes() == cc.observer_wavelengths().tobytes()
    for c in "xyz":
        got = getattr(ot.color, f"{c}_observer")(wl)
        assert_close(got, g[f"observers/{c}"], **TOL, what=f"{c}_observer")
        assert np.all(got[(wl < 360) | (wl > 830)] == 0)
    wl, spec = cc.spectrum_samples()
    assert wl.tobytes() == g["xyz_from_spectrum/wl"].tobytes() and spec.tobytes() == g["xyz_from_spectrum/spec"].tobytes()
    assert_close(ot.color.xyz_from_spectrum(wl, spec), g["xyz_from_spectrum/sum"], **TOL, what="sum")
    assert_close(ot.color.xyz_from_spectrum(wl, spec, method="trapz"), g["xyz_from_spectrum/trapz"], **TOL, what="trapz")
    assert np.abs(g["xyz_from_spectrum/sum"] - g["xyz_from_spectrum/trapz"]).max() > 1e-6  # the method is seen


@pytest.mark.parametrize("name", ["spectral", "ring"])
def test_dominant_and_complementary_wavelength(g, name):
    """NaN where the reference has NaN (purples for the dominant, greens for the complementary wavelength: no clamping to the
    ends of the locus), and the reference's value elsewhere -- including the angles between 699 and 780 nm, where the locus
    runs backwards and the reference's interpolation sorts its samples."""
    xyz = g[f"wavelengths/{name}/xyz"]
    dom = np.array([ot.color.dominant_wavelength(p) for p in xyz])
    com = np.array([ot.color.complementary_wavelength(p) for p in xyz])
    assert_close(dom, g[f"wavelengths/{name}/dominant"], **TOL, what=f"{name} dominant")
    assert_close(com, g[f"wavelengths/{name}/complementary"], **TOL, what=f"{name} complementary")
    assert np.nanmax(dom) > 699 or name == "ring"


def test_resolution_argument(g):
    p = g["wavelengths/ring/xyz"][100]
    coarse, fine = ot.color.dominant_wavelength(p, res=50), ot.color.dominant_wavelength(p)
    assert abs(coarse - fine) < 2 and coarse != fine


def test_light_spectrum_figures(g):
    for name, spec in cc.light_spectra(ot).items():
        assert_close(spec.xyz(), g[f"light/{name}/xyz"], **TOL, what=f"{name} xyz")
        if name in cc.NO_WAVELENGTHS:
            assert f"light/{name}/dominant" not in g.files
            continue
        assert_close(spec.dominant_wavelength(), g[f"light/{name}/dominant"], **TOL, what=f"{name} dominant")
        assert_close(spec.complementary_wavelength(), g[f"light/{name}/complementary"], **TOL, what=f"{name} complementary")
    assert abs(float(g["light/mono550/dominant"]) - 549.999772) < 1e-6 and np.isnan(g["light/mono550/complementary"])
    assert np.isnan(g["light/lines_purple/dominant"]) and abs(float(g["light/lines_purple/complementary"]) - 550.954645) < 1e-6


def test_transmission_spectrum_xyz(g):
    for name, spec in cc.transmission_spectra(ot).items():
        assert_close(spec.xyz(), g[f"transmission/{name}/xyz"], **TOL, what=f"{name} xyz")


def test_signatures_are_the_references():
    import inspect
    sig = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if k != "self"}  # noqa: E731
    E = inspect.Parameter.empty
    assert sig(ot.LightSpectrum.color) == dict(rendering_intent="Ignore", clip=False, L_th=0.0, chroma_scale=0.0)
    assert sig(ot.TransmissionSpectrum.color) == dict(rendering_intent="Absolute", clip=True, L_th=0, chroma_scale=None)
    assert sig(ot.color.xyz_to_srgb) == dict(xyz=E, normalize=True, clip=True, rendering_intent="Absolute", L_th=0, chroma_scale=None)
    assert sig(ot.color.xyz_to_srgb_linear) == dict(xyz=E, normalize=True, rendering_intent="Absolute", L_th=0., chroma_scale=None)
    assert sig(ot.color.get_chroma_scale) == dict(Luv=E, L_th=0.0, return_full=False)
    assert sig(ot.color.xyz_to_luv) == dict(xyz=E, normalize=True)
    assert sig(ot.color.dominant_wavelength) == dict(XYZ_s=E, res=10000)
    assert sig(ot.color.xyz_from_spectrum) == dict(wl=E, spec=E, method="sum")


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is present: the conversions run")
def test_no_fallback_without_a_device():
    with pytest.raises(ot.BackendError):
        ot.color.xyz_to_srgb(np.zeros((1, 1, 3)))
    with pytest.raises(ot.BackendError):
        ot.LightSpectrum("Monochromatic", wl=550).color()
    with pytest.raises(ot.BackendError):
        ot.TransmissionSpectrum("Constant", val=0.5).color()
    with pytest.raises(ot.BackendError):
        ot.color.spectral_colormap(np.array([500.0]))


# ---- the fixture itself ---------------------------------------------------------------------------------------------
def test_fixture_inputs_are_rebuilt_bit_for_bit(g):
    cases = cc.xyz_cases()
    assert sum(c.shape[0] * c.shape[1] for c in cases.values()) <= 1500
    for name, xyz in cases.items():
        assert g[f"{name}/xyz"].shape == xyz.shape and g[f"{name}/xyz"].tobytes() == xyz.tobytes(), name
    for name, wl in cc.colormap_wavelengths().items():
        assert g[f"colormap/{name}/wl"].tobytes() == wl.tobytes() and g[f"colormap/{name}/rgba"].shape == (wl.shape[0], 4)
    assert [v.shape[0] for v in cc.colormap_wavelengths().values()] == [401, 601, 5, 1]
    assert g["wavelengths/ring/xyz"].tobytes() == cc.hue_ring().tobytes()
    spectral = cases["spectral"].reshape(-1, 3)
    assert g["wavelengths/spectral/xyz"].tobytes() == spectral[np.any(spectral != 0, axis=1)].tobytes()
    for name, img in cc.log_extra_images().items():
        assert g[f"log_extra/{name}/in"].tobytes() == img.tobytes()


def test_fixture_drop_shares_and_records(g):
    keys = ["xyz_to_xyY", "xyY_to_xyz", "xyz_to_luv", "xyz_to_luv|nonorm", "luv_to_xyz", "luv_to_u_v_l", "luv_hue", "luv_chroma",
            "luv_saturation", "xyz_to_srgb", "xyz_to_srgb|Perceptual", "srgb_to_xyz", "srgb_linear_to_xyz", "outside_srgb_gamut",
            "log_srgb|Absolute", "log_srgb|Perceptual", "get_chroma_scale|full"] + [k for k, _ in cc.linear_keys()]
    assert len(cc.linear_keys()) == 10
    for name, xyz in cc.xyz_cases().items():
        lit = np.count_nonzero(np.any(xyz != 0, axis=2))
        for key in keys:
            val, keep = g[f"{name}/{key}"], g[f"{name}/{key}/keep"]
            assert val.shape[:2] == xyz.shape[:2] and keep.shape == xyz.shape[:2] and keep.dtype == bool, (name, key)
            assert np.count_nonzero(~keep) <= 0.01 * lit, f"{name} {key}: {np.count_nonzero(~keep)} of {lit} lit pixels dropped"
            assert not np.any(np.isnan(val.astype(np.float64))), (name, key)
        assert g[f"{name}/outside_srgb_gamut"].dtype == bool
        for L_th in cc.L_THS:
            assert 0.32 <= float(g[f"{name}/get_chroma_scale|Lth{L_th:g}"]) <= 1
    assert g["spectral/outside_srgb_gamut"].any() and not g["in_gamut/outside_srgb_gamut"].any()
    assert float(g["dim_outlier/get_chroma_scale|Lth0"]) == 0.32 and float(g["dim_outlier/get_chroma_scale|Lth1"]) == 1
    assert 0.32 < float(g["spectral/get_chroma_scale|Lth0"]) < 1


def test_fixture_log_srgb_and_hue_ring(g):
    # both early returns: one lightness only, nothing positive; and they occur among the cases too (1 x 1, all dark)
    for name in ("uniform", "black"):
        assert g[f"log_extra/{name}/out"].tobytes() == g[f"log_extra/{name}/in"].tobytes()
    assert np.any(g["log_extra/uniform/in"] > 0) and not np.any(g["log_extra/black/in"])
    assert np.array_equal(g["px1_spectral/log_srgb|Absolute"], g["px1_spectral/xyz_to_srgb"])
    assert np.abs(g["spectral/log_srgb|Absolute"] - g["spectral/xyz_to_srgb"]).max() > 0.1  # and the scaling itself
    for which in ("dominant", "complementary"):
        ring = g[f"wavelengths/ring/{which}"]
        assert ring.shape == (360,) and np.isnan(ring).any() and np.isfinite(ring).any(), which
    assert len(cc.light_spectra(ot)) == 13 and len(cc.transmission_spectra(ot)) == 3
    assert abs(g["transmission/gaussian550/color|default"] - np.array([0.50164, 1.0, 0.0, 0.76720])).max() < 1e-5
