"""Inputs of the colour fixture (tests/golden/color.npz) beyond the images of tests/image_convert_cases.py, shared by the
generator (tests/golden/generate_golden_color.py, which runs them through the reference) and by tests/test_color_host.py and
tests/test_gpu_color.py (which run them through optrace_amd).  Plain NumPy; the spectra are built from whichever package is
handed in, the reference or optrace_amd, through the constructor arguments both share.
"""
import numpy as np

from image_convert_cases import image_convert_cases, PERCEPTUAL_VARIANTS, D65_XY

INTENTS = ["Ignore", "Absolute", "Perceptual"]
L_THS = [kw.get("L_th", 0.0) for kw in PERCEPTUAL_VARIANTS.values() if "chroma_scale" not in kw]  # 0, 0.02, 0.05, 1


def xyz_cases() -> dict:
    """name -> (Ny, Nx, 3) contiguous XYZ image of the nine cases of image_convert_cases()."""
    return {name: np.ascontiguousarray(v[:, :, :3]) for name, v in image_convert_cases().items()}


def linear_keys() -> list:
    """(key, kwargs) of every recorded color.xyz_to_srgb_linear variant."""
    out = []
    for intent in INTENTS:
        for normalize in (True, False):
            out.append((f"xyz_to_srgb_linear|{intent}" + ("" if normalize else "|nonorm"),
                        dict(rendering_intent=intent, normalize=normalize)))
    for tag, kw in PERCEPTUAL_VARIANTS.items():
        if tag:
            out.append((f"xyz_to_srgb_linear|Perceptual{tag}", dict(rendering_intent="Perceptual", **kw)))
    return out


def log_extra_images() -> dict:
    """The two early returns of log_srgb: one lightness only, nothing positive."""
    return {"uniform": np.full((3, 4, 3), 0.4) * np.array([1.0, 0.5, 0.25]), "black": np.zeros((3, 4, 3))}


def colormap_wavelengths() -> dict:
    grid = np.linspace(380.0, 780.0, 401)
    extra = np.random.default_rng(20261018).uniform(380.0, 780.0, 200)
    return {"grid401": grid, "grid401_random200": np.concatenate([grid, extra]),
            "five": np.array([420.0, 505.5, 550.0, 610.25, 700.0]), "one": np.array([532.0])}


def observer_wavelengths() -> np.ndarray:
    """64 wavelengths: both ends of the table, two outside of it, table points and points between them."""
    inner = np.random.default_rng(20261019).uniform(360.0, 830.0, 52)
    return np.concatenate([[359.0, 360.0, 360.5, 380.0, 555.0, 555.5, 780.0, 829.5, 830.0, 830.001, 900.0, 400.25], inner])


def spectrum_samples() -> tuple:
    """(wl, spec) for xyz_from_spectrum: a skewed bump on 500 samples, cut off at both ends (where sum and trapz differ)."""
    wl = np.linspace(500.0, 640.0, 500)
    return wl, np.exp(-((wl - 560.0) / 45.0) ** 2) * (1 + 0.3 * np.sin(wl / 17.0))


def hue_ring() -> np.ndarray:
    """(360, 3) XYZ colours at 1 degree steps on a circle of radius 0.05 around D65 in the xy diagram, Y = 0.5."""
    a = np.deg2rad(np.arange(360.0))
    x, y = D65_XY[0] + 0.05 * np.cos(a), D65_XY[1] + 0.05 * np.sin(a)
    Y = np.full(360, 0.5)
    return np.stack([x / y * Y, Y, (1 - x - y) / y * Y], axis=1)


def _bump(wl):
    return 0.2 + np.sin(wl / 40.0) ** 2


def light_spectra(ot) -> dict:
    """The thirteen light spectra, built from package `ot`."""
    LS = ot.LightSpectrum
    wls = np.linspace(400.0, 700.0, 31)
    hist = LS("Histogram")
    hist._wls = np.linspace(420.0, 620.0, 11)
    hist._vals = np.linspace(0.1, 1.0, 10)
    return {
        "mono550": LS("Monochromatic", wl=550.0),
        "mono450": LS("Monochromatic", wl=450.0),
        "lines_FdC": LS("Lines", lines=[486.13, 587.56, 656.27], line_vals=[1.0, 1.0, 1.0]),
        "lines_purple": LS("Lines", lines=[440.0, 650.0], line_vals=[1.0, 2.0]),
        "blackbody3000": LS("Blackbody", T=3000.0),
        "blackbody5500": LS("Blackbody", T=5500.0),
        "gaussian480": LS("Gaussian", mu=480.0, sig=20.0),
        "rectangle600_680": LS("Rectangle", wl0=600.0, wl1=680.0),
        "constant": LS("Constant"),
        "data520": LS("Data", wls=wls, vals=np.exp(-(wls - 520.0) ** 2 / (2 * 30.0 ** 2))),
        "histogram": hist,
        "function": LS("Function", func=_bump),
        "d65": ot.presets.light_spectrum.d65,
    }


NO_WAVELENGTHS = ("d65",)  # on the whitepoint: the hue angle, and with it both wavelengths, is rounding noise

# argument sets of LightSpectrum.color: tag -> kwargs
LIGHT_COLOR_ARGS = {f"{intent}|{'clip' if clip else 'noclip'}": dict(rendering_intent=intent, clip=clip)
                    for intent in INTENTS for clip in (False, True)}


def transmission_spectra(ot) -> dict:
    TS = ot.TransmissionSpectrum
    return {"gaussian550": TS("Gaussian", mu=550.0, sig=30.0, val=0.8),
            "rectangle450_520": TS("Rectangle", wl0=450.0, wl1=520.0),
            "constant0.5": TS("Constant", val=0.5)}


# argument sets of TransmissionSpectrum.color: its own defaults, those of LightSpectrum.color, the Perceptual intent
TRANSMISSION_COLOR_ARGS = {"default": {}, "light_default": dict(rendering_intent="Ignore", clip=False, L_th=0.0, chroma_scale=0.0),
                           "Perceptual": dict(rendering_intent="Perceptual")}
