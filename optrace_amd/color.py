"""Colour conversions and colour figures: mirror of optrace/tracer/color (xyz.py, luv.py, srgb.py, observers.py, tools.py,
illuminants.py), every name but `random_wavelengths_from_srgb`: that one lives in `optrace_amd.random`
(`ot.random.random_wavelengths_from_srgb`), beside the samplers it is built from; the wavelengths of the pixels of an RGB
image source are drawn by the same arithmetic inside the generation kernel.

Two halves.  Tables and scalar figures (observers, illuminants, blackbody, `xyz_from_spectrum`, dominant and
complementary wavelength, the gamma curves of `image.py`) are NumPy on the host and need no GPU.  The per-pixel
conversions run on the device through `ot_color_convert` (csrc/ot_color.hpp), with the per-pixel arithmetic the image
stage behind `RenderImage.get` uses (csrc/ot_color_px.hpp): an (Ny, Nx, 3) array of any real dtype and any strides comes
back as a new float64 NumPy array; a float64 device tensor comes back as a device tensor, without crossing to the host.
Without a device these raise `BackendError`; there is no NumPy fallback.
"""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import torch

from . import _capi
from ._device import require_device, stream_ptr, ptr
from .options import global_options as go
from .spectrum import wavelengths, blackbody, normalized_blackbody, illuminant, _tables
from .image import (srgb_to_srgb_linear, srgb_linear_to_srgb, power_from_srgb_linear, srgb_r_primary, srgb_g_primary,
                    srgb_b_primary, SRGB_PRIMARY_POWER_FACTORS)

WP_D65_XYZ = [0.95047, 1.00000, 1.08883]   # xyz.py:10
WP_D65_XY = [0.31272, 0.32903]             # xyz.py:13
WP_D65_LUV = [100, 0.19783982, 0.4683363]  # luv.py:8
WP_D65_UV = WP_D65_LUV[1:]
SRGB_R_UV = [0.4507042254, 0.5228873239]   # luv.py:15-17
SRGB_G_UV = [0.125, 0.5625]
SRGB_B_UV = [0.1754385965, 0.1578947368]
SRGB_RENDERING_INTENTS = ["Ignore", "Absolute", "Perceptual"]  # srgb.py:13
SRGB_R_XY = [0.64, 0.33]                   # srgb.py:17-19
SRGB_G_XY = [0.30, 0.60]
SRGB_B_XY = [0.15, 0.06]

# ---- illuminants (illuminants.py): the tables of spectrum.py -------------------------------------------------------
_ILLUMINANTS = ["A", "C", "D50", "D55", "D65", "D75", "E", "F2", "F7", "F11", "LED_B1", "LED_B2", "LED_B3", "LED_B4",
                "LED_B5", "LED_BH1", "LED_RGB1", "LED_V1", "LED_V2"]
for _name in _ILLUMINANTS:
    globals()[f"{_name.lower()}_illuminant"] = illuminant(_name.replace("_", "-"))
from .spectrum import d65_illuminant  # noqa: E402,F811  (the object spectrum.py itself exports)


# ---- observers (observers.py:14-41) ---------------------------------------------------------------------------------
_observers = _tables["observers"]


def _observer(column: int, name: str):
    def f(wl: np.ndarray) -> np.ndarray:
        return np.interp(wl, _observers[:, 0], _observers[:, column], left=0, right=0)
    f.__name__ = f.__qualname__ = f"{name}_observer"
    f.__doc__ = f"CIE 1931 2 degree colorimetric standard observer {name}: linear between the table's 1 nm steps, zero outside."
    return f


x_observer, y_observer, z_observer = _observer(1, "x"), _observer(2, "y"), _observer(3, "z")


# ---- host figures (xyz.py:57-140) -----------------------------------------------------------------------------------
def xyz_from_spectrum(wl, spec, method="sum") -> np.ndarray:
    """Tristimulus values of a sampled spectrum; method "sum" or "trapz" (xyz.py:57-71)."""
    def integrate(y):
        return np.sum(y) if method == "sum" else np.sum((y[1:] + y[:-1]) / 2.0)
    return np.array([integrate(spec * x_observer(wl)), integrate(spec * y_observer(wl)), integrate(spec * z_observer(wl))])


def _wrap(phi):
    """Angles into [-pi/2, 3/2 pi), where the locus angle is (nearly) injective (xyz.py:95)."""
    return phi + 2 * np.pi if phi < -np.pi / 2 else phi


@functools.lru_cache(maxsize=4)
def _locus(res: int, wl_range: tuple):
    """Angles of the spectral locus around D65 in the xy diagram, sorted, with their wavelengths (xyz.py:86-98).  The
    angle runs backwards between about 699 and 780 nm; like scipy's interp1d the samples are sorted by angle (stable)."""
    wl = np.linspace(*wl_range, res)
    X, Y, Z = x_observer(wl), y_observer(wl), z_observer(wl)
    s = X + Y + Z
    lit = s > 0
    x = np.where(lit, X / np.where(lit, s, 1.0), WP_D65_XY[0])
    y = np.where(lit, Y / np.where(lit, s, 1.0), WP_D65_XY[1])
    phi = np.arctan2(y - WP_D65_XY[1], x - WP_D65_XY[0])
    phi[phi < -np.pi / 2] += 2 * np.pi
    order = np.argsort(phi, kind="mergesort")
    return phi[order], wl[order]


def _wavelength_at(phi_s: float, res: int) -> float:
    """Linear interpolation of the sorted locus at one angle; NaN outside of it (interp1d(bounds_error=False))."""
    phi, wl = _locus(int(res), tuple(float(v) for v in go.wavelength_range))
    if not phi[0] <= phi_s <= phi[-1]:
        return float("nan")
    hi = int(np.clip(np.searchsorted(phi, phi_s), 1, phi.shape[0] - 1))
    lo = hi - 1
    with np.errstate(all="ignore"):
        slope = (wl[hi] - wl[lo]) / (phi[hi] - phi[lo])
        return float(slope * (phi_s - phi[lo]) + wl[lo])


def _chrom_angle(XYZ_s) -> float:
    X, Y, Z = (float(v) for v in np.asarray(XYZ_s, dtype=np.float64).ravel()[:3])
    s = X + Y + Z
    x, y = (X / s, Y / s) if s > 0 else WP_D65_XY
    return _wrap(float(np.arctan2(y - WP_D65_XY[1], x - WP_D65_XY[0])))


def dominant_wavelength(XYZ_s: np.ndarray, res: int = 10000) -> float:
    """Wavelength with the hue of the colour XYZ_s seen from D65; NaN for purples (xyz.py:111-120)."""
    return _wavelength_at(_chrom_angle(XYZ_s), res)


def complementary_wavelength(XYZ_s: np.ndarray, res: int = 10000) -> float:
    """Wavelength with the opposite hue; NaN for greens (xyz.py:123-140)."""
    return _wavelength_at(_wrap(_chrom_angle(XYZ_s) - np.pi), res)


# ---- device conversions ---------------------------------------------------------------------------------------------
(_XYZ_TO_XYY, _XYY_TO_XYZ, _XYZ_TO_LUV, _LUV_TO_XYZ, _LUV_TO_UVL, _LUV_HUE, _LUV_CHROMA, _LUV_SATURATION,
 _SRGB_LINEAR_TO_XYZ, _SRGB_TO_XYZ, _XYZ_TO_SRGB_LINEAR, _XYZ_TO_SRGB, _OUTSIDE_GAMUT, _CHROMA_SCALE, _LOG_SRGB,
 _SPECTRAL_COLORMAP) = range(16)  # OT_COL_*
_NO_NORMALIZE, _NO_CLIP = 0x100, 0x200  # OT_IMG_FLAG_*
_INTENT = {"Ignore": 0, "Absolute": 0x1000, "Perceptual": 0x2000}  # OT_COL_INTENT_*


def _convert(op: int, arr, channels: int, L_th: float = 0.0, chroma_scale: float = None, full: bool = True):
    """One `ot_color_convert` call.  -> (result in the kind of `arr`: NumPy array or device tensor, the call's scalar)."""
    lib = _capi.load_library()
    dev = require_device()
    on_device = isinstance(arr, torch.Tensor)
    if on_device:
        src = arr.to(dev, torch.float64)
    else:  # float64 before any arithmetic; one contiguous copy, whatever the strides
        src = torch.from_numpy(np.ascontiguousarray(arr, dtype=np.float64)).to(dev)
    spectral = op == _SPECTRAL_COLORMAP
    if src.ndim != (1 if spectral else 3) or (not spectral and src.shape[2] != 3):
        raise ValueError("expected a wavelength vector" if spectral else "expected an image of shape (Ny, Nx, 3)")
    src = src.contiguous()
    lead = tuple(src.shape) if spectral else tuple(src.shape[:2])
    n = int(np.prod(lead))
    shape = lead + ((channels,) if channels > 1 else ())
    out = torch.empty(shape, dtype=torch.float64, device=dev) if full else None
    scalar = C.c_double(0.0)
    if n:
        cs = float("nan") if chroma_scale is None else float(chroma_scale)
        _capi.check(lib.ot_color_convert(ptr(src), n, op, float(L_th), cs, ptr(out), C.byref(scalar), stream_ptr()))
    if out is not None and not on_device:
        out = out.cpu().numpy()
    return out, scalar.value


def _intent(rendering_intent: str) -> int:
    if rendering_intent not in _INTENT:
        raise ValueError(f"rendering_intent needs to be one of {SRGB_RENDERING_INTENTS}, but is '{rendering_intent}'.")
    return _INTENT[rendering_intent]


def xyz_to_xyY(xyz):
    """XYZ -> xyY; black becomes the whitepoint with Y = 0 (xyz.py:17-35)."""
    return _convert(_XYZ_TO_XYY, xyz, 3)[0]


def xyY_to_xyz(xyy):
    """xyY -> XYZ (xyz.py:38-54)."""
    return _convert(_XYY_TO_XYZ, xyy, 3)[0]


def xyz_to_luv(xyz, normalize: bool = True):
    """XYZ -> CIELUV, normalised by the highest Y of the image if `normalize` (luv.py:20-71)."""
    return _convert(_XYZ_TO_LUV | (0 if normalize else _NO_NORMALIZE), xyz, 3)[0]


def luv_to_xyz(luv):
    """CIELUV -> XYZ (luv.py:74-109)."""
    return _convert(_LUV_TO_XYZ, luv, 3)[0]


def luv_to_u_v_l(luv):
    """CIELUV -> u'v'L chromaticities (luv.py:112-127)."""
    return _convert(_LUV_TO_UVL, luv, 3)[0]


def luv_saturation(luv):
    """Saturation image (Ny, Nx) of CIELUV values (luv.py:130-143)."""
    return _convert(_LUV_SATURATION, luv, 1)[0]


def luv_chroma(luv):
    """Chroma image (Ny, Nx) of CIELUV values (luv.py:146-153)."""
    return _convert(_LUV_CHROMA, luv, 1)[0]


def luv_hue(luv):
    """Hue image (Ny, Nx) in degrees, 0 to 360, of CIELUV values (luv.py:156-165)."""
    return _convert(_LUV_HUE, luv, 1)[0]


def srgb_linear_to_xyz(rgbl):
    """Linear sRGB -> XYZ (srgb.py:50-68)."""
    return _convert(_SRGB_LINEAR_TO_XYZ, rgbl, 3)[0]


def srgb_to_xyz(rgb):
    """sRGB -> XYZ (srgb.py:71-81)."""
    return _convert(_SRGB_TO_XYZ, rgb, 3)[0]


def xyz_to_srgb_linear(xyz, normalize: bool = True, rendering_intent: str = "Absolute", L_th: float = 0.,
                       chroma_scale: float = None):
    """XYZ -> linear sRGB with a rendering intent (srgb.py:267-354)."""
    op = _XYZ_TO_SRGB_LINEAR | _intent(rendering_intent) | (0 if normalize else _NO_NORMALIZE)
    return _convert(op, xyz, 3, L_th, chroma_scale)[0]


def xyz_to_srgb(xyz, normalize: bool = True, clip: bool = True, rendering_intent: str = "Absolute", L_th: float = 0,
                chroma_scale: float = None):
    """XYZ -> sRGB: `xyz_to_srgb_linear`, clipped to [0, 1] if `clip`, gamma-corrected (srgb.py:379-407)."""
    op = _XYZ_TO_SRGB | _intent(rendering_intent) | (0 if normalize else _NO_NORMALIZE) | (0 if clip else _NO_CLIP)
    return _convert(op, xyz, 3, L_th, chroma_scale)[0]


def outside_srgb_gamut(xyz):
    """Boolean image (Ny, Nx): the colour has no sRGB representation (srgb.py:84-92)."""
    return _convert(_OUTSIDE_GAMUT, xyz, 1)[0] != 0


def get_chroma_scale(Luv, L_th=0.0, return_full: bool = False):
    """Chroma factor that brings every valid colour above L_th * max(L) into the sRGB gamut, in [0.32, 1]; with
    `return_full` also the factor of every pixel (srgb.py:242-264)."""
    full, fact = _convert(_CHROMA_SCALE, Luv, 1, L_th, full=return_full)
    empty = not np.prod(Luv.shape[:2])
    return (1.0 if empty else fact, full) if return_full else (1.0 if empty else fact)


def log_srgb(img):
    """sRGB image with logarithmically scaled lightness at unchanged chromaticities (srgb.py:410-444)."""
    return _convert(_LOG_SRGB, img, 3)[0]


def spectral_colormap(wl):
    """(N, 4) sRGB colours and alpha = 1 for the wavelengths `wl` (srgb.py:569-606).  Both rendering intents run over the
    whole array as one image, so the colours depend on all of `wl`."""
    return _convert(_SPECTRAL_COLORMAP, wl, 4)[0]
