"""Huygens point spread function: the diffraction image of a point, summed on the device from the optical paths of a traced
bundle to the reference sphere of the wavefront analysis.

`Raytracer.huygens_psf` has no counterpart in optrace.  Every used ray sends one spherical wavelet from its place on the sphere,
with the phase of its optical path, and the wavelets are added coherently at the points of an image plane around the focus.
Definition: DESIGN.md, "Huygens PSF".  Kernels: csrc/ot_psf.hpp behind `ot_psf_rays` and `ot_psf_sum`; the paths and their mean
come from `ot_wavefront_paths` and `ot_wavefront_moments` (wavefront.py).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from . import wavefront as _wavefront
from ._warn import warning
from .base import BaseClass, check_type, check_not_below, check_not_above
from .image import GrayscaleImage, srgb_linear_to_srgb


def check_arguments(nt: int, section, focus, radius, n_px, size, dz):
    """Argument checks of `Raytracer.huygens_psf`, host only; nt: sections per ray of the geometry.
    -> (focus as a float64 array or None, radius, size as floats or None, dz as a float)."""
    check_type("n_px", n_px, int)
    check_not_below("n_px", n_px, 1)
    check_not_above("n_px", n_px, _capi.PSF_MAX_PX)
    if size is not None:
        size = _wavefront._finite_number("size", size, positive=True)
    dz = _wavefront._finite_number("dz", dz)
    focus, radius = _wavefront.check_sphere_arguments(nt, section, focus, radius)
    return focus, radius, size, dz


class HuygensPSF(BaseClass):
    """Result of `Raytracer.huygens_psf`; lengths in mm.

    N, power: rays used (weight > 0 in the section, met by the reference sphere) and their summed weight.  n_missed: rays alive in
    the section whose line does not meet the sphere.  section, focus (3), radius: as for `WavefrontAnalysis`.  wavelength:
    power-weighted mean, nm.  size, dz: side length of the square of image points about the focus and its distance from the
    focus along z.  intensity: (n_px, n_px), row index y, column index x, |U|^2 / (sum a)^2 with a = sqrt(weight): 1 at the focus
    of a perfect wave.  strehl: the same figure exactly on the axis, at focus + (0, 0, dz), where with an even n_px no pixel
    centre lies.  noise_floor: sum a^2 / (sum a)^2, the background that a sum over randomly placed rays carries everywhere
    (1 / N for equal weights): the reason to trace many rays.  peak: largest value of `intensity`.  Without a usable ray
    N = power = 0, `intensity` is all NaN and every other figure NaN."""

    _tracked = False

    def __init__(self, N: int, power: float, n_missed: int, section: int, focus, radius: float, wavelength: float, size: float,
                 dz: float, intensity, strehl: float, noise_floor: float, **kwargs) -> None:
        super().__init__(**kwargs)
        self.N = int(N)
        self.power = float(power)
        self.n_missed = int(n_missed)
        self.section = int(section)
        self.focus = np.array(focus, dtype=np.float64)
        self.radius = float(radius)
        self.wavelength = float(wavelength)
        self.size = float(size)
        self.dz = float(dz)
        self.intensity = np.array(intensity, dtype=np.float64)
        self.strehl = float(strehl)
        self.noise_floor = float(noise_floor)
        self.peak = float(self.intensity.max()) if self.N else np.nan
        self.lock()

    def to_image(self) -> GrayscaleImage:
        """`intensity / peak` as a grayscale image with side lengths [size, size], which `convolve` takes as its `psf`.  The
        values of a `GrayscaleImage` carry the sRGB gamma, as those of the preset PSFs do: `convolve` removes it and works on the
        intensity itself."""
        if not self.peak > 0:
            raise RuntimeError("No usable ray: there is no image of this point spread function.")
        return GrayscaleImage(srgb_linear_to_srgb(self.intensity / self.peak), s=[self.size, self.size], quantity="Intensity",
                              long_desc=self.long_desc)


def _empty(section: int, focus, radius, n_px: int, size, dz: float, n_missed: int = 0, **kwargs) -> HuygensPSF:
    """(the rule of `wavefront._empty`: what the caller fixed stays)"""
    nan = np.nan
    return HuygensPSF(0, 0.0, n_missed, section, np.full(3, nan) if focus is None else focus, nan if radius is None else radius, nan,
                      nan if size is None else size, dz, np.full((n_px, n_px), nan), nan, nan, **kwargs)


def default_size(moments) -> float:
    """10 lambda_mean / pupil_radius from the moments record (float64): in air about 8 Airy diameters."""
    m = np.asarray(moments, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10 * (m[5] / m[0] * 1e-6) / m[10])


def figures(field, centre):
    """(intensity (n_px, n_px), strehl, noise_floor) from what `ot_psf_sum` returns: field (2, n_px, n_px), centre (4)."""
    A2 = centre[2] * centre[2]
    return (field[0] ** 2 + field[1] ** 2) / A2, (centre[0] ** 2 + centre[1] ** 2) / A2, centre[3] / A2


def analyse(rays, first: int, count: int, section: int, origin, focus, radius, n_px: int, size, dz: float, **kwargs) -> HuygensPSF:
    """The point spread function of the rays [first, first + count) of the storage `rays` behind section `section`.  origin: a
    point near the section's start that the device subtracts before it sums positions; the other arguments as `check_arguments`
    returned them.  The host reads the focus sums (where focus or radius is left to it), the moments record (where size is) and,
    at the end, one buffer with everything else."""
    import torch
    from ._device import ptr, stream_ptr
    lib = _capi.load_library()
    parts = [2 * n_px * n_px, 4, 2]  # field | centre | wl range
    S = _wavefront.sphere_stage(rays, first, count, section, origin, focus, radius, sum(parts))
    focus, radius = S.focus, S.radius
    if S.empty:
        return _empty(section, focus, radius, n_px, size, dz, **kwargs)
    st = stream_ptr()
    field, centre, wl_range = S.extra.split(parts)
    # (for the warning alone: the range of the used rays' wavelengths)
    used = S.w > 0
    wl_range[0] = torch.where(used, S.wl, torch.inf).amin()
    wl_range[1] = torch.where(used, S.wl, -torch.inf).amax()
    if size is None:
        m = S.mom.cpu().numpy()
        if not m[0] > 0:
            return _empty(section, focus, radius, n_px, size, dz, int(S.missed.cpu()[0]), **kwargs)
        size = default_size(m)
        if not (np.isfinite(size) and size > 0):
            raise RuntimeError("The used rays meet the reference sphere in one place, which gives the image no scale: pass `size`.")
    rec = torch.empty(_capi.PSF_REC * count, dtype=torch.float64, device=S.w.device)
    _capi.check(lib.ot_psf_rays(C.byref(S.R), first, count, section, (C.c_double * 3)(*focus), radius, ptr(S.opl), ptr(S.mom),
                                ptr(rec), st))
    psf_ws = torch.empty(_capi.psf_ws(count, n_px), dtype=torch.float64, device=S.w.device)
    _capi.check(lib.ot_psf_sum(count, ptr(rec), radius, n_px, size, dz, ptr(psf_ws), ptr(field), ptr(centre), st))
    m, n_missed, h = S.read()
    W = m[0]
    if not W > 0:
        return _empty(section, focus, radius, n_px, size, dz, n_missed, **kwargs)
    field, centre, wl_range = np.split(h, np.cumsum(parts)[:-1])
    if wl_range[0] != wl_range[1]:
        warning(f"The used rays carry wavelengths from {wl_range[0]:.6g} nm to {wl_range[1]:.6g} nm and are added coherently, each "
                "with its own: the point spread function is meaningful for a monochromatic source only.")
    intensity, strehl, noise_floor = figures(field.reshape(2, n_px, n_px), centre)
    return HuygensPSF(int(m[1]), W, n_missed, section, focus, radius, m[5] / W, size, dz, intensity, strehl, noise_floor, **kwargs)
