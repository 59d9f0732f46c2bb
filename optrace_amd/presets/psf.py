"""Point spread function presets for `convolve()` (presets/psf.py): grayscale images with the sRGB gamma, side lengths in
mm from parameters in micrometres.  Host NumPy: the largest has 801 x 801 pixels and `GrayscaleImage` holds host data."""
from __future__ import annotations

import numpy as np

from ..base import check_above, check_not_above, check_not_below
from ..image import GrayscaleImage, srgb_linear_to_srgb

#: first and third zero of the Bessel function J1
_J1_ZERO1, _J1_ZERO3 = 3.8317, 10.1735


def _grid(half: float, n: int):
    """(Y, X) of n x n samples over [-half, half] in both directions."""
    return np.mgrid[-half:half:n * 1j, -half:half:n * 1j]


def _image(linear: np.ndarray, side_um: float) -> GrayscaleImage:
    return GrayscaleImage(srgb_linear_to_srgb(linear), [side_um / 1000, side_um / 1000])


def circle(d: float = 1.0) -> GrayscaleImage:
    """Disc of diameter `d` [um] on a frame 5 % larger, with a three-step edge; 601 px."""
    check_above("d", d, 0)
    half, n = 1.05 / 2, 601
    Y, X = _grid(half, n)
    R2 = X ** 2 + Y ** 2
    Z = np.zeros((n, n), dtype=np.float64)
    step = half / n
    for radius, level in ((0.5 + step, 0.25), (0.5, 0.75), (0.5 - step, 1.0)):
        Z[R2 <= radius ** 2] = level
    return _image(Z, 2 * half * d)


def gaussian(sig: float = 0.5) -> GrayscaleImage:
    """Gaussian with standard deviation `sig` [um], out to five sigma; 401 px."""
    check_above("sig", sig, 0)
    half = 5 * sig
    Y, X = _grid(half, 401)
    return _image(np.exp(-(X ** 2 + Y ** 2) / 2 / sig ** 2), 2 * half)


def airy(r: float = 1.0) -> GrayscaleImage:
    """Airy pattern with resolution limit `r` [um] (radius of the first dark ring), cut after the third zero; 401 px."""
    from scipy.special import j1
    check_above("r", r, 0)
    half, n = _J1_ZERO3 / _J1_ZERO1, 401
    Y, X = _grid(half, n)
    R = np.sqrt(X ** 2 + Y ** 2) * _J1_ZERO1
    Z = np.ones((n, n), dtype=np.float64)
    off_centre = R != 0
    Z[off_centre] = (2 * j1(R[off_centre]) / R[off_centre]) ** 2
    Z[R > _J1_ZERO3] = 0
    return _image(Z, 2 * half * r)


def glare(sig1: float = 0.5, sig2: float = 3.0, a: float = 0.15) -> GrayscaleImage:
    """Focus (Gaussian, `sig1` um) plus a wider glare (Gaussian, `sig2` um) of relative amplitude `a`; 801 px."""
    check_above("sig1", sig1, 0)
    check_above("sig2", sig2, 0)
    check_not_below("a", a, 0)
    check_not_above("a", a, 1)
    if sig2 <= sig1:
        raise ValueError("sig2 must be larger than sig1.")
    half = 5 * sig2
    Y, X = _grid(half, 801)
    R2 = X ** 2 + Y ** 2
    Z = a * np.exp(-R2 / 2 / sig2 ** 2) + (1 - a) * np.exp(-R2 / 2 / sig1 ** 2)
    Z /= Z.max()
    return _image(Z, 2 * half)


def halo(sig1: float = 0.5, sig2: float = 0.25, r: float = 4.0, a: float = 0.3) -> GrayscaleImage:
    """Focus (Gaussian, `sig1` um) plus a ring at radius `r` um (Gaussian profile, `sig2` um) of relative brightness `a`;
    801 px."""
    check_above("sig1", sig1, 0)
    check_above("sig2", sig2, 0)
    check_not_below("a", a, 0)
    check_not_above("a", a, 1)
    check_not_below("r", r, 0)
    half = r + 5 * sig2
    Y, X = _grid(half, 801)
    R = np.sqrt(X ** 2 + Y ** 2)
    Z = np.exp(-R ** 2 / 2 / sig1 ** 2) + a * np.exp(-(R - r) ** 2 / 2 / sig2 ** 2)
    Z /= Z.max()
    return _image(Z, 2 * half)
