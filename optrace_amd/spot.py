"""Spot analysis: the figures of a traced bundle on a detector, reduced on the device from the hit list.

`Raytracer.spot_analysis` has no counterpart in optrace, where these numbers are formed in NumPy from `rays.p_list`;
here that would bring the whole ray storage to the host.  Kernels: csrc/ot_spot.hpp behind `ot_spot_*`.
"""
from __future__ import annotations

import numpy as np

from . import _capi
from .base import BaseClass, check_type, check_not_below, check_not_above

N_DEFAULT_FREQUENCIES = 65


def check_arguments(n_radii, frequencies):
    """Argument checks of `Raytracer.spot_analysis`, host only.  -> frequencies as a float64 array, or None."""
    check_type("n_radii", n_radii, int)
    check_not_below("n_radii", n_radii, 1)
    check_not_above("n_radii", n_radii, _capi.SPOT_MAX_RADII)
    if frequencies is None:
        return None
    check_type("frequencies", frequencies, (list, tuple, np.ndarray))
    freq = np.asarray(frequencies)
    if freq.size and not (np.issubdtype(freq.dtype, np.floating) or np.issubdtype(freq.dtype, np.integer)):
        raise TypeError(f"Property 'frequencies' needs to hold real numbers, but holds {freq.dtype}.")
    freq = np.array(freq, dtype=np.float64)
    if freq.ndim != 1:
        raise ValueError(f"Property 'frequencies' needs to be one-dimensional, but has {freq.ndim} dimensions.")
    check_not_above("len(frequencies)", freq.shape[0], _capi.SPOT_MAX_FREQ)
    if not np.all(np.isfinite(freq)):
        raise ValueError("Property 'frequencies' needs to hold finite values only.")
    return freq


class SpotAnalysis(BaseClass):
    """Result of `Raytracer.spot_analysis`; positions and radii in the detector's (or its projection's) length unit.

    N, power: number of hits (weight > 0) and their summed power.  centroid: power-weighted mean position (2).
    rms_x, rms_y, rms_radius, cov_xy: second moments about the centroid.  max_radius: largest distance of a hit from it.
    ee_radii, ee: n_radii + 1 equal-width radii over [0, max_radius] and the fraction of power inside each.
    frequencies (cycles per length unit), otf_x, otf_y (complex), mtf_x, mtf_y: geometric transfer function about the
    centroid, sum w exp(-2 pi i nu d) / sum w along each axis.  extent: extent of the hits, [x0, x1, y0, y1].
    Without a hit N = power = 0, ee is zero and every other figure NaN."""

    _tracked = False

    def __init__(self, N: int, power: float, centroid, rms_x: float, rms_y: float, cov_xy: float, max_radius: float,
                 extent, ee, frequencies, otf_x, otf_y, **kwargs) -> None:
        super().__init__(**kwargs)
        self.N = int(N)
        self.power = float(power)
        self.centroid = np.array(centroid, dtype=np.float64)
        self.rms_x, self.rms_y = float(rms_x), float(rms_y)
        self.rms_radius = float(np.sqrt(self.rms_x ** 2 + self.rms_y ** 2))
        self.cov_xy = float(cov_xy)
        self.max_radius = float(max_radius)
        self.extent = np.array(extent, dtype=np.float64)
        self.ee = np.array(ee, dtype=np.float64)
        self.ee_radii = np.linspace(0, self.max_radius, self.ee.shape[0])
        self.frequencies = np.array(frequencies, dtype=np.float64)
        self.otf_x = np.array(otf_x, dtype=np.complex128)
        self.otf_y = np.array(otf_y, dtype=np.complex128)
        self.mtf_x, self.mtf_y = np.abs(self.otf_x), np.abs(self.otf_y)
        self.lock()

    def encircled_energy(self, r):
        """Fraction of the power within radius r of the centroid: `ee` interpolated linearly, 1 beyond `max_radius`."""
        r = np.asarray(r, dtype=np.float64)
        if not self.N:
            return np.zeros_like(r)[()]
        return np.interp(r, self.ee_radii, self.ee, left=0.0, right=1.0)[()]

    def radius_of(self, fraction):
        """Radius about the centroid that holds `fraction` of the power, 0 < fraction <= 1: the inverse of
        `encircled_energy`.  Where `ee` is flat the answer is the smallest such radius (the left edge of the step)."""
        f = np.asarray(fraction, dtype=np.float64)
        if np.any(~(f > 0)) or np.any(f > 1):
            raise ValueError(f"Property 'fraction' needs to be above 0 and at most 1, but is {fraction}.")
        if not self.N:
            return np.full(f.shape, np.nan)[()]
        # the segment (k - 1, k) with ee[k - 1] < f <= ee[k]: never a flat one
        k = np.searchsorted(self.ee, f, side="left")
        e0, e1 = self.ee[k - 1], self.ee[k]
        r0, r1 = self.ee_radii[k - 1], self.ee_radii[k]
        return (r0 + (f - e0) / (e1 - e0) * (r1 - r0))[()]


def _empty(extent, n_radii: int, freq, **kwargs) -> SpotAnalysis:
    nan = np.nan
    if freq is None:
        freq = np.linspace(0, 1, N_DEFAULT_FREQUENCIES)
    otf = np.full(freq.shape[0], complex(nan, nan))
    return SpotAnalysis(0, 0.0, (nan, nan), nan, nan, nan, nan, extent, np.zeros(n_radii + 1), freq, otf, otf, **kwargs)


def analyse(xy, w, n: int, fill, extent, n_radii: int, freq, **kwargs) -> SpotAnalysis:
    """Figures of a hit list of `Raytracer._hit_detectors`.  xy: flat f64 device tensor, x plane then y plane; w: f32 device
    tensor; n: rays of the bundle; fill: fill counts of a compact list (x, y, w then hold 1024 pieces) or None;
    freq: what `check_arguments` returned."""
    import torch
    from ._device import require_device, ptr, stream_ptr, to_dev
    lib = _capi.load_library()
    dev = require_device()
    if n < 1:
        return _empty(extent, n_radii, freq, **kwargs)
    cap = int(w.shape[0])  # entries per plane
    x, y = xy[:cap], xy[cap:2 * cap]
    K = N_DEFAULT_FREQUENCIES if freq is None else int(freq.shape[0])
    M = _capi.SPOT_M
    ws = torch.empty(_capi.spot_ws(K), dtype=torch.float64, device=dev)
    res = torch.zeros(M + n_radii + 4 * K, dtype=torch.float64, device=dev)  # moments | radial sums | OTF sums
    mom, hist, otf = res[:M], res[M:M + n_radii], res[M + n_radii:]
    st = stream_ptr()
    _capi.check(lib.ot_spot_moments(n, ptr(fill), ptr(x), ptr(y), ptr(w), ptr(ws), ptr(mom), st))
    _capi.check(lib.ot_spot_radial(n, ptr(fill), ptr(x), ptr(y), ptr(w), ptr(mom), n_radii, ptr(hist), st))

    def rms(m):
        W = m[0]
        return np.sqrt(m[4] / W), np.sqrt(m[5] / W)

    if freq is None:  # the default grid reaches to 1 / rms radius: the moments come back first
        m = mom.cpu().numpy()
        if not m[0] > 0:
            return _empty(extent, n_radii, None, **kwargs)
        rms_x, rms_y = rms(m) if m[3] > 1 else (0.0, 0.0)
        rms_radius = float(np.sqrt(rms_x ** 2 + rms_y ** 2))
        freq = np.linspace(0, 1 / rms_radius if rms_radius > 0 else 1, N_DEFAULT_FREQUENCIES)
    if K:
        d_freq = to_dev(freq, np.float64)
        _capi.check(lib.ot_spot_otf(n, ptr(fill), ptr(x), ptr(y), ptr(w), ptr(mom), ptr(d_freq), K, ptr(ws), ptr(otf), st))
    h = res.cpu().numpy()
    m, hist_h, otf_h = h[:M], h[M:M + n_radii], h[M + n_radii:].reshape(4, K)
    W = m[0]
    if not W > 0:
        return _empty(extent, n_radii, freq, **kwargs)
    if m[3] == 1:  # one hit is its own centroid: w x / w need not return x to the last bit, the figures say so exactly
        ee = np.concatenate(([0.0], np.ones(n_radii)))
        return SpotAnalysis(1, W, (m[1] / W, m[2] / W), 0.0, 0.0, 0.0, 0.0, extent, ee, freq, np.ones(K), np.ones(K), **kwargs)
    cum = np.concatenate(([0.0], np.cumsum(hist_h)))
    rms_x, rms_y = rms(m)
    return SpotAnalysis(int(m[3]), W, (m[1] / W, m[2] / W), rms_x, rms_y, m[6] / W, np.sqrt(m[7]), extent, cum / cum[-1],
                        freq, (otf_h[0] + 1j * otf_h[1]) / W, (otf_h[2] + 1j * otf_h[3]) / W, **kwargs)
