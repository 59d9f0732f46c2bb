"""Wavefront analysis: optical path difference of a traced bundle against a reference sphere, its RMS and peak-to-valley, a Zernike
decomposition and a pupil map, reduced on the device from the ray storage.

`Raytracer.wavefront_analysis` has no counterpart in optrace, where these numbers would be formed in NumPy from
`rays.optical_lengths()`; here that would bring whole position and index planes to the host.  Definition: DESIGN.md, "Wavefront
analysis".  Kernels: csrc/ot_wavefront.hpp behind `ot_wavefront_*`.
"""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _capi
from ._warn import warning
from .base import BaseClass, check_type, check_not_below, check_not_above


def noll_indices(j: int) -> tuple:
    """Radial order n and signed azimuthal order m of Noll's Z_j (j from 1): within an order |m| rises, and an even j carries
    the cosine term (m >= 0), an odd one the sine term (m < 0)."""
    n = 0
    while (n + 1) * (n + 2) // 2 < j:
        n += 1
    p = j - n * (n + 1) // 2 - 1  # position within the order
    m = 2 * (p // 2) + 1 if n % 2 else 2 * ((p + 1) // 2)
    return n, (m if j % 2 == 0 else -m)


def zernike(j: int, x, y):
    """Noll's orthonormal Zernike polynomial Z_j, 1 <= j <= 36, at the points (x, y) of the unit disc:
    Z_j = sqrt(n + 1) R_n^0(rho) for m = 0, otherwise sqrt(2 (n + 1)) R_n^|m|(rho) times cos(m theta) for even j and
    sin(|m| theta) for odd j, with R_n^m(rho) = sum_k (-1)^k (n - k)! / (k! ((n + m) / 2 - k)! ((n - m) / 2 - k)!) rho^(n - 2 k).
    The integral of Z_i Z_j over the disc is pi for i = j and 0 otherwise."""
    check_type("j", j, int)
    check_not_below("j", j, 1)
    check_not_above("j", j, _capi.WF_MAX_J)
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n, m = noll_indices(j)
    ma = abs(m)
    rho, theta = np.hypot(x, y), np.arctan2(y, x)
    f = math.factorial
    radial = sum((-1) ** k * f(n - k) / (f(k) * f((n + ma) // 2 - k) * f((n - ma) // 2 - k)) * rho ** (n - 2 * k)
                 for k in range((n - ma) // 2 + 1))
    if m == 0:
        return math.sqrt(n + 1) * radial
    return math.sqrt(2 * (n + 1)) * radial * (np.cos(ma * theta) if m > 0 else np.sin(ma * theta))


def _finite_number(key: str, val, nonzero: bool = False, positive: bool = False) -> float:
    check_type(key, val, (int, float, np.integer, np.floating))
    if not np.isfinite(val):
        raise ValueError(f"Property '{key}' needs to be finite, but is {val}.")
    if (nonzero and val == 0) or (positive and not val > 0):
        raise ValueError(f"Property '{key}' needs to be {'above zero' if positive else 'non-zero'}, but is {val}.")
    return float(val)


def check_sphere_arguments(nt: int, section, focus, radius):
    """The share of `check_arguments` that `psf.check_arguments` needs too.  -> (focus, radius), as there."""
    if section is not None:
        check_type("section", section, int)
        check_not_below("section", section, 0)
        check_not_above("section", section, nt - 2)
    if focus is not None:
        check_type("focus", focus, (list, tuple, np.ndarray))
        f = np.asarray(focus)
        if f.shape != (3,):
            raise ValueError(f"Property 'focus' needs to hold three numbers, but has shape {f.shape}.")
        if not (np.issubdtype(f.dtype, np.floating) or np.issubdtype(f.dtype, np.integer)):
            raise TypeError(f"Property 'focus' needs to hold real numbers, but holds {f.dtype}.")
        focus = np.array(f, dtype=np.float64)
        if not np.all(np.isfinite(focus)):
            raise ValueError("Property 'focus' needs to hold finite values only.")
    if radius is not None:
        radius = _finite_number("radius", radius, nonzero=True)
    return focus, radius


def check_arguments(nt: int, section, focus, radius, n_zernike, n_grid, pupil_radius):
    """Argument checks of `Raytracer.wavefront_analysis`, host only; nt: sections per ray of the geometry.
    -> (focus as a float64 array or None, radius, pupil_radius as floats or None)."""
    check_type("n_zernike", n_zernike, int)
    check_not_below("n_zernike", n_zernike, 1)
    check_not_above("n_zernike", n_zernike, _capi.WF_MAX_J)
    check_type("n_grid", n_grid, int)
    check_not_below("n_grid", n_grid, 1)
    check_not_above("n_grid", n_grid, _capi.WF_MAX_GRID)
    focus, radius = check_sphere_arguments(nt, section, focus, radius)
    if pupil_radius is not None:
        pupil_radius = _finite_number("pupil_radius", pupil_radius, positive=True)
    return focus, radius, pupil_radius


class WavefrontAnalysis(BaseClass):
    """Result of `Raytracer.wavefront_analysis`; lengths in mm.

    N, power: rays used (weight > 0 in the section, met by the reference sphere) and their summed weight.  n_missed: rays alive in
    the section whose line does not meet the sphere.  section: the section analysed.  focus (3), radius: centre and signed
    radius of the reference sphere (positive: a converging bundle, the sphere upstream of the focus).  wavelength: power-weighted
    mean, nm.  opl_mean: weighted mean optical path to the sphere; the OPD of a ray is its path minus this mean.  rms, pv,
    opd_min, opd_max: weighted RMS, peak-to-valley and extremes of the OPD.  pupil_centre (2), pupil_radius: weighted mean of the
    intersections' (x, y) about the focus in units of |radius|, and the radius of the disc about it that the polynomials and the
    map live on.  zernike: Noll-ordered orthonormal coefficients of the weighted least-squares fit.  opd_map, weight_map:
    (n_grid, n_grid) over the square around the pupil disc, row index y, column index x; opd_map is the weighted mean OPD per
    cell and NaN where no ray fell.  Without a usable ray N = power = 0, weight_map is zero and every other figure NaN."""

    _tracked = False

    def __init__(self, N: int, power: float, n_missed: int, section: int, focus, radius: float, wavelength: float,
                 opl_mean: float, rms: float, opd_min: float, opd_max: float, pupil_centre, pupil_radius: float, zernike,
                 opd_map, weight_map, **kwargs) -> None:
        super().__init__(**kwargs)
        self.N = int(N)
        self.power = float(power)
        self.n_missed = int(n_missed)
        self.section = int(section)
        self.focus = np.array(focus, dtype=np.float64)
        self.radius = float(radius)
        self.wavelength = float(wavelength)
        self.opl_mean = float(opl_mean)
        self.rms = float(rms)
        self.opd_min, self.opd_max = float(opd_min), float(opd_max)
        self.pv = self.opd_max - self.opd_min
        self.pupil_centre = np.array(pupil_centre, dtype=np.float64)
        self.pupil_radius = float(pupil_radius)
        self.zernike = np.array(zernike, dtype=np.float64)
        self.opd_map = np.array(opd_map, dtype=np.float64)
        self.weight_map = np.array(weight_map, dtype=np.float64)
        self.lock()

    @property
    def rms_waves(self) -> float:
        """RMS of the OPD in units of the mean wavelength."""
        return self.rms / (self.wavelength * 1e-6)

    @property
    def pv_waves(self) -> float:
        """Peak-to-valley of the OPD in units of the mean wavelength."""
        return self.pv / (self.wavelength * 1e-6)

    @property
    def strehl(self) -> float:
        """Strehl ratio by Maréchal's approximation, exp(-(2 pi rms / lambda)^2)."""
        return float(np.exp(-(2 * np.pi * self.rms_waves) ** 2))


def _empty(section: int, focus, radius, n_zernike: int, n_grid: int, n_missed: int = 0, **kwargs) -> WavefrontAnalysis:
    nan = np.nan
    return WavefrontAnalysis(0, 0.0, n_missed, section, np.full(3, nan) if focus is None else focus, nan if radius is None else radius,
                             nan, nan, nan, nan, nan, (nan, nan), nan, np.full(n_zernike, nan), np.full((n_grid, n_grid), nan),
                             np.zeros((n_grid, n_grid)), **kwargs)


def closest_point(sums, origin):
    """The point closest to all ray lines from the sums of `ot_wavefront_focus` (float64 host arithmetic), three NaN where the
    system is singular or its solution not finite (a collimated bundle): the singularity test of the wavefront analysis, which the
    chromatic analysis shares."""
    f = np.asarray(sums, dtype=np.float64)
    A = np.array([[f[8], f[9], f[10]], [f[9], f[11], f[12]], [f[10], f[12], f[13]]])
    try:
        focus = origin + np.linalg.solve(A, f[14:17])
    except np.linalg.LinAlgError:
        focus = np.full(3, np.nan)
    return focus if np.all(np.isfinite(focus)) else np.full(3, np.nan)


def reference_sphere(sums, origin, focus, radius):
    """Centre and signed radius of the default reference sphere from the sums of `ot_wavefront_focus` (float64 host arithmetic):
    the centre is the point closest to all ray lines, the radius its distance from the mean start of the section, positive
    when the bundle runs towards the centre.  `focus`, `radius`: the caller's, where given."""
    f = np.asarray(sums, dtype=np.float64)
    W = f[0]
    if focus is None:
        focus = closest_point(f, origin)
        if not np.all(np.isfinite(focus)):
            raise RuntimeError("The rays of the section have no common closest point (a collimated bundle?): "
                               "pass `focus` and `radius`.")
    if radius is None:
        d = focus - (origin + f[2:5] / W)
        radius = float(np.linalg.norm(d))
        if not radius > 0:
            raise RuntimeError("The focus lies in the mean start position of the section: pass `radius`.")
        if not d @ f[5:8] > 0:
            radius = -radius
    return focus, radius


def unpack_normal_equations(packed, J: int):
    """out of `ot_wavefront_zernike` -> (G (J, J) symmetric, g (J,))."""
    tri = J * (J + 1) // 2
    G = np.zeros((J, J))
    G[np.triu_indices(J)] = packed[:tri]
    return G + np.triu(G, 1).T, np.array(packed[tri:tri + J])


class SphereStage:
    """What `sphere_stage` leaves.  focus, radius: the sphere, as given or as found; empty: no usable ray at the focus stage, and
    nothing else set.  On the device: the planes u, v, opl, w of `ot_wavefront_paths`, wl of the storage, the views mom | missed
    (int64) | extra of one zero-filled float64 buffer, the reductions' workspace ws; R: the rays struct of the C-ABI."""

    def __init__(self, focus, radius) -> None:
        self.focus, self.radius, self.empty = focus, radius, True

    def read(self):
        """-> (moments record, n_missed, extra) on the host: the whole buffer in one read."""
        m, missed, extra = np.split(self._res.cpu().numpy(), [_capi.WF_M, _capi.WF_M + 1])
        return m, int(missed.view(np.int64)[0]), extra


def sphere_stage(rays, first: int, count: int, section: int, origin, focus, radius, extra: int) -> SphereStage:
    """The start that wavefront analysis and Huygens PSF share, arguments as for `analyse`: the reference sphere (`ot_wavefront_focus`,
    where focus or radius is left to it), the paths to it and their moments.  extra: doubles of the result buffer behind the
    moments and the missed count, for the caller's own passes."""
    import torch
    from ._device import require_device, ptr, stream_ptr
    lib = _capi.load_library()
    dev = require_device()
    S = SphereStage(focus, radius)
    if count < 1:
        return S
    st = stream_ptr()
    S.R = R = rays._rays_struct()
    S.ws = ws = torch.empty(_capi.WF_WS, dtype=torch.float64, device=dev)
    d3 = C.c_double * 3
    if focus is None or radius is None:
        sums = torch.zeros(_capi.WF_FOCUS_M, dtype=torch.float64, device=dev)
        origin = np.array(origin, dtype=np.float64)
        _capi.check(lib.ot_wavefront_focus(C.byref(R), first, count, section, d3(*origin), ptr(ws), ptr(sums), st))
        f = sums.cpu().numpy()
        if not f[0] > 0:
            return S
        S.focus, S.radius = focus, radius = reference_sphere(f, origin, focus, radius)

    rays._dev["n"]  # (the index plane is written when it is read: this fills it if the trace left it stale)
    planes = torch.empty(3 * count, dtype=torch.float64, device=dev)
    S.u, S.v, S.opl = u, v, opl = planes[:count], planes[count:2 * count], planes[2 * count:]
    S.w = w = torch.empty(count, dtype=torch.float32, device=dev)
    S._res = torch.zeros(_capi.WF_M + 1 + extra, dtype=torch.float64, device=dev)
    S.mom, S.missed, S.extra = S._res.split([_capi.WF_M, 1, extra])
    S.missed = S.missed.view(torch.int64)
    _capi.check(lib.ot_wavefront_paths(C.byref(R), first, count, section, d3(*focus), radius, ptr(u), ptr(v), ptr(opl), ptr(w),
                                       ptr(S.missed), st))
    S.wl = wl = rays._dev["wl"][first:first + count]
    _capi.check(lib.ot_wavefront_moments(count, ptr(u), ptr(v), ptr(opl), ptr(w), ptr(wl), ptr(ws), ptr(S.mom), st))
    S.empty = False
    return S


def analyse(rays, first: int, count: int, section: int, origin, focus, radius, n_zernike: int, n_grid: int, pupil_radius,
            **kwargs) -> WavefrontAnalysis:
    """Figures of the rays [first, first + count) of the storage `rays` behind section `section`.  origin: a point near the
    section's start that the device subtracts before it sums positions; the other arguments as `check_arguments` returned
    them."""
    from ._device import ptr, stream_ptr
    lib = _capi.load_library()
    J = n_zernike
    T, cells = J * (J + 1) // 2 + J, n_grid * n_grid
    S = sphere_stage(rays, first, count, section, origin, focus, radius, T + 2 * cells)  # extra: normal equations | map sums
    focus, radius = S.focus, S.radius
    if S.empty:
        return _empty(section, focus, radius, J, n_grid, **kwargs)
    st = stream_ptr()
    u, v, opl, w, mom = ptr(S.u), ptr(S.v), ptr(S.opl), ptr(S.w), ptr(S.mom)
    pr = np.nan if pupil_radius is None else pupil_radius
    _capi.check(lib.ot_wavefront_map(count, u, v, opl, w, mom, pr, n_grid, ptr(S.extra[T:]), st))
    _capi.check(lib.ot_wavefront_zernike(count, u, v, opl, w, mom, pr, J, ptr(S.ws), ptr(S.extra[:T]), st))
    m, n_missed, h = S.read()
    packed, sums = h[:T], h[T:].reshape(2, n_grid, n_grid)
    W = m[0]
    if not W > 0:
        return _empty(section, focus, radius, J, n_grid, n_missed, **kwargs)
    G, g = unpack_normal_equations(packed, J)
    try:
        coeff = np.linalg.solve(G, g)
    except np.linalg.LinAlgError:
        warning("The Zernike fit is singular (fewer distinct rays than polynomials): no coefficients.")
        coeff = np.full(J, np.nan)
    mean = m[2] / W
    weight = sums[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        opd_map = np.where(weight > 0, sums[1] / weight, np.nan)
    return WavefrontAnalysis(int(m[1]), W, n_missed, section, focus, radius, m[5] / W, mean, np.sqrt(m[8] / W), m[6] - mean,
                             m[7] - mean, (m[3] / W, m[4] / W), m[10] if pupil_radius is None else pupil_radius, coeff,
                             opd_map, weight, **kwargs)
