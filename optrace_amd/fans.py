"""Ray fans: the transverse ray aberration and the optical path difference of a traced bundle against the pupil coordinate, along
the tangential and the sagittal cut of the pupil, one curve per band of wavelengths, together with every band's own wavefront and
spot figures -- reduced on the device from the planes the sphere stage of the wavefront analysis leaves there.

`Raytracer.ray_fans` has no counterpart in optrace.  Definition: DESIGN.md, "Ray fans".  Kernels: csrc/ot_fans.hpp behind
`ot_fans_*`; the sphere is that of `wavefront.sphere_stage`, the bands are those of `huygens_stack` and `chromatic_analysis`
(`psf.assign_bands`, `psf.settle_bands`).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from . import psf as _psf
from . import wavefront as _wavefront
from .base import BaseClass, check_type, check_not_below, check_not_above


def check_arguments(nt: int, section, bands, focus, radius, n_bins, slab, pupil_radius):
    """Argument checks of `Raytracer.ray_fans`, host only; nt: sections per ray of the geometry.
    -> (bands as `psf.check_bands` returns them, focus as a float64 array or None, radius, slab, pupil_radius as floats or None)."""
    focus, radius = _wavefront.check_sphere_arguments(nt, section, focus, radius)
    bands = _psf.check_bands(bands)
    check_type("n_bins", n_bins, int)
    check_not_below("n_bins", n_bins, 1)
    check_not_above("n_bins", n_bins, _capi.FAN_MAX_BINS)
    slab = _wavefront._finite_number("slab", slab, positive=True)
    if slab > 1:
        raise ValueError(f"Property 'slab' needs to be above 0 and at most 1, but is {slab}.")
    if pupil_radius is not None:
        pupil_radius = _wavefront._finite_number("pupil_radius", pupil_radius, positive=True)
    return bands, focus, radius, slab, pupil_radius


class RayFans(BaseClass):
    """Result of `Raytracer.ray_fans`; lengths in mm, wavelengths in nm, powers in W.  K bands of wavelengths, n_bins bins over the
    pupil coordinate -1 .. 1 in each of two fans: fan 0 the tangential one (rays with |x| <= slab, binned by y), fan 1 the sagittal
    one (|y| <= slab, binned by x), (x, y) the unit-disc coordinates of the wavefront analysis.

    section: the section analysed.  focus (3), radius: the reference sphere, one for all bands.  pupil_centre (2), pupil_radius: as
    for `WavefrontAnalysis`, the same for all bands.  slab: half width of a cut.  n_bands: K; band_edges (K + 1) or None for
    bands="lines".  band_N, band_power: rays of a band and their power; N, power: their totals.  n_missed: living rays whose
    line does not meet the sphere; n_parallel: used rays that run within a plane z = const and so never cross the focus' plane;
    n_out_of_band: used rays in no band.  wavelengths: power-weighted mean per band.
    Per band, the wavefront: opl_mean; opd_rms, opd_min, opd_max, opd_pv of the path difference against the band's own mean;
    opd_rms_waves in units of the band's wavelength.  Per band, the spot in the plane z = focus z: centroid (K, 2) relative to the
    focus, rms_x, rms_y, rms_radius about the band's own centroid, max_radius from it; a band of one ray has RMS figures of
    exactly 0.  A band without a ray has band_N = band_power = 0 and NaN elsewhere.
    Per band, fan and bin, (K, 2, n_bins): weight and count of the rays; pupil, their weighted mean coordinate; ex, ey, the
    weighted mean transverse aberration, where the ray crosses the plane z = focus z minus the focus; opd, the weighted mean
    path difference against the band's mean.  The last four are NaN where count == 0.
    records (K, 13), bins (K, 2, n_bins, 6): what the device returned (include/optrace_amd.h, ot_fans_bands, ot_fans_bins)."""

    _tracked = False

    def __init__(self, records, bins, section: int, focus, radius: float, pupil_centre, pupil_radius: float, slab: float,
                 n_missed: int = 0, n_parallel: int = 0, n_out_of_band: int = 0, band_edges=None, **kwargs) -> None:
        super().__init__(**kwargs)
        rec = np.array(records, dtype=np.float64)
        if rec.ndim != 2 or rec.shape[1] != _capi.FAN_M:
            raise ValueError(f"Records of shape (K, {_capi.FAN_M}) are needed, but the shape is {rec.shape}.")
        K = rec.shape[0]
        if not 1 <= K <= _capi.CHROM_MAX_BANDS:
            raise ValueError(f"1 to {_capi.CHROM_MAX_BANDS} bands, but the records hold {K}.")
        b = np.array(bins, dtype=np.float64)
        if b.ndim != 4 or b.shape[0] != K or b.shape[1] != 2 or b.shape[3] != _capi.FAN_BIN_M:
            raise ValueError(f"Bins of shape ({K}, 2, n_bins, {_capi.FAN_BIN_M}) are needed, but the shape is {b.shape}.")
        if not 1 <= b.shape[2] <= _capi.FAN_MAX_BINS:
            raise ValueError(f"1 to {_capi.FAN_MAX_BINS} bins, but there are {b.shape[2]}.")
        self.records, self.bins = rec, b
        self.band_edges = None if band_edges is None else np.array(band_edges, dtype=np.float64).reshape(-1)
        if self.band_edges is not None and self.band_edges.shape[0] != K + 1:
            raise ValueError(f"{K} bands need {K + 1} edges, but there are {self.band_edges.shape[0]}.")
        self.focus = np.array(focus, dtype=np.float64).reshape(-1)
        self.pupil_centre = np.array(pupil_centre, dtype=np.float64).reshape(-1)
        if self.focus.shape[0] != 3 or self.pupil_centre.shape[0] != 2:
            raise ValueError("A focus of three numbers and a pupil centre of two are needed.")
        self.n_bands, self.n_bins, self.section = K, int(b.shape[2]), int(section)
        self.radius, self.pupil_radius, self.slab = float(radius), float(pupil_radius), float(slab)
        self.n_missed, self.n_parallel, self.n_out_of_band = int(n_missed), int(n_parallel), int(n_out_of_band)
        self.band_N, self.band_power = rec[:, 1].astype(np.int64), rec[:, 0].copy()
        self.N, self.power = int(self.band_N.sum()), float(self.band_power.sum())
        some, single = self.band_N > 0, self.band_N == 1
        with np.errstate(invalid="ignore", divide="ignore"):
            W = np.where(some, self.band_power, np.nan)
            self.wavelengths = rec[:, 5] / W
            self.opl_mean = rec[:, 2] / W
            # (one ray is its own mean: w a / w need not return a to the last bit, the figures say so exactly)
            self.opd_rms = np.where(single, 0.0, np.sqrt(rec[:, 8] / W))
            self.opd_min, self.opd_max = rec[:, 6] - self.opl_mean, rec[:, 7] - self.opl_mean
            self.opd_pv = self.opd_max - self.opd_min
            self.opd_rms_waves = self.opd_rms / (self.wavelengths * 1e-6)
            self.centroid = rec[:, 3:5] / W[:, None]
            self.rms_x = np.where(single, 0.0, np.sqrt(rec[:, 9] / W))
            self.rms_y = np.where(single, 0.0, np.sqrt(rec[:, 10] / W))
            self.rms_radius = np.sqrt(self.rms_x ** 2 + self.rms_y ** 2)
            self.max_radius = np.where(some, np.sqrt(rec[:, 12]), np.nan)
            self.weight = b[..., 0].copy()
            self.count = b[..., 1].astype(np.int64)
            Wb = np.where(self.count > 0, self.weight, np.nan)
            self.pupil, self.ex, self.ey, self.opd = (b[..., s] / Wb for s in (2, 3, 4, 5))
        self.lock()

    def tangential(self, band: int = 0):
        """-> (pupil coordinate y, ey, opd) of the tangential fan of a band, (n_bins,) each."""
        return self.pupil[band, 0], self.ey[band, 0], self.opd[band, 0]

    def sagittal(self, band: int = 0):
        """-> (pupil coordinate x, ex, opd) of the sagittal fan of a band, (n_bins,) each."""
        return self.pupil[band, 1], self.ex[band, 1], self.opd[band, 1]


def _empty(section: int, bands, focus, radius, n_bins: int, slab: float, pupil_radius, n_missed: int = 0, n_parallel: int = 0,
           n_out_of_band: int = 0, **kwargs) -> RayFans:
    """(the rule of `chromatic._empty`: what the caller fixed stays; bands given as edges keep them, else one band without a ray)"""
    edges = bands if isinstance(bands, np.ndarray) else None
    K = 1 if edges is None else edges.shape[0] - 1
    rec = np.zeros((K, _capi.FAN_M))
    rec[:, 9:12] = np.nan
    nan = np.nan
    return RayFans(rec, np.zeros((K, 2, n_bins, _capi.FAN_BIN_M)), section, np.full(3, nan) if focus is None else focus,
                   nan if radius is None else radius, (nan, nan), nan if pupil_radius is None else pupil_radius, slab, n_missed,
                   n_parallel, n_out_of_band, edges, **kwargs)


def analyse(rays, first: int, count: int, section: int, origin, bands, focus, radius, n_bins: int, slab: float, pupil_radius,
            **kwargs) -> RayFans:
    """Fans of the rays [first, first + count) of the storage `rays` behind section `section`; origin: a point near the section's
    start that the device subtracts before it sums positions; the other arguments as `check_arguments` returned them.  Reads of
    the device: those of `wavefront.sphere_stage`; for "lines" the table of lines, 33 doubles, before the launches; one for the
    moments, the records, the bins and the counts together."""
    import torch
    from ._device import ptr, stream_ptr
    lib = _capi.load_library()
    lines = isinstance(bands, str)
    K_set = _capi.PSF_MAX_BANDS if lines else bands.shape[0] - 1 if isinstance(bands, np.ndarray) else bands
    M, cells = _capi.FAN_M, 2 * n_bins * _capi.FAN_BIN_M
    parts = [K_set * M, K_set * cells, 1, 1, K_set + 1]  # records | bins | parallel (int64) | out of band | the band table
    S = _wavefront.sphere_stage(rays, first, count, section, origin, focus, radius, sum(parts))
    focus, radius = S.focus, S.radius
    empty = lambda *counts: _empty(section, bands, focus, radius, n_bins, slab, pupil_radius, *counts, **kwargs)
    if S.empty:
        return empty()
    st, k = stream_ptr(), section
    rec, out, par, oob, tab = S.extra.split(parts)
    planes = torch.empty(2 * count, dtype=torch.float64, device=S.u.device)
    ex, ey = planes[:count], planes[count:]
    _capi.check(lib.ot_fans_transverse(C.byref(S.R), first, count, k, (C.c_double * 3)(*focus), ptr(S.w), ptr(ex), ptr(ey), ptr(par), st))

    live = S.w > 0
    key, _, table = _psf.assign_bands(S.wl, live, bands)
    oob.copy_(torch.count_nonzero(live & (key >= K_set)).to(torch.float64).reshape(1))
    key8 = torch.where(key < K_set, key, _capi.CHROM_NO_BAND).to(torch.uint8)
    K = K_set  # the bands of the launches
    if lines:  # (the table is read here, 33 doubles: the launches take the lines there are, not the 32 the table has room for)
        table = table.cpu().numpy()
        K = max(1, min(int(table[0]), K_set))
    else:
        tab.copy_(table)
    ws = torch.empty(max(1, lib.ot_fans_workspace(count, K)), dtype=torch.float64, device=S.u.device)
    pr = np.nan if pupil_radius is None else pupil_radius
    _capi.check(lib.ot_fans_bands(count, ptr(S.opl), ptr(ex), ptr(ey), ptr(S.w), ptr(S.wl), ptr(key8), K, ptr(ws), ptr(rec), st))
    _capi.check(lib.ot_fans_bins(count, ptr(S.u), ptr(S.v), ptr(S.opl), ptr(ex), ptr(ey), ptr(S.w), ptr(key8), ptr(S.mom), pr, ptr(rec),
                                 K, n_bins, slab, ptr(out), st))

    m, n_missed, h = S.read()
    rec, out, par, oob, tab = np.split(h, np.cumsum(parts)[:-1])
    counts = int(par.view(np.int64)[0]), int(oob[0])
    rec, out = rec[:K * M].reshape(K, M), out[:K * cells].reshape(K, 2, n_bins, _capi.FAN_BIN_M)
    table = table if lines else tab
    n_band = np.zeros(K_set)
    n_band[:K] = rec[:, 1]
    starts = np.concatenate([[0], np.cumsum(n_band)]).astype(np.int64)
    K_left, starts, edges = _psf.settle_bands(bands, K_set, starts, table)
    if not starts[-1]:
        return empty(n_missed, *counts)
    # the bands that are left: the lines there are; or the last one, where an int asked for bands over a single wavelength
    keep = slice(K - 1, K) if not lines and K_left < K else slice(0, K_left)
    return RayFans(rec[keep], out[keep], section, focus, radius, (m[3] / m[0], m[4] / m[0]),
                   m[10] if pupil_radius is None else pupil_radius, slab, n_missed, *counts, edges, **kwargs)
