"""Chromatic analysis: how a traced bundle differs from one band of wavelengths to the next -- the focus of every band (axial
colour) and where the bands cross a common plane (lateral colour, spot per band), reduced on the device from the position, weight
and wavelength planes of one section of the ray storage.

`Raytracer.chromatic_analysis` has no counterpart in optrace, where these figures take a trace per spectral line or the whole ray
storage on the host.  Definition: DESIGN.md, "Chromatic analysis".  Kernels: csrc/ot_chromatic.hpp behind `ot_chromatic_*`; the
bands are those of `huygens_stack` (`psf.assign_bands`, `psf.settle_bands`), the focus of a band that of the wavefront analysis
(`wavefront.closest_point`).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from . import psf as _psf
from . import wavefront as _wavefront
from .base import BaseClass, check_type


def check_arguments(nt: int, section, bands, z, reference):
    """Argument checks of `Raytracer.chromatic_analysis`, host only; nt: sections per ray of the geometry.
    -> (bands as `psf.check_stack_arguments` returns them, z and reference as floats or None)."""
    _wavefront.check_sphere_arguments(nt, section, None, None)
    bands = _psf.check_bands(bands)
    if z is not None:
        z = _wavefront._finite_number("z", z)
    if reference is not None:
        reference = _wavefront._finite_number("reference", reference)
    return bands, z, reference


class ChromaticAnalysis(BaseClass):
    """Result of `Raytracer.chromatic_analysis`; lengths in mm, wavelengths in nm, powers in W.  K bands of wavelengths.

    section: the section analysed.  n_bands: K; band_edges (K + 1) or None for bands="lines".  band_N, band_power: rays of a band
    in the plane sums and their power; N, power: their totals; n_parallel: used rays that run parallel to the plane and are in none
    of them.  wavelengths: power-weighted mean per band.  reference_band: the band the shifts refer to -- the band with used rays
    whose mean wavelength (the line itself for bands="lines") lies nearest to `reference` --, -1 when there is none.
    focus (K, 3): the point closest to the band's ray lines, NaN where there is none (a collimated band, a single ray);
    focal_shift: focus z minus that of the reference band; axial_colour: largest minus smallest focus z over the bands that have one.
    z: the plane the bands' spots are compared on.  centroid (K, 2): power-weighted mean of where a band's rays cross it;
    lateral_shift (K, 2): centroid minus that of the reference band; lateral_colour: the largest length of a lateral shift.  rms_x,
    rms_y, rms_radius, cov_xy, max_radius: second moments and largest distance about the band's own centroid; a band of one ray has
    RMS figures of exactly 0.  centroid_all (2), rms_radius_all: the polychromatic spot, all bands about their common centroid.
    A band without a ray has band_N = band_power = 0 and NaN elsewhere.  records (K, 10): what the device returned
    (include/optrace_amd.h, ot_chromatic_plane)."""

    _tracked = False

    def __init__(self, records, focus, z: float, reference_band: int, section: int, band_edges=None, **kwargs) -> None:
        super().__init__(**kwargs)
        rec = np.array(records, dtype=np.float64).reshape(-1, _capi.CHROM_M)
        K = rec.shape[0]
        if not 1 <= K <= _capi.CHROM_MAX_BANDS:
            raise ValueError(f"1 to {_capi.CHROM_MAX_BANDS} bands, but the records hold {K}.")
        self.records = rec
        self.focus = np.array(focus, dtype=np.float64).reshape(-1, 3)
        if self.focus.shape[0] != K:
            raise ValueError(f"{K} bands, but {self.focus.shape[0]} foci.")
        self.band_edges = None if band_edges is None else np.array(band_edges, dtype=np.float64).reshape(-1)
        if self.band_edges is not None and self.band_edges.shape[0] != K + 1:
            raise ValueError(f"{K} bands need {K + 1} edges, but there are {self.band_edges.shape[0]}.")
        check_type("reference_band", reference_band, (int, np.integer))
        if not -1 <= reference_band < K:
            raise ValueError(f"Reference band {reference_band} out of range for {K} bands.")
        self.n_bands, self.reference_band, self.section, self.z = K, int(reference_band), int(section), float(z)
        ref = self.reference_band
        self.band_N, self.band_power = rec[:, 1].astype(np.int64), rec[:, 0].copy()
        self.N, self.power, self.n_parallel = int(self.band_N.sum()), float(self.band_power.sum()), int(rec[:, 9].sum())
        some, single = self.band_N > 0, self.band_N == 1
        nan2 = np.full(2, np.nan)
        with np.errstate(invalid="ignore", divide="ignore"):
            W = np.where(some, self.band_power, np.nan)
            self.wavelengths = rec[:, 4] / W
            self.centroid = rec[:, 2:4] / W[:, None]
            # (one ray is its own centroid: w x / w need not return x to the last bit, the figures say so exactly)
            self.rms_x = np.where(single, 0.0, np.sqrt(rec[:, 5] / W))
            self.rms_y = np.where(single, 0.0, np.sqrt(rec[:, 6] / W))
            self.cov_xy = np.where(single, 0.0, rec[:, 7] / W)
            self.rms_radius = np.sqrt(self.rms_x ** 2 + self.rms_y ** 2)
            self.max_radius = np.where(some, np.sqrt(rec[:, 8]), np.nan)
            self.focal_shift = self.focus[:, 2] - (self.focus[ref, 2] if ref >= 0 else np.nan)
            fz = self.focus[np.isfinite(self.focus[:, 2]), 2]
            self.axial_colour = float(fz.max() - fz.min()) if fz.shape[0] else float("nan")
            self.lateral_shift = self.centroid - (self.centroid[ref] if ref >= 0 else nan2)
            shift = np.hypot(self.lateral_shift[:, 0], self.lateral_shift[:, 1])
            self.lateral_colour = float(np.nanmax(shift)) if np.any(np.isfinite(shift)) else float("nan")
            if self.power > 0:
                Wb, cb = self.band_power[some], self.centroid[some]
                self.centroid_all = rec[some, 2:4].sum(axis=0) / self.power
                apart = ((cb - self.centroid_all) ** 2).sum(axis=1)
                self.rms_radius_all = float(np.sqrt((rec[some, 5] + rec[some, 6] + Wb * apart).sum() / self.power))
            else:
                self.centroid_all, self.rms_radius_all = nan2, float("nan")
        self.lock()


def _empty(section: int, bands, z, **kwargs) -> ChromaticAnalysis:
    """(the rule of `spot._empty`: what the caller fixed stays; bands given as edges keep them, else one band without a ray)"""
    edges = bands if isinstance(bands, np.ndarray) else None
    K = 1 if edges is None else edges.shape[0] - 1
    rec = np.zeros((K, _capi.CHROM_M))
    rec[:, 5:8] = np.nan
    return ChromaticAnalysis(rec, np.full((K, 3), np.nan), np.nan if z is None else z, -1, section, edges, **kwargs)


def band_foci(sums, origin):
    """sums (K, 17) of `ot_chromatic_focus` -> foci (K, 3): `wavefront.closest_point` per band.  A band of fewer than two rays has
    no focus, and neither has one whose system is singular to rounding (rank below 3 at NumPy's tolerance, 3 eps times the largest
    singular value: rays of one direction, where rounding may leave the solver a pivot); this rank test is the chromatic
    analysis' own, on top of the wavefront analysis' test."""
    def focus(f):
        A = np.array([[f[8], f[9], f[10]], [f[9], f[11], f[12]], [f[10], f[12], f[13]]])
        if f[1] < 2 or not np.all(np.isfinite(A)) or np.linalg.matrix_rank(A) < 3:
            return np.full(3, np.nan)
        return _wavefront.closest_point(f, origin)
    return np.array([focus(f) for f in np.asarray(sums, dtype=np.float64).reshape(-1, _capi.WF_FOCUS_M)]).reshape(-1, 3)


def reference_band(wavelengths, counts, reference: float) -> int:
    """The band with rays (counts > 0) whose mean wavelength lies nearest to `reference`, the lower index on a tie; -1 if none."""
    with np.errstate(invalid="ignore"):
        dist = np.where(np.asarray(counts) > 0, np.abs(np.asarray(wavelengths, dtype=np.float64) - reference), np.inf)
    dist = np.where(np.isnan(dist), np.inf, dist)
    b = int(np.argmin(dist))
    return b if np.isfinite(dist[b]) else -1


def analyse(rays, first: int, count: int, section: int, origin, bands, z, reference, **kwargs) -> ChromaticAnalysis:
    """Figures of the rays [first, first + count) of the storage `rays` in section `section`; origin: a point near the section's
    start that the device subtracts before it sums positions; bands, z, reference as `check_arguments` returned them.  Reads the p,
    w and wl planes only.  The reference band is the band with used rays whose mean wavelength lies nearest to `reference`: a line
    for bands="lines", slot 4 / slot 0 of the records otherwise (a band whose used rays all run within a plane z = const has none
    and is passed over).  Reads of the device: for "lines" the table of lines, 33 doubles, before the launches; one for the focus
    sums and, with `z` given, the records; with `z` left open a second one for the records on the reference band's focus' plane --
    other bands than lines then need a first plane pass, on the plane through `origin`, for their mean wavelengths."""
    import torch
    from ._device import require_device, ptr, stream_ptr
    lib = _capi.load_library()
    dev = require_device()
    if count < 1:
        return _empty(section, bands, z, **kwargs)
    nt, Np, k = int(rays.Nt), int(rays._Np), section
    R = rays._rays_struct(tail_only=k >= nt - 2)  # (addresses only: neither the index plane nor the polarisation planes are filled)
    st = stream_ptr()
    raw = lambda name: dict.__getitem__(rays._dev, name)  # (past the hook of `_dev`: no fill)
    p, w_k = raw("p"), raw("w")[Np * k + first:Np * k + first + count]
    wl = rays._dev["wl"][first:first + count]

    # the used rays, as the kernels test them, for the bands' definition
    L2 = torch.zeros(count, dtype=torch.float64, device=dev)
    for c in range(3):
        at = Np * (k + nt * c) + first
        L2 += (p[at + Np:at + Np + count] - p[at:at + count]) ** 2
    live = (w_k > 0) & (L2 > 0)
    key, K_set, table = _psf.assign_bands(wl, live, bands)
    key8 = torch.where(key < K_set, key, _capi.CHROM_NO_BAND).to(torch.uint8)
    lines = isinstance(bands, str)
    K = K_set  # the bands of the launches
    if lines:  # (the table is read here, 33 doubles: the launches take the lines there are, not the 32 the table has room for)
        table = table.cpu().numpy()
        K = max(1, min(int(table[0]), K_set))
    # power and power times wavelength of all used rays, for the default `reference`
    w64 = torch.where(live, w_k.to(torch.float64), 0.0)
    wwl = w64 * wl.to(torch.float64)

    M = _capi.WF_FOCUS_M
    ws = torch.empty(max(1, lib.ot_chromatic_workspace(count, K)), dtype=torch.float64, device=dev)
    sums = torch.zeros(K * M, dtype=torch.float64, device=dev)
    origin = np.array(origin, dtype=np.float64)
    _capi.check(lib.ot_chromatic_focus(C.byref(R), first, count, k, ptr(key8), K, (C.c_double * 3)(*origin), ptr(ws), ptr(sums), st))

    def plane(z0: float):
        rec = torch.zeros(K * _capi.CHROM_M, dtype=torch.float64, device=dev)
        _capi.check(lib.ot_chromatic_plane(C.byref(R), first, count, k, ptr(key8), K, z0, ptr(ws), ptr(rec), st))
        return rec

    # A line is its band's mean wavelength.  Other bands take theirs from the records, slot 4 / slot 0, which like the power and the
    # ray count of a band are the same on every plane: with `z` left open a first pass on the plane through `origin` gives them, in
    # the same read as the focus sums.
    rec = plane(z if z is not None else float(origin[2])) if z is not None or not lines else sums[:0]
    head = torch.cat([sums, w64.sum().reshape(1), wwl.sum().reshape(1), rec] + ([] if lines else [table])).cpu().numpy()
    sums, totals, rec, rest = np.split(head, np.cumsum([K * M, 2, rec.shape[0]]))
    table = table if lines else rest
    sums, rec = sums.reshape(K, M), rec.reshape(-1, _capi.CHROM_M)
    counts = np.zeros(K_set)
    counts[:K] = sums[:, 1]
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    K_left, starts, edges = _psf.settle_bands(bands, K_set, starts, table)
    if not starts[-1]:
        return _empty(section, bands, z, **kwargs)
    # the bands that are left: the lines there are; or the last one, where an int asked for bands over a single wavelength
    keep = slice(K - 1, K) if not lines and K_left < K else slice(0, K_left)
    sums = sums[keep]
    focus = band_foci(sums, origin)
    if reference is None:
        reference = totals[1] / totals[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        band_wl = table[1:1 + K_left] if lines else rec[keep, 4] / rec[keep, 0]
    ref = reference_band(band_wl, sums[:, 1], reference)
    if z is None:
        z = float(focus[ref, 2]) if ref >= 0 else np.nan  # (no band with a mean wavelength: every used ray runs within a plane z = const)
        if not np.isfinite(z):
            raise RuntimeError("The rays of the reference band have no common closest point (a collimated bundle, a single ray?): "
                               "pass `z`.")
        rec = plane(z).cpu().numpy().reshape(-1, _capi.CHROM_M)
    rec = rec[keep]
    return ChromaticAnalysis(rec, focus, z, ref, section, edges, **kwargs)
