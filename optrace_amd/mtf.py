"""MTF analysis: the geometric modulation transfer function across the field and through focus -- per field point (the rays of one
source), band of wavelengths, plane and spatial frequency the contrast along the tangential direction of the field and across it,
reduced on the device from the position, weight and wavelength planes of one section of the ray storage in one call for all
fields, bands, planes and frequencies.

`Raytracer.mtf_analysis` has no counterpart in optrace.  Definition: DESIGN.md, "MTF analysis".  Kernel: csrc/ot_mtf.hpp behind
`ot_mtf_sums`; fields, bands, used rays and ray lines are those of the field analysis (`field.band_records`), whose records give
the means the phases are taken about.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from . import field as _field
from .base import BaseClass, check_type

N_DEFAULT_FREQUENCIES = 17  # (those of `spot_analysis`)


def check_arguments(frequencies, dz):
    """Argument checks of `Raytracer.mtf_analysis` beyond those of `field.check_arguments`, host only.  -> (frequencies as a float64
    array or None, dz as a float64 array)."""
    if frequencies is not None:
        check_type("frequencies", frequencies, (list, tuple, np.ndarray))
        freq = np.asarray(frequencies)
        if freq.size and not (np.issubdtype(freq.dtype, np.floating) or np.issubdtype(freq.dtype, np.integer)):
            raise TypeError(f"Property 'frequencies' needs to hold real numbers, but holds {freq.dtype}.")
        frequencies = np.array(freq, dtype=np.float64)
        if frequencies.ndim != 1 or not 1 <= frequencies.shape[0] <= _capi.MTF_MAX_FREQ:
            raise ValueError(f"Property 'frequencies' needs to hold 1 to {_capi.MTF_MAX_FREQ} values in one dimension, but has the "
                             f"shape {frequencies.shape}.")
        if not np.all(np.isfinite(frequencies)) or np.any(frequencies < 0):
            raise ValueError("Property 'frequencies' needs to hold finite values of 0 or above only.")
    if dz is None:
        return frequencies, np.zeros(1)
    check_type("dz", dz, (list, tuple, np.ndarray))
    off = np.asarray(dz)
    if off.size and not (np.issubdtype(off.dtype, np.floating) or np.issubdtype(off.dtype, np.integer)):
        raise TypeError(f"Property 'dz' needs to hold real numbers, but holds {off.dtype}.")
    off = np.array(off, dtype=np.float64)
    if off.ndim != 1 or not 1 <= off.shape[0] <= _capi.MTF_MAX_PLANES:
        raise ValueError(f"Property 'dz' needs to hold 1 to {_capi.MTF_MAX_PLANES} offsets in one dimension, but has the shape {off.shape}.")
    if not np.all(np.isfinite(off)) or np.any(np.diff(off) <= 0):
        raise ValueError("Property 'dz' needs to hold finite, strictly increasing offsets.")
    return frequencies, off


def parabola_peak(x, y):
    """x (Z) ascending, y (..., Z) -> (...): where the parabola through the largest y and its two neighbours has its vertex; NaN
    for Z < 3, a largest value on the first or last plane (of equal values the first counts), or a NaN among the values."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    out = np.full(y.shape[:-1], np.nan)
    if x.shape[0] < 3:
        return out
    bad = np.any(np.isnan(y), axis=-1)
    i = np.argmax(np.where(np.isnan(y), -np.inf, y), axis=-1)
    inner = ~bad & (i > 0) & (i < x.shape[0] - 1)
    j = np.where(inner, i, 1)
    take = lambda off: np.take_along_axis(y, (j + off)[..., None], axis=-1)[..., 0]
    y0, y1, y2 = take(-1), take(0), take(1)
    x0, x2 = x[j - 1] - x[j], x[j + 1] - x[j]
    # y1 + b u + c u^2 through (x0, y0) and (x2, y2), u from the plane of the largest value: c < 0, the vertex lies at -b / 2c
    with np.errstate(invalid="ignore", divide="ignore"):
        c = ((y2 - y1) / x2 - (y0 - y1) / x0) / (x2 - x0)
        b = (y2 - y1) / x2 - c * x2
        at = x[j] + np.where(c < 0, -b / (2 * c), 0.0)
    out[inner] = at[inner]
    return out


class MTFAnalysis(BaseClass):
    """Result of `Raytracer.mtf_analysis`; lengths in mm, wavelengths in nm, powers in W, frequencies in cycles per mm.  F field
    points, K bands of wavelengths, Z planes, Q frequencies.

    sources (F), section, band_edges (K + 1) or None for bands="lines", wavelengths (K), reference_band, reference_field, field
    (F, 2), t (F, 2): as in `FieldAnalysis`; s = (-t_y, t_x) is the sagittal direction.  records (F, K, 18): the records of
    `ot_field_sums` the means are taken from; origin (3): the point its lines refer to.  z: the plane `dz` counts from; planes (Z):
    z + dz; frequencies (Q).  band_N, band_power (F, K): rays of a cell in the sums and their power.
    sums (F, K, Z, Q, 4): what the device returned (include/optrace_amd.h, ot_mtf_sums).  otf_t, otf_s (F, K, Z, Q) complex:
    sum w exp(-2 pi i nu u . (x - centroid)) / sum w over the cell's rays where they cross the plane, u = t and s; mtf_t, mtf_s:
    their moduli; centroid (F, K, Z, 2): the power-weighted mean of where the cell's rays cross the plane.  A cell of one ray has
    the OTF 1 exactly.
    otf_t_all, otf_s_all, mtf_t_all, mtf_s_all (F, Z, Q): the polychromatic transfer function of a field, all its bands about their
    common centroid on the plane, each with the weight of its power.
    focus_mtf_t, focus_mtf_s (F, K, Q): z of the through-focus peak of the MTF, the vertex of the parabola through the plane of the
    largest MTF and its two neighbours; NaN for fewer than three planes and where the largest value lies on the first or last one.
    A cell without a ray has band_N = band_power = 0 and NaN elsewhere."""

    _tracked = False

    def __init__(self, sums, records, origin, z: float, planes, frequencies, reference_band: int, reference_field: int, section: int,
                 sources, field, band_edges=None, **kwargs) -> None:
        super().__init__(**kwargs)
        self.sources = np.array(sources, dtype=np.int64).reshape(-1)
        F = self.sources.shape[0]
        if not 1 <= F <= _capi.FIELD_MAX_FIELDS:
            raise ValueError(f"1 to {_capi.FIELD_MAX_FIELDS} fields, but there are {F}.")
        rec = np.array(records, dtype=np.float64).reshape(F, -1, _capi.FIELD_M)
        K = rec.shape[1]
        if not 1 <= K <= _capi.CHROM_MAX_BANDS:
            raise ValueError(f"1 to {_capi.CHROM_MAX_BANDS} bands, but the records hold {K}.")
        self.planes = np.array(planes, dtype=np.float64).reshape(-1)
        self.frequencies = np.array(frequencies, dtype=np.float64).reshape(-1)
        Z, Q = self.planes.shape[0], self.frequencies.shape[0]
        if not 1 <= Z <= _capi.MTF_MAX_PLANES or not 1 <= Q <= _capi.MTF_MAX_FREQ:
            raise ValueError(f"1 to {_capi.MTF_MAX_PLANES} planes and 1 to {_capi.MTF_MAX_FREQ} frequencies, but there are {Z} and {Q}.")
        self.sums = np.array(sums, dtype=np.float64).reshape(F, K, Z, Q, 4)
        self.records = rec
        self.origin = np.array(origin, dtype=np.float64).reshape(3)
        self.band_edges = None if band_edges is None else np.array(band_edges, dtype=np.float64).reshape(-1)
        if self.band_edges is not None and self.band_edges.shape[0] != K + 1:
            raise ValueError(f"{K} bands need {K + 1} edges, but there are {self.band_edges.shape[0]}.")
        check_type("reference_band", reference_band, (int, np.integer))
        check_type("reference_field", reference_field, (int, np.integer))
        if not -1 <= reference_band < K:
            raise ValueError(f"Reference band {reference_band} out of range for {K} bands.")
        if not 0 <= reference_field < F:
            raise ValueError(f"Reference field {reference_field} out of range for {F} fields.")
        self.n_fields, self.n_bands, self.n_planes, self.n_frequencies = F, K, Z, Q
        self.section, self.z = int(section), float(z)
        self.reference_band, self.reference_field = int(reference_band), int(reference_field)
        self.field = np.array(field, dtype=np.float64).reshape(F, 2)
        self.t = _field.directions(self.field)

        self.band_N, self.band_power = rec[:, :, 1].astype(np.int64), rec[:, :, 0].copy()
        some, single = self.band_N > 0, self.band_N == 1
        zeta = self.planes - self.origin[2]
        s = np.stack([-self.t[:, 1], self.t[:, 0]], axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            W = np.where(some, self.band_power, np.nan)
            Wk = rec[:, :, 0].sum(axis=0)
            self.wavelengths = np.where(self.band_N.sum(axis=0) > 0, rec[:, :, 6].sum(axis=0) / Wk, np.nan)
            Wc = W[:, :, None, None]
            one = single[:, :, None, None]  # (one ray is its own centroid: the figures say so exactly)
            self.otf_t = np.where(one, 1.0, (self.sums[..., 0] + 1j * self.sums[..., 1]) / Wc)
            self.otf_s = np.where(one, 1.0, (self.sums[..., 2] + 1j * self.sums[..., 3]) / Wc)
            self.mtf_t, self.mtf_s = np.abs(self.otf_t), np.abs(self.otf_s)
            mean = rec[:, :, None, 2:4] + zeta[None, None, :, None] * rec[:, :, None, 4:6]
            self.centroid = self.origin[:2] + mean / W[:, :, None, None]

            # all bands of a field about their common centroid: the band's OTF turned by the phase of its centroid's offset
            Wb = np.where(some, self.band_power, 0.0)
            Wf = np.where(some.any(axis=1), Wb.sum(axis=1), np.nan)
            c = np.where(some[:, :, None, None], self.centroid, 0.0)
            c_all = (Wb[:, :, None, None] * c).sum(axis=1) / Wf[:, None, None]
            off = c - c_all[:, None]

            def together(otf, u):
                d = off[..., 0] * u[:, None, None, 0] + off[..., 1] * u[:, None, None, 1]  # (F, K, Z)
                turn = np.exp(-2j * np.pi * self.frequencies[None, None, None, :] * d[..., None])
                term = np.where(some[:, :, None, None], Wb[:, :, None, None] * otf * turn, 0.0)
                return term.sum(axis=1) / Wf[:, None, None]

            self.otf_t_all, self.otf_s_all = together(self.otf_t, self.t), together(self.otf_s, s)
            self.mtf_t_all, self.mtf_s_all = np.abs(self.otf_t_all), np.abs(self.otf_s_all)
        self.focus_mtf_t = parabola_peak(self.planes, np.moveaxis(self.mtf_t, 2, -1))
        self.focus_mtf_s = parabola_peak(self.planes, np.moveaxis(self.mtf_s, 2, -1))
        self.lock()


def _empty(section: int, bands, z, dz, freq, origin, reference_field: int, sources, field, **kwargs) -> MTFAnalysis:
    """(the rule of `field._empty`: what the caller fixed stays; bands given as edges keep them, else one band without a ray; no
    frequencies given: those of `spot._empty`)"""
    edges = bands if isinstance(bands, np.ndarray) else None
    K = 1 if edges is None else edges.shape[0] - 1
    rec = np.zeros((len(sources), K, _capi.FIELD_M))
    rec[:, :, 8:] = np.nan
    freq = np.linspace(0, 1, N_DEFAULT_FREQUENCIES) if freq is None else freq
    z = np.nan if z is None else z
    return MTFAnalysis(np.zeros((len(sources), K, dz.shape[0], freq.shape[0], 4)), rec, origin, z, z + dz, freq, -1, reference_field,
                       section, sources, field, edges, **kwargs)


def analyse(rays, ranges, section: int, origin, bands, freq, z, dz, reference, reference_field: int, sources, field, power,
            **kwargs) -> MTFAnalysis:
    """MTF of the fields `ranges` [(first, count), ...] of the storage `rays` in section `section`; origin, bands, z, reference,
    sources, field, power: as for `field.analyse`; freq, dz: as `check_arguments` returned them.  Reads the p, w and wl planes only.
    Reads of the device: those of `field.band_records` -- the records give the default z and the default frequencies -- and one
    for the sums."""
    import torch
    from ._device import require_device, ptr, stream_ptr, to_dev
    lib = _capi.load_library()
    dev = require_device()
    fixed = dict(origin=origin, reference_field=reference_field, sources=sources, field=field)
    front = _field.band_records(rays, ranges, section, origin, bands, reference)
    if front is None:
        return _empty(section, bands, z, dz, freq, **fixed, **kwargs)
    ref = front.reference_band
    if z is None:
        z = _field.default_plane(front, reference_field, section, sources, field, power)
    if freq is None:
        on_z = _field.FieldAnalysis(front.rec, front.origin, z, ref, reference_field, section, sources, field, power, None, front.edges)
        radius = float(on_z.rms_radius[reference_field, ref]) if ref >= 0 else np.nan
        if not radius > 0:
            raise ValueError("The rays of the reference field and band have no RMS radius above 0 on the plane z (a single ray, no "
                             "ray, a perfect focus?): pass `frequencies`.")
        freq = np.linspace(0, 1 / radius, N_DEFAULT_FREQUENCIES)
    planes = z + dz
    zeta = planes - front.origin[2]
    t = _field.directions(field)
    F, K, Z, Q = front.F, front.K, int(dz.shape[0]), int(freq.shape[0])
    ws = torch.empty(max(1, lib.ot_mtf_workspace(front.flat, F, K, Z, Q)), dtype=torch.float64, device=dev)
    d_sums = torch.zeros(F * K * Z * Q * 4, dtype=torch.float64, device=dev)
    d_freq = to_dev(freq, np.float64)
    _capi.check(lib.ot_mtf_sums(C.byref(front.R), front.flat, F, section, ptr(front.key8), front.lo, K, (C.c_double * 3)(*front.origin),
                                ptr(front.d_rec), (C.c_double * (2 * F))(*t.reshape(-1)), (C.c_double * Z)(*zeta), Z, ptr(d_freq), Q,
                                ptr(ws), ptr(d_sums), stream_ptr()))
    sums = d_sums.cpu().numpy().reshape(F, K, Z, Q, 4)[:, front.keep]
    return MTFAnalysis(sums, front.rec, front.origin, z, planes, freq, ref, reference_field, section, sources, field, front.edges,
                       **kwargs)
