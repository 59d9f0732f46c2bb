"""Field analysis: how the image changes across the field -- per field point (the rays of one source) and band of wavelengths the
tangential and the sagittal focus (astigmatism, field curvature), centroid and distortion, spot size and relative illumination,
reduced on the device from the position, weight and wavelength planes of one section of the ray storage in one call for all
fields and bands.

`Raytracer.field_analysis` has no counterpart in optrace.  Definition: DESIGN.md, "Field analysis".  Kernels: csrc/ot_field.hpp
behind `ot_field_*`; the bands are those of `huygens_stack` and `chromatic_analysis` (`psf.assign_bands`, `psf.settle_bands`),
assigned over the used rays of all chosen fields together.  The device's records do not depend on the plane: a ray is the line
origin_xy + a + (z - origin_z) m, the records hold the first and second moments of (a, m), and every figure on a plane `z` is
host arithmetic on them.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from . import chromatic as _chromatic
from . import psf as _psf
from . import wavefront as _wavefront
from .base import BaseClass, check_type

PARAXIAL = ("tma", None)


def check_arguments(nt: int, n_sources: int, sources, section, bands, z, reference, reference_field, paraxial):
    """Argument checks of `Raytracer.field_analysis`, host only; nt: sections per ray of the geometry, n_sources: ray sources there
    are.  -> (sources as a list, bands as `psf.check_bands` returns them, z and reference as floats or None)."""
    if sources is None:
        sources = list(range(n_sources))
        if not sources:
            raise RuntimeError("Ray Sources Missing.")
    else:
        check_type("sources", sources, (list, tuple, np.ndarray))
        sources = list(np.asarray(sources).tolist()) if isinstance(sources, np.ndarray) else list(sources)
        if not 1 <= len(sources) <= _capi.FIELD_MAX_FIELDS:
            raise ValueError(f"Property 'sources' needs to hold 1 to {_capi.FIELD_MAX_FIELDS} source indices, but holds {len(sources)}.")
        for s in sources:
            check_type("sources", s, int)
            if not 0 <= s < n_sources:
                raise IndexError(f"Invalid source index {s} in 'sources': there are {n_sources} ray sources.")
        if len(set(sources)) != len(sources):
            raise ValueError("Property 'sources' needs to hold distinct source indices.")
    if len(sources) > _capi.FIELD_MAX_FIELDS:
        raise ValueError(f"{len(sources)} ray sources, but a field analysis takes {_capi.FIELD_MAX_FIELDS} at the most: pass `sources`.")
    _wavefront.check_sphere_arguments(nt, section, None, None)
    bands = _psf.check_bands(bands)
    if z is not None:
        z = _wavefront._finite_number("z", z)
    if reference is not None:
        reference = _wavefront._finite_number("reference", reference)
    check_type("reference_field", reference_field, int)
    if not 0 <= reference_field < len(sources):
        raise IndexError(f"reference_field={reference_field} is no index into the {len(sources)} sources of the analysis.")
    if paraxial not in PARAXIAL:
        raise ValueError(f"Property 'paraxial' needs to be 'tma' or None, but is '{paraxial}'.")
    return sources, bands, z, reference


def directions(field):
    """field (F, 2) -> t (F, 2): its unit vectors, (0, 1) for a field on the axis (or without a direction)."""
    field = np.asarray(field, dtype=np.float64).reshape(-1, 2)
    t = np.tile([0.0, 1.0], (field.shape[0], 1))
    length = np.hypot(field[:, 0], field[:, 1])
    off = np.isfinite(length) & (length > 0)
    t[off] = field[off] / length[off, None]
    return t


class FieldAnalysis(BaseClass):
    """Result of `Raytracer.field_analysis`; lengths in mm, wavelengths in nm, powers in W.  F field points, K bands of wavelengths;
    arrays have the shape (F, K) unless said otherwise.

    sources (F): the ray sources that are the field points.  section: the section analysed.  band_edges (K + 1) or None for
    bands="lines".  records (F, K, 18): what the device returned (include/optrace_amd.h, ot_field_sums); origin (3): the point its
    lines refer to.  band_N, band_power: rays of a cell in the sums and their power; n_parallel: used rays that run within a plane
    z = const and are in none of them.  wavelengths (K): power-weighted mean per band over all fields.  reference_band: the band
    with rays whose mean wavelength lies nearest to `reference`, -1 when there is none; reference_field: the field the curvatures
    and the relative illumination refer to.
    field (F, 2): the source's x, y relative to the optical axis, its direction tangents where that is zero; t (F, 2): its unit
    vector, the tangential direction, (0, 1) on the axis.  focus_t, focus_s: z where the spot is narrowest along t and across it;
    focus_rms: z of the smallest RMS radius; NaN for fewer than two rays and for a collimated cell.  astigmatism: focus_t minus
    focus_s.  field_curvature_t, _s, _rms: the foci minus focus_rms of the reference field in the same band.
    z: the plane the spots are compared on.  centroid (F, K, 2): power-weighted mean of where a cell's rays cross it; rms_t, rms_s,
    rms_radius: RMS size about it along t, across it and in both, exactly 0 for one ray; rms_radius_best: rms_radius on the plane
    of the cell's own focus_rms.  transmission (F): power in the sums over the power the source emitted; relative_illumination
    (F): transmission over that of the reference field.  paraxial (F, K, 2): the paraxial image of the field point on the plane z,
    NaN where there is none; distortion: (centroid . h / |h| - |h|) / |h| with h = paraxial, both from the optical axis `axis` (2),
    NaN where |h| is 0.
    A cell without a ray has band_N = band_power = 0 and NaN elsewhere."""

    _tracked = False

    def __init__(self, records, origin, z: float, reference_band: int, reference_field: int, section: int, sources, field, power,
                 paraxial=None, band_edges=None, axis=(0.0, 0.0), **kwargs) -> None:
        super().__init__(**kwargs)
        self.sources = np.array(sources, dtype=np.int64).reshape(-1)
        F = self.sources.shape[0]
        if not 1 <= F <= _capi.FIELD_MAX_FIELDS:
            raise ValueError(f"1 to {_capi.FIELD_MAX_FIELDS} fields, but there are {F}.")
        rec = np.array(records, dtype=np.float64).reshape(F, -1, _capi.FIELD_M)
        K = rec.shape[1]
        if not 1 <= K <= _capi.CHROM_MAX_BANDS:
            raise ValueError(f"1 to {_capi.CHROM_MAX_BANDS} bands, but the records hold {K}.")
        self.records = rec
        self.origin = np.array(origin, dtype=np.float64).reshape(3)
        self.axis = np.array(axis, dtype=np.float64).reshape(2)
        self.band_edges = None if band_edges is None else np.array(band_edges, dtype=np.float64).reshape(-1)
        if self.band_edges is not None and self.band_edges.shape[0] != K + 1:
            raise ValueError(f"{K} bands need {K + 1} edges, but there are {self.band_edges.shape[0]}.")
        check_type("reference_band", reference_band, (int, np.integer))
        check_type("reference_field", reference_field, (int, np.integer))
        if not -1 <= reference_band < K:
            raise ValueError(f"Reference band {reference_band} out of range for {K} bands.")
        if not 0 <= reference_field < F:
            raise ValueError(f"Reference field {reference_field} out of range for {F} fields.")
        self.n_fields, self.n_bands, self.section, self.z = F, K, int(section), float(z)
        self.reference_band, self.reference_field = int(reference_band), int(reference_field)
        self.field = np.array(field, dtype=np.float64).reshape(F, 2)
        self.t = directions(self.field)
        power = np.array(power, dtype=np.float64).reshape(F)
        paraxial = np.full((F, K, 2), np.nan) if paraxial is None else np.array(paraxial, dtype=np.float64).reshape(F, K, 2)
        self.paraxial = paraxial

        self.band_N, self.band_power = rec[:, :, 1].astype(np.int64), rec[:, :, 0].copy()
        self.n_parallel = rec[:, :, 7].astype(np.int64)
        some, single, many = self.band_N > 0, self.band_N == 1, self.band_N > 1
        zeta = self.z - self.origin[2]
        tx, ty = self.t[:, 0:1], self.t[:, 1:2]
        with np.errstate(invalid="ignore", divide="ignore"):
            W = np.where(some, self.band_power, np.nan)
            Wk = rec[:, :, 0].sum(axis=0)
            self.wavelengths = np.where(self.band_N.sum(axis=0) > 0, rec[:, :, 6].sum(axis=0) / Wk, np.nan)

            def along(ux, uy):
                """The quadratic of the variance along the unit vector (ux, uy): A + 2 zeta C + zeta^2 V, times W."""
                A = ux * ux * rec[:, :, 8] + 2 * (ux * uy) * rec[:, :, 9] + uy * uy * rec[:, :, 10]
                Cc = ux * ux * rec[:, :, 11] + ux * uy * (rec[:, :, 12] + rec[:, :, 13]) + uy * uy * rec[:, :, 14]
                V = ux * ux * rec[:, :, 15] + 2 * (ux * uy) * rec[:, :, 16] + uy * uy * rec[:, :, 17]
                return A, Cc, V

            def focus(Cc, V):
                return np.where(many & (V > 0), self.origin[2] - Cc / V, np.nan)

            def rms(A, Cc, V, at):
                var = (A + 2 * at * Cc + at * at * V) / W
                return np.where(single, 0.0, np.sqrt(np.maximum(var, 0.0) + 0 * var))  # (NaN stays NaN)

            At, Ct, Vt = along(tx, ty)
            As, Cs, Vs = along(-ty, tx)
            Ar, Cr, Vr = rec[:, :, 8] + rec[:, :, 10], rec[:, :, 11] + rec[:, :, 14], rec[:, :, 15] + rec[:, :, 17]
            self.focus_t, self.focus_s, self.focus_rms = focus(Ct, Vt), focus(Cs, Vs), focus(Cr, Vr)
            self.astigmatism = self.focus_t - self.focus_s
            base = self.focus_rms[self.reference_field][None, :]
            self.field_curvature_t, self.field_curvature_s = self.focus_t - base, self.focus_s - base
            self.field_curvature_rms = self.focus_rms - base
            self.centroid = self.origin[:2] + (rec[:, :, 2:4] + zeta * rec[:, :, 4:6]) / W[:, :, None]
            self.rms_t, self.rms_s, self.rms_radius = rms(At, Ct, Vt, zeta), rms(As, Cs, Vs, zeta), rms(Ar, Cr, Vr, zeta)
            best = self.focus_rms - self.origin[2]
            self.rms_radius_best = np.where(np.isfinite(best), rms(Ar, Cr, Vr, np.where(np.isfinite(best), best, 0.0)), np.nan)
            self.transmission = self.band_power.sum(axis=1) / power
            self.relative_illumination = self.transmission / self.transmission[self.reference_field]
            hv = paraxial - self.axis
            h = np.hypot(hv[:, :, 0], hv[:, :, 1])
            h = np.where(h > 0, h, np.nan)
            self.distortion = (((self.centroid - self.axis) * hv).sum(axis=2) / h - h) / h
        self.lock()


def _empty(section: int, bands, z, origin, reference_field: int, sources, field, power, axis=(0.0, 0.0), **kwargs) -> FieldAnalysis:
    """(the rule of `spot._empty`: what the caller fixed stays; bands given as edges keep them, else one band without a ray)"""
    edges = bands if isinstance(bands, np.ndarray) else None
    K = 1 if edges is None else edges.shape[0] - 1
    rec = np.zeros((len(sources), K, _capi.FIELD_M))
    rec[:, :, 8:] = np.nan
    return FieldAnalysis(rec, origin, np.nan if z is None else z, -1, reference_field, section, sources, field, power, None, edges,
                         axis, **kwargs)


def paraxial_images(matrix_at, wavelengths, positions, tangents, z: float):
    """The paraxial image of every field point on the plane z per band: M[0, 0] pos_xy + M[0, 1] tangents, M = matrix_at(wl, source
    z, z), a 2 x 2 matrix or None where there is none.  -> (F, K, 2), NaN where there is no matrix."""
    F, K = len(positions), len(wavelengths)
    out = np.full((F, K, 2), np.nan)
    if matrix_at is None or not np.isfinite(z):
        return out
    for f in range(F):
        for b in range(K):
            if not np.isfinite(wavelengths[b]) or not np.all(np.isfinite(tangents[f])):
                continue
            M = matrix_at(float(wavelengths[b]), float(positions[f][2]), float(z))
            if M is not None:
                out[f, b] = M[0, 0] * np.asarray(positions[f][:2], dtype=np.float64) + M[0, 1] * np.asarray(tangents[f], dtype=np.float64)
    return out


class _Front:
    """What `band_records` hands on: the launch of `ot_field_sums` and what the host made of it."""
    __slots__ = ("R", "flat", "F", "lo", "key8", "K", "d_rec", "keep", "rec", "origin", "edges", "reference", "reference_band")


def band_records(rays, ranges, section: int, origin, bands, reference):
    """The front half of the analyses per field and band (`analyse` here, `mtf.analyse`): the used rays of the chosen fields as the
    kernels test them, their band keys, the `ot_field_sums` launch, `psf.settle_bands` and the reference band.  -> None when no ray
    is left in any band, else a `_Front`: R, flat, F, lo, key8, K, d_rec -- the arguments of the launch and the device tensor of
    its full records (F, K, 18) --, keep: the slice of the K bands that are left, rec = records[:, keep] on the host, origin as an
    array, edges, reference and reference_band.  Reads of the device: for "lines" the table of lines, 33 doubles, before the
    launches; one for the records (with the edges for a number of bands)."""
    import torch
    from ._device import require_device, ptr, stream_ptr
    lib = _capi.load_library()
    dev = require_device()
    some = [(a, n) for a, n in ranges if n > 0]
    if not some:
        return None
    F = len(ranges)
    lo, hi = min(a for a, _ in some), max(a + n for a, n in some)
    span = hi - lo
    nt, Np, k = int(rays.Nt), int(rays._Np), section
    R = rays._rays_struct(tail_only=k >= nt - 2)  # (addresses only: neither the index plane nor the polarisation planes are filled)
    st = stream_ptr()
    raw = lambda name: dict.__getitem__(rays._dev, name)  # (past the hook of `_dev`: no fill)
    p, w_k = raw("p"), raw("w")[Np * k + lo:Np * k + hi]
    wl = rays._dev["wl"][lo:hi]

    # the used rays of the chosen fields, as the kernels test them, for the bands' definition
    chosen = torch.zeros(span, dtype=torch.bool, device=dev)
    for a, n in some:
        chosen[a - lo:a - lo + n] = True
    L2 = torch.zeros(span, dtype=torch.float64, device=dev)
    for c in range(3):
        at = Np * (k + nt * c) + lo
        L2 += (p[at + Np:at + Np + span] - p[at:at + span]) ** 2
    live = chosen & (w_k > 0) & (L2 > 0)
    key, K_set, table = _psf.assign_bands(wl, live, bands)
    key8 = torch.where(key < K_set, key, _capi.CHROM_NO_BAND).to(torch.uint8)
    lines = isinstance(bands, str)
    K = K_set  # the bands of the launch
    if lines:  # (the table is read here, 33 doubles: the launch takes the lines there are, not the 32 the table has room for)
        table = table.cpu().numpy()
        K = max(1, min(int(table[0]), K_set))

    M = _capi.FIELD_M
    flat = (C.c_int64 * (2 * F))(*[int(v) for pair in ranges for v in pair])
    ws = torch.empty(max(1, lib.ot_field_workspace(flat, F, K)), dtype=torch.float64, device=dev)
    d_rec = torch.zeros(F * K * M, dtype=torch.float64, device=dev)
    origin = np.array(origin, dtype=np.float64)
    _capi.check(lib.ot_field_sums(C.byref(R), flat, F, k, ptr(key8), lo, K, (C.c_double * 3)(*origin), ptr(ws), ptr(d_rec), st))
    head = torch.cat([d_rec] + ([] if lines else [table])).cpu().numpy()
    rec, rest = head[:F * K * M].reshape(F, K, M), head[F * K * M:]
    table = table if lines else rest

    counts = np.zeros(K_set)
    counts[:K] = (rec[:, :, 1] + rec[:, :, 7]).sum(axis=0)
    starts = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    K_left, starts, edges = _psf.settle_bands(bands, K_set, starts, table)
    if not starts[-1]:
        return None
    # the bands that are left: the lines there are; or the last one, where an int asked for bands over a single wavelength
    keep = slice(K - 1, K) if not lines and K_left < K else slice(0, K_left)
    rec = rec[:, keep]
    with np.errstate(invalid="ignore", divide="ignore"):
        W = rec[:, :, 0].sum(axis=0)
        band_wl = table[1:1 + K_left] if lines else rec[:, :, 6].sum(axis=0) / W
        if reference is None:
            reference = rec[:, :, 6].sum() / W.sum()
    front = _Front()
    front.R, front.flat, front.F, front.lo, front.key8, front.K, front.d_rec = R, flat, F, lo, key8, K, d_rec
    front.keep, front.rec, front.origin, front.edges, front.reference = keep, rec, origin, edges, reference
    front.reference_band = _chromatic.reference_band(band_wl, rec[:, :, 1].sum(axis=0), reference)
    return front


def default_plane(front, reference_field: int, section: int, sources, field, power) -> float:
    """z of the plane the analyses compare on where none is given: the `focus_rms` of (reference field, reference band)."""
    ref = front.reference_band
    probe = FieldAnalysis(front.rec, front.origin, 0.0, ref, reference_field, section, sources, field, power, None, front.edges)
    z = float(probe.focus_rms[reference_field, ref]) if ref >= 0 else np.nan
    if not np.isfinite(z):
        raise RuntimeError("The rays of the reference field and band have no focus (a collimated bundle, a single ray, no ray?): "
                           "pass `z`.")
    return z


def analyse(rays, ranges, section: int, origin, bands, z, reference, reference_field: int, sources, field, power, positions,
            tangents, matrix_at, axis=(0.0, 0.0), **kwargs) -> FieldAnalysis:
    """Figures of the fields `ranges` [(first, count), ...] of the storage `rays` in section `section`; origin: the point the device
    refers the lines to; bands, z, reference as `check_arguments` returned them; sources, field, power, positions (relative to the
    optical axis `axis`), tangents: per field, what `FieldAnalysis` and `paraxial_images` take; matrix_at: see `paraxial_images`.  Reads the
    p, w and wl planes only.  Reads of the device: those of `band_records`.  The default `reference` is the power-weighted mean
    wavelength of the rays in the sums."""
    fixed = dict(origin=origin, reference_field=reference_field, sources=sources, field=field, power=power, axis=axis)
    front = band_records(rays, ranges, section, origin, bands, reference)
    if front is None:
        return _empty(section, bands, z, **fixed, **kwargs)
    rec, origin, edges, ref = front.rec, front.origin, front.edges, front.reference_band
    if z is None:
        z = default_plane(front, reference_field, section, sources, field, power)
    with np.errstate(invalid="ignore", divide="ignore"):
        W = rec[:, :, 0].sum(axis=0)
        mean_wl = np.where(rec[:, :, 1].sum(axis=0) > 0, rec[:, :, 6].sum(axis=0) / W, np.nan)
    parax = paraxial_images(matrix_at, mean_wl, positions, tangents, z) + np.asarray(axis, dtype=np.float64)
    return FieldAnalysis(rec, origin, z, ref, reference_field, section, sources, field, power, parax, edges, axis, **kwargs)
