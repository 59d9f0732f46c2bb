"""Spot diagrams: where the rays of every field point (the rays of one source) and band of wavelengths land on a plane and on planes
either side of it -- a matrix of power maps at one common scale, binned on the device from the position, weight and wavelength
planes of one section of the ray storage in one call for all fields, bands and planes.

`Raytracer.spot_diagram` has no counterpart in optrace.  Definition: DESIGN.md, "Spot diagrams".  Kernels: csrc/ot_spot_diagram.hpp
behind `ot_spotdiag_extent` and `ot_spotdiag_maps`; fields, bands, used rays and ray lines are those of the field analysis
(`field.band_records`), whose records give the centres the tiles are drawn about.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from . import field as _field
from .base import BaseClass, check_type
from .image import ScalarImage

CENTRES = ("centroid", "band", "reference")
# The default side of a tile: SIZE_FACTOR times the largest distance R of a used ray from its centre.  A ray has |e_x| <= R (1 + 3u),
# u = 2^-53 (the squares, their sum and the root round once each), so with size = 2 R (1 + 2^-32) the product e_x * scale is at most
# n_px / 2 (1 - 2^-33) in magnitude after its two roundings, and e_x * scale + half lies in [2^-34 n_px, n_px (1 - 2^-34)] -- an ulp of
# n_px is 2^-52 n_px at the most: the floor lies in [0, n_px) for every used ray, by the arithmetic of the definition.
SIZE_FACTOR = 2.0 * (1.0 + 2.0 ** -32)
R2_MIN = 1e-280  # (a largest squared distance below this has lost its relative accuracy to underflow: no extent to scale by)


def check_arguments(n_px, size, centre, n_sources: int):
    """Argument checks of `Raytracer.spot_diagram` beyond those of `field.check_arguments` and `mtf.check_arguments` (dz), host
    only; n_sources: the fields of the analysis.  -> (n_px, size as a float or None, centre as a name or a float64 array (F, 2))."""
    check_type("n_px", n_px, (int, np.integer))
    if isinstance(n_px, bool) or not 1 <= n_px <= _capi.SD_MAX_PX:
        raise ValueError(f"Property 'n_px' needs to be an int from 1 to {_capi.SD_MAX_PX}, but is {n_px}.")
    if size is not None:
        check_type("size", size, (int, float, np.integer, np.floating))
        size = float(size)
        if not np.isfinite(size) or not size > 0:
            raise ValueError(f"Property 'size' needs to be finite and above 0, but is {size}.")
    check_type("centre", centre, (str, list, tuple, np.ndarray))
    if isinstance(centre, str):
        if centre not in CENTRES:
            raise ValueError(f"Property 'centre' needs to be one of {CENTRES} or an array (F, 2), but is '{centre}'.")
    else:
        c = np.asarray(centre)
        if c.size and not (np.issubdtype(c.dtype, np.floating) or np.issubdtype(c.dtype, np.integer)):
            raise TypeError(f"Property 'centre' needs to hold real numbers, but holds {c.dtype}.")
        centre = np.array(c, dtype=np.float64)
        if centre.shape != (n_sources, 2):
            raise ValueError(f"Property 'centre' needs the shape ({n_sources}, 2), a point per field, but has {centre.shape}.")
        if not np.all(np.isfinite(centre)):
            raise ValueError("Property 'centre' needs to hold finite values only.")
    return int(n_px), size, centre


def check_cap(F: int, K: int, Z: int, n_px: int) -> None:
    """The limit of `ot_spotdiag_maps` on the cells of all tiles, said before anything of that size is asked of the device."""
    if F * K * Z * n_px * n_px > _capi.SD_MAX_CELLS:
        raise RuntimeError(f"{F} fields x {K} bands x {Z} planes x {n_px}^2 cells are more than {_capi.SD_MAX_CELLS} doubles on the "
                           "device: ask for fewer fields, bands, planes or cells per call.")


def centres(rec, zeta, centre, reference_band: int, origin_xy):
    """The point every tile is drawn about, relative to `origin_xy`, from the records (F, K, 18) of `ot_field_sums` in f64:
    (slot 2..3 + zeta slot 4..5) / slot 0 of the band ("band"), of the reference band ("reference"), the sums of numerator and
    denominator over the bands first ("centroid"); or the array (F, 2) of absolute points less `origin_xy`, on every plane.
    -> (F, K, Z, 2); NaN where the quotient has no ray behind it."""
    rec, zeta = np.asarray(rec, dtype=np.float64), np.asarray(zeta, dtype=np.float64)
    F, K, Z = rec.shape[0], rec.shape[1], zeta.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        num = rec[:, :, None, 2:4] + zeta[None, None, :, None] * rec[:, :, None, 4:6]  # (F, K, Z, 2)
        den = rec[:, :, None, 0:1]                                                     # (F, K, 1, 1)
        if isinstance(centre, str):
            if centre == "band":
                out = num / den
            elif centre == "reference":
                out = num[:, reference_band:reference_band + 1] / den[:, reference_band:reference_band + 1] if reference_band >= 0 \
                    else np.full((F, 1, Z, 2), np.nan)
            else:
                out = num.sum(axis=1, keepdims=True) / den.sum(axis=1, keepdims=True)
        else:
            out = (np.asarray(centre, dtype=np.float64) - np.asarray(origin_xy, dtype=np.float64))[:, None, None, :]
    return np.ascontiguousarray(np.broadcast_to(out, (F, K, Z, 2)))


class SpotDiagram(BaseClass):
    """Result of `Raytracer.spot_diagram`; lengths in mm, wavelengths in nm, powers in W.  F field points, K bands of wavelengths,
    Z planes; arrays have the shape (F, K, Z) unless said otherwise.

    sources (F), section, band_edges (K + 1) or None for bands="lines", wavelengths (K), reference_band, reference_field, field
    (F, 2), t (F, 2), records (F, K, 18), origin (3), z, planes (Z), band_N, band_power (F, K): as in `MTFAnalysis`.
    n_px: cells per side of every tile; size: the side of every tile, the same for all.  centre (F, K, Z, 2): the absolute point
    every tile is drawn about; centre_rel: the same relative to origin_xy, as the device was given it.
    power (F, K, Z, n_px, n_px): W per cell, row from y, column from x, row 0 the lowest y; N: rays binned; outside_N,
    outside_power: rays that fall outside the tile and their power -- nothing is clamped into the map.  geo_radius: largest distance
    of a ray from the centre; rms_radius: sqrt(sum w |e|^2 / sum w) about the centre.  power_all (F, Z, n_px, n_px): the sum over
    the bands.
    A cell without a ray has zeros in the maps and counts and NaN in the radii and the centre."""

    _tracked = False

    def __init__(self, power, counts, outside_power, extents, centre_rel, records, origin, z: float, planes, n_px: int, size: float,
                 reference_band: int, reference_field: int, section: int, sources, field, band_edges=None, **kwargs) -> None:
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
        Z = self.planes.shape[0]
        if not 1 <= Z <= _capi.MTF_MAX_PLANES:
            raise ValueError(f"1 to {_capi.MTF_MAX_PLANES} planes, but there are {Z}.")
        check_type("n_px", n_px, (int, np.integer))
        if not 1 <= n_px <= _capi.SD_MAX_PX:
            raise ValueError(f"1 to {_capi.SD_MAX_PX} cells per side, but n_px is {n_px}.")
        self.n_px, self.size = int(n_px), float(size)
        if not (np.isnan(self.size) or (np.isfinite(self.size) and self.size > 0)):  # (NaN: the empty result without a size)
            raise ValueError(f"A finite size above 0, but it is {size}.")
        self.power = np.array(power, dtype=np.float64).reshape(F, K, Z, self.n_px, self.n_px)
        counts = np.array(counts).astype(np.int64).reshape(F, K, Z, 2)
        self.N, self.outside_N = counts[..., 0].copy(), counts[..., 1].copy()
        self.outside_power = np.array(outside_power, dtype=np.float64).reshape(F, K, Z)
        self.extents = np.array(extents, dtype=np.float64).reshape(F, K, Z, 2)
        self.centre_rel = np.array(centre_rel, dtype=np.float64).reshape(F, K, Z, 2)
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
        self.n_fields, self.n_bands, self.n_planes = F, K, Z
        self.section, self.z = int(section), float(z)
        self.reference_band, self.reference_field = int(reference_band), int(reference_field)
        self.field = np.array(field, dtype=np.float64).reshape(F, 2)
        self.t = _field.directions(self.field)

        self.band_N, self.band_power = rec[:, :, 1].astype(np.int64), rec[:, :, 0].copy()
        some = (self.band_N > 0)[:, :, None]
        with np.errstate(invalid="ignore", divide="ignore"):
            Wk = rec[:, :, 0].sum(axis=0)
            self.wavelengths = np.where(self.band_N.sum(axis=0) > 0, rec[:, :, 6].sum(axis=0) / Wk, np.nan)
            self.centre = np.where(some[..., None], self.origin[:2] + self.centre_rel, np.nan)
            self.geo_radius = np.where(some, np.sqrt(self.extents[..., 0]), np.nan)
            self.rms_radius = np.where(some, np.sqrt(self.extents[..., 1] / self.band_power[:, :, None]), np.nan)
        self.power_all = self.power.sum(axis=1)
        self.lock()

    def _tile(self, field, plane):
        for name, v, n in (("field", field, self.n_fields), ("plane", plane, self.n_planes)):
            check_type(name, v, (int, np.integer))
            if not -n <= v < n:
                raise IndexError(f"{name} {v} out of range for {n}.")
        return field % self.n_fields, plane % self.n_planes

    def image(self, field: int, plane: int, band: int = None) -> ScalarImage:
        """Power map of one tile over its centre +- size / 2 (W per cell); band=None: all bands of the field on that plane,
        `power_all`, about the mean of the band centres weighted by band power."""
        f, j = self._tile(field, plane)
        if band is None:
            W = np.where(self.band_N[f] > 0, self.band_power[f], 0.0)
            c = np.where(self.band_N[f, :, None] > 0, self.centre[f, :, j], 0.0)
            with np.errstate(invalid="ignore", divide="ignore"):
                c = (W[:, None] * c).sum(axis=0) / W.sum()
            data, what = self.power_all[f, j], "all bands"
        else:
            check_type("band", band, (int, np.integer))
            if not -self.n_bands <= band < self.n_bands:
                raise IndexError(f"band {band} out of range for {self.n_bands}.")
            band %= self.n_bands
            c, data, what = self.centre[f, band, j], self.power[f, band, j], f"band {band}"
        if not np.all(np.isfinite(c)) or not np.isfinite(self.size):
            raise ValueError(f"Field {f}, {what}, plane {j}: no ray, no centre to draw the tile about.")
        h = self.size / 2
        return ScalarImage(data.copy(), extent=[c[0] - h, c[0] + h, c[1] - h, c[1] + h], quantity="Power",
                           long_desc=f"Spot of field {f}, {what}, z = {self.planes[j]:.6g} mm" + (f" of {self.long_desc}" if self.long_desc else ""))

    def matrix(self, band: int = None) -> ScalarImage:
        """All tiles of one band (None: `power_all`) in one image: fields in rows, field 0 at the bottom, planes in columns; tile
        (f, j) covers x from j size to (j + 1) size and y from f size to (f + 1) size."""
        if band is None:
            tiles = self.power_all
        else:
            check_type("band", band, (int, np.integer))
            if not -self.n_bands <= band < self.n_bands:
                raise IndexError(f"band {band} out of range for {self.n_bands}.")
            tiles = self.power[:, band % self.n_bands]
        if not np.isfinite(self.size):
            raise ValueError("No size: the diagram holds no ray.")
        F, Z, n = self.n_fields, self.n_planes, self.n_px
        data = tiles.transpose(0, 2, 1, 3).reshape(F * n, Z * n)  # (row 0 the lowest y: field 0 at the bottom)
        return ScalarImage(data.copy(), extent=[0.0, Z * self.size, 0.0, F * self.size], quantity="Power",
                           long_desc="Spot diagram" + (f", band {band}" if band is not None else "") + (f" of {self.long_desc}" if self.long_desc else ""))


def _empty(section: int, bands, z, dz, n_px: int, size, origin, reference_field: int, sources, field, **kwargs) -> SpotDiagram:
    """(the rule of `mtf._empty`: what the caller fixed stays; bands given as edges keep them, else one band without a ray; no size
    given: NaN)"""
    edges = bands if isinstance(bands, np.ndarray) else None
    K = 1 if edges is None else edges.shape[0] - 1
    F, Z = len(sources), dz.shape[0]
    rec = np.zeros((F, K, _capi.FIELD_M))
    rec[:, :, 8:] = np.nan
    z = np.nan if z is None else z
    return SpotDiagram(np.zeros((F, K, Z, n_px, n_px)), np.zeros((F, K, Z, 2), dtype=np.int64), np.zeros((F, K, Z)), np.zeros((F, K, Z, 2)),
                       np.full((F, K, Z, 2), np.nan), rec, origin, z, z + dz, n_px, np.nan if size is None else size, -1, reference_field,
                       section, sources, field, edges, **kwargs)


def analyse(rays, ranges, section: int, origin, bands, z, dz, n_px: int, size, centre, reference, reference_field: int, sources, field,
            power, **kwargs) -> SpotDiagram:
    """Spot diagram of the fields `ranges` [(first, count), ...] of the storage `rays` in section `section`; origin, bands, z,
    reference, sources, field, power: as for `field.analyse`; dz: as `mtf.check_arguments` returned it; n_px, size, centre: as
    `check_arguments` returned them.  Reads the p, w and wl planes only.  Reads of the device: those of `field.band_records` -- the
    records give the default z and the centres --, one for the extents, which give the default size, and one for the maps."""
    import torch
    from ._device import require_device, ptr, stream_ptr, to_dev
    lib = _capi.load_library()
    dev = require_device()
    fixed = dict(origin=origin, reference_field=reference_field, sources=sources, field=field)
    # (the fewest bands there can be: the lines are counted on the device, edges and a number say it themselves)
    check_cap(len(sources), 1 if isinstance(bands, str) else bands.shape[0] - 1 if isinstance(bands, np.ndarray) else int(bands),
              int(dz.shape[0]), n_px)
    front = _field.band_records(rays, ranges, section, origin, bands, reference)
    if front is None:
        return _empty(section, bands, z, dz, n_px, size, **fixed, **kwargs)
    ref = front.reference_band
    if z is None:
        z = _field.default_plane(front, reference_field, section, sources, field, power)
    planes = z + dz
    zeta = planes - front.origin[2]
    F, K, Z = front.F, front.K, int(dz.shape[0])
    check_cap(F, K, Z, n_px)
    # the centres of the bands of the launch: those that are left from the records, the others hold no ray
    rel = np.full((F, K, Z, 2), np.nan)
    rel[:, front.keep] = centres(front.rec, zeta, centre, ref, front.origin[:2])
    d_centre = to_dev(rel.reshape(-1), np.float64)
    org, c_zeta = (C.c_double * 3)(*front.origin), (C.c_double * Z)(*zeta)
    ws = torch.empty(max(1, lib.ot_spotdiag_workspace(front.flat, F, K, Z)), dtype=torch.float64, device=dev)
    d_ext = torch.zeros(F * K * Z * 2, dtype=torch.float64, device=dev)
    _capi.check(lib.ot_spotdiag_extent(C.byref(front.R), front.flat, F, section, ptr(front.key8), front.lo, K, org, ptr(d_centre), c_zeta,
                                       Z, ptr(ws), ptr(d_ext), stream_ptr()))
    ext = d_ext.cpu().numpy().reshape(F, K, Z, 2)[:, front.keep]
    if size is None:
        r2 = float(np.nanmax(np.where(front.rec[:, :, 1, None] > 0, ext[..., 0], 0.0), initial=0.0))
        if not (np.isfinite(r2) and r2 > R2_MIN):
            raise ValueError("No used ray lies away from the centre of its tile (a single ray, no ray, a perfect focus?), or one lies "
                             "beyond every scale: pass `size`.")
        size = SIZE_FACTOR * float(np.sqrt(r2))
        if not np.isfinite(size):
            raise ValueError("The rays lie too far from their centres for a common scale: pass `size`.")
    cells = F * K * Z * n_px * n_px
    d_maps = torch.zeros(cells + F * K * Z, dtype=torch.float64, device=dev)  # the maps, then the power outside
    d_counts = torch.zeros(F * K * Z * 2, dtype=torch.int64, device=dev)
    _capi.check(lib.ot_spotdiag_maps(C.byref(front.R), front.flat, F, section, ptr(front.key8), front.lo, K, org, ptr(d_centre), c_zeta, Z,
                                     n_px, size, ptr(d_maps), ptr(d_counts), ptr(d_maps[cells:]), stream_ptr()))
    got = d_maps.cpu().numpy()
    maps, out_w = got[:cells].reshape(F, K, Z, n_px, n_px)[:, front.keep], got[cells:].reshape(F, K, Z)[:, front.keep]
    counts = d_counts.cpu().numpy().reshape(F, K, Z, 2)[:, front.keep]
    return SpotDiagram(maps, counts, out_w, ext, rel[:, front.keep], front.rec, front.origin, z, planes, n_px, size, ref, reference_field,
                       section, sources, field, front.edges, **kwargs)
