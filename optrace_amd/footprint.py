"""Beam footprints: per section of a stored trace the rays alive and arriving, their power, and where the living ones cross
the surface, reduced on the device from the position and weight planes.

`Raytracer.footprints` has no counterpart in optrace, where these numbers are formed in NumPy from `rays.p_list` and
`rays.w_list`; here that would bring the whole ray storage to the host.  Kernels: csrc/ot_footprint.hpp behind `ot_footprint_*`.
"""
from __future__ import annotations

import numpy as np

from . import _capi
from .base import BaseClass, check_type, check_not_below, check_not_above
from .image import ScalarImage


def check_arguments(source_index, n_px) -> None:
    """Argument checks of `Raytracer.footprints`, host only."""
    if source_index is not None:
        check_type("source_index", source_index, int)
    if n_px is not None:
        check_type("n_px", n_px, int)
        check_not_below("n_px", n_px, 1)
        check_not_above("n_px", n_px, _capi.FP_MAX_PX)


def surface_radius(surface) -> float:
    """Largest xy distance of a surface's outline from its `pos`: r for round surfaces, half the diagonal for rectangular ones."""
    from .geometry.surfaces import RectangularSurface
    if isinstance(surface, RectangularSurface):
        return float(np.hypot(surface.dim[0], surface.dim[1]) / 2)
    return float(surface.r)


class Footprints(BaseClass):
    """Result of `Raytracer.footprints`: arrays over the nt sections of the trace -- section 0 the sources, section i the space
    behind tracing surface i - 1, the last one the rays' ends.  Lengths in mm, powers in W.

    labels: source, element and side per surface, "end" for the last section.  N, power: rays alive in the section and their
    power; N_in, power_in: rays that arrived at its surface and their power (section 0: the same as alive); loss = power_in -
    power; transmission = power / power_in, NaN where nothing arrives.  centroid (nt, 3): power-weighted mean of where the
    living rays cross the surface; extent (nt, 6): x0, x1, y0, y1, z0, z1 of those points; rms_x, rms_y, rms_radius, cov_xy:
    second moments about the centroid; max_radius: largest xy distance from `axis` (nt, 2), the xy of the surface's position.
    surface_radius: largest xy distance of the surface's outline from its position, NaN for the first and the last section;
    fill = max_radius / surface_radius.  total_transmission: power behind the last surface over the power of the sources.
    A section without a living ray has N = power = 0 and NaN geometry; one with a single ray has RMS figures of exactly 0.
    records (nt, 17): what the device returned (include/optrace_amd.h, ot_footprint_moments)."""

    _tracked = False

    def __init__(self, records, labels, axis, surface_radius, maps=None, **kwargs) -> None:
        super().__init__(**kwargs)
        rec = np.array(records, dtype=np.float64).reshape(-1, _capi.FP_M)
        nt = rec.shape[0]
        if nt < 2:
            raise ValueError(f"A trace has at least 2 sections, but the records hold {nt}.")
        self.records = rec
        self.labels = tuple(str(name) for name in labels)
        self.axis = np.array(axis, dtype=np.float64).reshape(nt, 2)
        self.surface_radius = np.array(surface_radius, dtype=np.float64).reshape(nt)
        if len(self.labels) != nt:
            raise ValueError(f"{nt} sections, but {len(self.labels)} labels.")
        self.N, self.N_in = rec[:, 1].astype(np.int64), rec[:, 3].astype(np.int64)
        self.power, self.power_in = rec[:, 0].copy(), rec[:, 2].copy()
        self.loss = self.power_in - self.power
        alive, single = self.N > 0, self.N == 1
        with np.errstate(invalid="ignore", divide="ignore"):
            W = np.where(alive, self.power, np.nan)
            self.transmission = np.where(self.N_in > 0, self.power / self.power_in, np.nan)
            self.centroid = rec[:, 4:7] / W[:, None]
            # (one ray is its own centroid: w x / w need not return x to the last bit, the figures say so exactly)
            self.rms_x = np.where(single, 0.0, np.sqrt(rec[:, 13] / W))
            self.rms_y = np.where(single, 0.0, np.sqrt(rec[:, 14] / W))
            self.cov_xy = np.where(single, 0.0, rec[:, 15] / W)
            self.total_transmission = float(self.power[nt - 2] / self.power[0]) if self.power[0] > 0 else float("nan")
        self.rms_radius = np.sqrt(self.rms_x ** 2 + self.rms_y ** 2)
        self.extent = np.where(alive[:, None], rec[:, 7:13], np.nan)
        self.max_radius = np.where(alive, np.sqrt(rec[:, 16]), np.nan)
        self.fill = self.max_radius / self.surface_radius
        self.maps = None
        if maps is not None:
            self.maps = np.array(maps, dtype=np.float64)
            if self.maps.ndim != 3 or self.maps.shape[0] != nt or self.maps.shape[1] != self.maps.shape[2]:
                raise ValueError(f"Property 'maps' needs the shape ({nt}, n_px, n_px), but has {self.maps.shape}.")
        self.lock()

    def image(self, i: int) -> ScalarImage:
        """Power map of the footprint of section i over `axis[i]` +- `max_radius[i]` (W per cell)."""
        if self.maps is None:
            raise ValueError("No maps: call Raytracer.footprints with n_px.")
        check_type("i", i, (int, np.integer))
        nt = len(self.labels)
        if not -nt <= i < nt:
            raise IndexError(f"Section {i} out of range for {nt} sections.")
        i %= nt
        R = self.max_radius[i]
        R = float(R) if R > 0 else 1.0  # (no ray, or all in one place: a cell of some size about the axis)
        ax, ay = (float(a) for a in self.axis[i])
        return ScalarImage(self.maps[i].copy(), extent=[ax - R, ax + R, ay - R, ay + R], quantity="Power",
                           long_desc=f"Footprint {self.labels[i]}" + (f" of {self.long_desc}" if self.long_desc else ""))


def analyse(rays, first: int, count: int, axis, n_px, labels, surface_radius, **kwargs) -> Footprints:
    """Footprints of the rays [first, first + count) of the storage `rays`.  axis: (nt, 2), the xy the largest radius and the maps
    refer to; n_px: cells per side of the maps or None; labels, surface_radius: handed on to `Footprints`."""
    import ctypes as C
    import torch
    from ._device import require_device, ptr, stream_ptr, to_dev
    lib = _capi.load_library()
    dev = require_device()
    nt, M = int(rays.Nt), _capi.FP_M
    axis = np.array(axis, dtype=np.float64).reshape(nt, 2)
    cells = n_px * n_px if n_px else 0
    if count < 1:  # (no launch: the records of sections without a ray)
        rec = np.zeros((nt, M))
        rec[:, 7:13] = np.nan
        return Footprints(rec, labels, axis, surface_radius, np.zeros((nt, n_px, n_px)) if n_px else None, **kwargs)
    R = rays._rays_struct()  # (addresses only: neither the index plane nor the polarisation planes are filled)
    st = stream_ptr()
    d_axis = to_dev(axis, np.float64)
    ws = torch.empty(max(1, lib.ot_footprint_workspace(count, nt)), dtype=torch.float64, device=dev)
    rec = torch.zeros(nt * M, dtype=torch.float64, device=dev)
    _capi.check(lib.ot_footprint_moments(C.byref(R), first, count, ptr(d_axis), ptr(ws), ptr(rec), st))
    maps = None
    if n_px:
        maps = torch.zeros(nt * cells, dtype=torch.float64, device=dev)
        _capi.check(lib.ot_footprint_maps(C.byref(R), first, count, ptr(d_axis), ptr(rec), n_px, ptr(maps), st))
        maps = maps.cpu().numpy().reshape(nt, n_px, n_px)
    return Footprints(rec.cpu().numpy(), labels, axis, surface_radius, maps, **kwargs)
