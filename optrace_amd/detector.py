"""Detector stage on the GPU: section search, detector intersection, sphere projection.

Device implementation of Raytracer._hit_detector (raytracer.py:881-1051) through `ot_detector_hits_multi`, and of the
detector image through `ot_detector_images` and `ot_detector_image_auto_*`.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from dataclasses import dataclass

import numpy as np
import torch

from . import _capi
from ._device import require_device, stream_ptr, ptr, to_dev, f_order_flat, from_f_order, mailbox, sync_stream, alloc_retry


@dataclass(slots=True)
class DetectorRequest:
    """One (detector, position, ray range) request of the detector stage: made once by `Raytracer._detector_requests` from
    the keyword arguments of a public call and used as it is until `_requests` fills the C struct from it."""
    first: int                  # ray range; count None: the whole of whatever storage the request is launched on
    count: int
    surf: _capi.Surface         # the detector's surface at the position asked for (a detector may move on afterwards)
    projection: str             # sphere projection by name, None for a detector that is not spherical
    crop: np.ndarray            # [x0, x1, y0, y1] the hits are restricted to (hits outside: weight 0), None: automatic extent
    detector_index: int
    source_index: int           # None: all sources
    label: str                  # the detector's description at this position
    want_z: bool = False        # hit list with a z plane
    compact: bool = False       # hit list of the valid hits only, gathered at the front of its 1024 pieces
    weights_only: bool = False  # a compact list without positions (detector spectrum)
    extent: np.ndarray = None   # from here on the image grid of `detector_images` (`Raytracer._plan_renders`): fixed extent
    Nx: int = 0
    Ny: int = 0
    hist: torch.Tensor = None   # flat f64 device tensor of Ny * Nx * 4 entries that the hits are ADDED to
    weight_scale: float = 1.0   # every weight times this before it is added

    @property
    def proj_id(self) -> int:
        return _capi.PROJECTIONS[self.projection]

    @property
    def centre(self) -> np.ndarray:
        """the extent of an image no ray reaches: the detector's position (raytracer.py:1048-1049)"""
        x, y, _ = self.surf.pos
        return np.array([x, x, y, y])

    @property
    def image_label(self) -> str:
        """long_desc of an image or spot of these hits"""
        return self.label if self.source_index is None else f"Rays from RS{self.source_index} at {self.label}"


# What `detector_hits_multi` returns per request: ph flat f64 (x plane, y plane and, with want_z, z plane; None for
# weights_only), hw f32 weights, extent [x0, x1, y0, y1] of the valid hits (+-inf without one; None for a request with a crop),
# and for a compact list the hits' wavelengths and the fill counts of the pieces (both None for a dense list)
HitList = namedtuple("HitList", "ph hw extent ill_count wl fill")
# What `Raytracer._hit_detectors` returns per spec (fill: None for a dense list)
DetectorHits = namedtuple("DetectorHits", "xy w wl extent projection ill_count label fill")


def rays_for(rays, surfs) -> _capi.Rays:
    """The `ot_rays` of `rays` for a launch of the detector stage against the detector surfaces `surfs` (`_capi.Surface` at
    the positions asked for): THE rule for when the sections a trace left out (OT_DEFER_SECTIONS, everything before
    section nt - 2) need not be written first.  The section search of `ot_detector.hpp::detector_hit` reads a plane before
    nt - 2 only for a ray with z[nt - 2] >= z_min of its detector; every other ray is settled from the last two sections
    (`detector_hit_last`, the first branch of the search).  So no ray reads an early plane if all of this holds:
      - every detector's z_min lies behind the largest z_max of the tracing surfaces: at section nt - 2 a ray stands on
        the last surface, or rests where it was absorbed on an earlier one (a NaN position compares false as well);
      - the OUTLINE_INTERSECTION counters of the trace are all zero: a clipped ray rests somewhere on the outline box;
      - the storage has nt >= 3 (with fewer nothing is left out).
    The trace states the last two as `RayStorage._tail_z`.  Otherwise, and always once the sections are filled, the storage
    is complete when this returns.  A `TailStorage` has two sections and nothing to fill."""
    if not hasattr(rays, "_sections_stale"):
        return rays._rays_struct()
    z = rays._tail_z
    return rays._rays_struct(tail_only=z is not None and rays._nt >= 3 and all(float(s.z_min) > z for s in surfs))


def batches(requests: list):
    """The launches of a list of requests: grouped by ray range in order of first appearance, at most `_capi.DET_MAX` per
    launch.  -> (indices into `requests`, those requests) per launch."""
    groups: dict = {}
    for n, rq in enumerate(requests):
        groups.setdefault((rq.first, rq.count), []).append(n)
    for idx in groups.values():
        for b in range(0, len(idx), _capi.DET_MAX):
            part = idx[b:b + _capi.DET_MAX]
            yield part, [requests[n] for n in part]


def _requests(struct, requests: list, ill: torch.Tensor):
    """ctypes array of `struct` for `requests` with the fields every request type has: detector, projection, crop
    ([x0, x1, y0, y1] or NULL), ill_count (two counters per request in `ill`).  -> (array, the objects it points into)."""
    reqs = (struct * len(requests))()
    keep = []
    for k, rq in enumerate(requests):
        crop4 = None if rq.crop is None else (C.c_double * 4)(*(float(v) for v in rq.crop))
        keep.append((rq.surf, crop4))
        r = reqs[k]
        r.detector = C.addressof(rq.surf)
        r.projection = rq.proj_id
        r.crop4 = None if crop4 is None else C.addressof(crop4)
        r.ill_count = ill.data_ptr() + 16 * k
    return reqs, keep


def _ill_counts(ill: torch.Tensor, requests: list) -> np.ndarray:
    """(ill-conditioned, timed out) per request.  Closed-form hits can neither be ill-conditioned nor time out: read back
    (and wait) only where a detector needs the numeric hit search.  A timeout raises."""
    numeric = any(_capi.numeric_hit(rq.surf) for rq in requests)
    ill_h = ill.cpu().numpy() if numeric else np.zeros(2 * len(requests), dtype=np.int64)
    if ill_h[1::2].any():
        raise TimeoutError("Timeout after 200 iterations in hit finding. Try retracing.")
    return ill_h


def detector_hits_multi(rays, first: int, count: int, requests: list, extent_only: bool = False) -> list:
    """Hit search for several detectors (`DetectorRequest`, at most `_capi.DET_MAX`) in one pass over the ray sections
    (`ot_detector_hits_multi`).  A request without a crop also gets the extent of its valid hits; one with a crop has the
    hits outside come back with weight 0 (raytracer.py:1036-1040).  `extent_only`: no hit lists at all (`detector_extents`).
    -> `HitList` per request; the planes of a dense list have `count` entries each.  Binning and spectra use x and y only."""
    lib = _capi.load_library()
    dev = require_device()
    n = len(requests)
    # extents go straight to a pinned host buffer (plain stores of one small kernel), 4 doubles per request behind 2n unused
    # words; the ill-conditioned counts are device atomics and stay in device memory (read back for numeric detectors only)
    mb_t, mb = mailbox()
    mbf = mb.view(np.float64)
    ill = torch.zeros(2 * n, dtype=torch.int64, device=dev)
    reqs, keep = _requests(_capi.DetectorReq, requests, ill)
    outs = []
    for k, rq in enumerate(requests):
        want_z = rq.want_z and not extent_only
        compact = rq.compact and not want_z and not extent_only
        cap = _capi.HIT_PIECES * int(lib.ot_hit_piece_len(int(count))) if compact else count  # entries per plane
        no_pos = compact and rq.weights_only  # (detector spectrum: weights and wavelengths alone)
        if extent_only:
            ph = hw = wl_c = fill = None
        else:
            # (hit lists are the large allocations of this stage: out of memory -> the library's kept scratch goes back first)
            ph, hw, wl_c, fill = alloc_retry(lambda: (
                None if no_pos else torch.empty((3 if want_z else 2) * cap, dtype=torch.float64, device=dev),
                torch.empty(cap, dtype=torch.float32, device=dev),
                torch.empty(cap, dtype=torch.float32, device=dev) if compact else None,
                torch.zeros(_capi.HIT_PIECES, dtype=torch.int32, device=dev) if compact else None))
        ext = None
        if rq.crop is None:
            ext = 2 * n + 4 * k  # word offset in the mailbox
            mbf[ext:ext + 4] = [np.inf, -np.inf, np.inf, -np.inf]
        r = reqs[k]
        r.xy_only = 0 if want_z else 1
        r.ph, r.hw = (None if ph is None else ph.data_ptr()), (None if hw is None else hw.data_ptr())
        r.extent4 = mb_t.data_ptr() + 8 * ext if ext is not None else None
        r.wl_out, r.fill = (wl_c.data_ptr(), fill.data_ptr()) if compact else (None, None)
        outs.append((ph, hw, ext, wl_c, fill))
    rs = rays_for(rays, [rq.surf for rq in requests])
    _capi.check(lib.ot_detector_hits_multi(C.byref(rs), int(first), int(count), reqs, n, stream_ptr()))
    ill_h = _ill_counts(ill, requests)
    if any(o[2] is not None for o in outs):
        sync_stream()  # the mailbox is complete; no wait at all for closed-form detectors with user extents
    return [HitList(ph, hw, mbf[ext:ext + 4].copy() if ext is not None else None, int(ill_h[2 * k]), wl_c, fill)
            for k, (ph, hw, ext, wl_c, fill) in enumerate(outs)]


def detector_extents(rays, first: int, count: int, requests: list) -> list:
    """Extent of the valid hits of up to `_capi.DET_MAX` detectors (requests without a crop) in one pass over the ray sections,
    without hit lists (`ot_detector_hits_multi` with ph = hw = NULL): 52 B read per ray, nothing written.  The first half of
    an image with an automatic extent (raytracer.py:1042-1046); the second is `detector_images` with that extent.
    -> list of (extent4 numpy [x0, x1, y0, y1], +-inf without a hit; ill_count)."""
    return [(h.extent, h.ill_count) for h in detector_hits_multi(rays, first, count, requests, extent_only=True)]


def detector_extent_sample(rays, first: int, count: int, surf_desc: _capi.Surface, projection: int,
                           stride: int) -> np.ndarray:
    """Extent [x0, x1, y0, y1] (+-inf without a hit) of the hits of every `stride`-th wave of 64 rays
    (`ot_detector_extent_sample`): a box inside the automatic extent of raytracer.py:1042-1046, for ~1 / stride of the
    bytes."""
    lib = _capi.load_library()
    require_device()
    mb_t, mb = mailbox()
    rs = rays_for(rays, [surf_desc])
    _capi.check(lib.ot_detector_extent_sample(C.byref(rs), int(first), int(count), C.byref(surf_desc), int(projection),
                                              int(stride), C.c_void_p(mb_t.data_ptr()), stream_ptr()))
    return mb.view(np.float64)[:4].copy()  # (the call waits for the stream)


class AutoImage:
    """Detector image with an automatic extent in one pass over the ray sections (`ot_detector_image_auto_*`): the hits
    are sorted into the tiles of a provisional grid, the exact extent comes back, `finish` bins into the final grid.  For
    detectors with `_capi.fused_ok`: closed-form hit (flat, conic / spherical), no sphere projection with transcendentals.

    grid: (X0, Y0, tile_w, tile_h, tiles_x, tiles_y).  After construction: extent (numpy, +-inf without a hit),
    escaped (hits outside the grid) and escape_capacity; `finish` or `cancel` must follow."""

    def __init__(self, rays, first: int, count: int, surf_desc: _capi.Surface, projection: int, grid: tuple) -> None:
        self._lib = _capi.load_library()
        require_device()
        mb_t, mb = mailbox()
        rs = rays_for(rays, [surf_desc])
        origin = (C.c_double * 2)(float(grid[0]), float(grid[1]))
        tile = (C.c_double * 2)(float(grid[2]), float(grid[3]))
        tiles = (C.c_int32 * 2)(int(grid[4]), int(grid[5]))
        self._handle = C.c_void_p()
        _capi.check(self._lib.ot_detector_image_auto_begin(C.byref(rs), int(first), int(count), C.byref(surf_desc),
                                                           int(projection), origin, tile, tiles,
                                                           C.c_void_p(mb_t.data_ptr()), C.byref(self._handle),
                                                           stream_ptr()))
        res = mb.view(np.float64)[:6].copy()  # (the call waits for the stream)
        self.extent = res[:4]
        self.escaped = int(res[4])
        self.escape_capacity = int(res[5])

    def finish(self, extent, Nx: int, Ny: int, hist: torch.Tensor) -> None:
        """Add the image to hist (flat f64 device tensor of Ny * Nx * 4 entries); extent = the fixed image extent."""
        h, self._handle = self._handle, C.c_void_p()
        ext = (C.c_double * 4)(*[float(v) for v in extent])
        _capi.check(self._lib.ot_detector_image_auto_finish(h, ext, int(Nx), int(Ny), ptr(hist), stream_ptr()))

    def cancel(self) -> None:
        if self._handle:
            self._lib.ot_detector_image_auto_cancel(self._handle)
            self._handle = C.c_void_p()

    def __del__(self):
        try:
            self.cancel()
        except Exception:
            pass


def detector_images(rays, first: int, count: int, requests: list) -> list:
    """Hit search and binning fused (`ot_detector_images`) for detector images whose extent is known beforehand.

    requests: `DetectorRequest` (at most `_capi.DET_MAX`) with crop (the user or automatic extent the hits are restricted
    to) and the image grid: extent, Nx, Ny, hist, weight_scale.  -> ill-conditioned count per request."""
    lib = _capi.load_library()
    dev = require_device()
    n = len(requests)
    ill = torch.zeros(2 * n, dtype=torch.int64, device=dev)
    reqs, keep = _requests(_capi.DetectorImageReq, requests, ill)
    for k, rq in enumerate(requests):
        r = reqs[k]
        r.Nx, r.Ny = int(rq.Nx), int(rq.Ny)
        r.extent[:] = [float(v) for v in rq.extent]
        r.hist = rq.hist.data_ptr()
        r.weight_scale = float(rq.weight_scale)
    rs = rays_for(rays, [rq.surf for rq in requests])
    _capi.check(lib.ot_detector_images(C.byref(rs), int(first), int(count), reqs, n, stream_ptr()))
    return [int(v) for v in _ill_counts(ill, requests)[0::2]]  # (no read-back, no sync for closed-form detectors)


def project_points(surf_desc: _capi.Surface, p: np.ndarray, projection: int) -> np.ndarray:
    """SphericalSurface.sphere_projection (spherical_surface.py:36-97) via `ot_sphere_projection`."""
    lib = _capi.load_library()
    dev = require_device()
    n = int(np.shape(p)[0])
    dp = to_dev(f_order_flat(p), np.float64)
    out = torch.empty(3 * n, dtype=torch.float64, device=dev)
    _capi.check(lib.ot_sphere_projection(C.byref(surf_desc), int(projection), n, ptr(dp), ptr(out), stream_ptr()))
    return from_f_order(out, n, 3).copy()
