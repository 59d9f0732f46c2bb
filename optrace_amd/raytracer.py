"""Raytracer: sequential tracing of a scene on one MI355X (or one per rank).

Mirror of optrace/tracer/raytracer.py:28-1279 for the hot path named in BASELINE.json:
`trace` (ray generation, all surface interactions, section stores, counters), `detector_image`
(detector hit search + binning) and `iterative_render`.  The object keeps the reference's API; the work
happens in HIP kernels reached through the C-ABI (include/optrace_amd.h):

    trace(N)          -> ot_generate_and_trace   (one fused launch: generation + every surface)
    detector_image()  -> ot_detector_images      (known extent: hit search and binning in one pass)
                         ot_detector_image_auto_begin / _finish  (automatic extent, long bundles: one pass)
                         ot_detector_hits_multi + ot_render_accumulate  (otherwise: hit list, then binning)

Geometry validation (element order, collisions) is one-off host work per trace and stays in NumPy.
"""
from __future__ import annotations

import ctypes as C
from enum import IntEnum
from typing import Any

import numpy as np
import torch

from . import _capi
from . import base as _base
from .base import check_type
from .geometry.elements import Group, Detector
from .geometry.surfaces import Surface, Point, Line, SphericalSurface, RingSurface, SlitSurface
from .options import global_options
from .ray_storage import RayStorage, TailStorage, SceneRef
from .refraction_index import RefractionIndex
from .render_image import RenderImage
from .spectrum import LightSpectrum
from . import spot as _spot
from .spot import SpotAnalysis
from . import wavefront as _wavefront
from .wavefront import WavefrontAnalysis
from . import psf as _psf
from .psf import HuygensPSF, HuygensStack
from . import footprint as _footprint
from .footprint import Footprints
from . import chromatic as _chromatic
from .chromatic import ChromaticAnalysis
from . import field as _field
from .field import FieldAnalysis
from . import mtf as _mtf
from .mtf import MTFAnalysis
from . import spot_diagram as _spot_diagram
from .spot_diagram import SpotDiagram
from . import wavefront_field as _wavefront_field
from .wavefront_field import WavefrontField
from . import psf_field as _psf_field
from .psf_field import HuygensField
from . import fans as _fans
from .fans import RayFans
from .geometry.ray_source import RaySource
from .scene import CompiledScene, SectionTable, tracing_elements
from ._device import require_device, stream_ptr, ptr, alloc_retry, mailbox
from ._warn import warning
from . import detector as _detector
from . import checks as _checks


class _TraceRecord:
    """What a full trace established, valid while `Raytracer._scene_unchanged()`.  The slow path of `trace` drops it as a
    whole: no split, range record or book-keeping of render-only traces outlives a change of the scene."""
    __slots__ = ("epoch", "structure", "snap", "scene", "watch", "splits", "ranges", "book", "z_last")

    def __init__(self, snap: dict, scene: CompiledScene, watch: list) -> None:
        self.epoch = self.structure = None  # mutation_epoch(), Raytracer._structure(): read when its trace is done
        self.snap, self.scene, self.watch = snap, scene, watch  # tracing_snapshot(), [(small writeable array, its bytes)]
        self.splits, self.ranges = {}, {}  # N -> split_rays(); (N, power scale) -> range records of a split without remainder
        self.book = None  # RayStorage without buffers: split, ranges and powers of render-only traces
        self.z_last = None  # SectionTable.z_last() of this scene (`RayStorage._tail_proof`)


class Raytracer(Group):

    N_EPS: float = 1e-11
    HURB_FACTOR: float = 2 ** 0.5
    MAX_RAY_STORAGE_RAM: int = 200_000_000_000
    """Upper bound for the ray storage of one trace.  The reference guards host RAM with 6 GB
    (raytracer.py:37); here the storage lives in the 288 GB of HBM3E of one MI355X."""
    ITER_RAYS_STEP: int = None
    """Rays per chunk of `iterative_render` (the reference: 1 M, to bound host RAM, raytracer.py:40).  None: as many
    as ITER_STORAGE_BYTES of ray storage hold, in equal chunks."""
    COMPACT_HITS_FROM: int = 1 << 21
    """`detector_image` with an automatic extent: from this many rays on the hit list between hit search and binning
    holds the valid hits only (`ot_detector_req.fill`)."""
    AUTO_ONE_PASS_FROM: int = 1 << 24
    """... and from this many rays on, where the detector allows it, the sections are read once and the hits sorted on a
    provisional tile grid laid over the extent of a sample: every AUTO_SAMPLE_STRIDE-th wave of 64 rays
    (`_auto_image_one_pass`)."""
    AUTO_SAMPLE_STRIDE: int = 128
    AUTO_MARGINS: tuple = ((0.05, 361), (0.02, 361), (0.5, 1024), (0.3, 1024), (0.15, 1024), (0.3, 2048), (0.15, 2048), (0.05, 2048))
    """(margin around the sample's extent as a fraction of its sides, most tiles) in order of preference."""
    ITER_EXTENT_RAYS: int = 1_000_000
    """`iterative_render` with automatic extents: the extents are those of the hits of the reference's FIRST ITERATION, 1 M
    rays (ITER_RAYS_STEP, raytracer.py:40, 1212-1262); everything after is cropped to them.  A chunk here is tens of
    millions of rays: an evenly spread sample of about this many of the first chunk's rays plays the first iteration's part
    (every k-th wave of 64 rays, `ot_detector_extent_sample`), the rest of the chunk is cropped to that extent like the
    later ones (`_render_detectors` passes the automatic extent as the crop)."""
    ITER_RENDER_ONLY: bool = True
    """`iterative_render`: every chunk but the last is traced render-only -- no section is stored, the last section of
    every ray alive behind the last surface goes to a compact `TailStorage` (56 B per LIVING ray instead of 36-48 B per
    ray and section), which the detector passes read -- wherever that gives the stored path's images: no
    orientation="Function" source, every detector position behind the last tracing surface (every feature level of the
    trace kernel has its render-only form).  False: every chunk through the ray storage."""
    ITER_LAST_RAYS: int = 1 << 20
    """... and the last chunk, whose rays stay in `self.rays` afterwards like those of the reference's last iteration
    (ITER_RAYS_STEP = 1 M there, raytracer.py:40, 1235-1267), then has this many rays."""
    ITER_MERGE_LAST: bool = True
    """... and is binned together with the render-only chunk before it: the last sections of its living rays join that chunk's
    tail (`TailStorage.append_living`), one binning pass less per render.  False: a pass of its own."""
    ITER_GROUP: int = 8
    """Detector positions per pass over a chunk's rays (at most 8: `ot_detector_images`)."""
    ITER_STORAGE_BYTES: int = 16_000_000_000
    """Ray storage of one chunk of `iterative_render` when ITER_RAYS_STEP is None: 16 GB of the 288 GB of HBM are
    19 M rays of a 15-surface scene with polarisation or 93 M rays of a two-surface scene without."""

    class INFOS(IntEnum):
        ABSORB_MISSING = 0
        TIR = 1
        ILL_COND = 2
        OUTLINE_INTERSECTION = 3
        HURB_NEG_DIR = 4

    def __init__(self, outline, n0: RefractionIndex = None, no_pol: bool = False, use_hurb: bool = False,
                 seed: int = None, **kwargs) -> None:
        self.outline = outline
        self.no_pol = no_pol
        self.use_hurb = use_hurb
        self.seed = seed  #: base seed of the device RNG (None: drawn from numpy's global RNG per trace)
        self.rays = RayStorage()
        self._msgs = np.array([])
        self.geometry_error = self._ignore_geometry_error = False   # found by the checks / tracing goes on regardless
        self.fault_pos = np.array([])        # where the geometry checks found surfaces colliding
        self._last_trace_snapshot = None     # tracing_snapshot() of the last trace
        self._scene = None
        self._scene_handle = None
        self._scene_ref = None  # owner of `_scene_handle` (ray_storage.SceneRef), shared with a storage that still needs it
        self._scene_key = None
        self._checked_key = None
        self._rays_known_current = False
        self._source_cache = None  # (key, SourceTable, power scale): device copy of the source records, reused while unchanged
        self._record = None        # _TraceRecord of the last full trace: the shortcut of `trace` for an unchanged scene
        self._msgs_host = None
        self._kernel_ms_log = None  # a list: every trace appends its kernel's duration (HIP events of the library; bench.py)
        super().__init__(None, n0, **kwargs)
        self._new_lock = True

    # bookkeeping of the tracer itself: writing these is not a scene change (base.mutation_epoch)
    _INTERNAL = frozenset(("_msgs", "_last_trace_snapshot", "_scene", "_scene_handle", "_scene_ref", "_scene_key", "_checked_key",
                           "_rays_known_current", "_source_cache", "geometry_error", "fault_pos", "_record",
                           "_msgs_host", "_kernel_ms_log", "_lock", "_new_lock",
                           "seed"))  # (the RNG seed is read at every trace and part of nothing that is compiled or checked)

    def __setattr__(self, key: str, val: Any) -> None:
        if key in self._INTERNAL:
            self.__dict__[key] = val
            return
        if key == "outline":
            check_type(key, val, (list, np.ndarray))
            box = np.asarray_chkfinite(val, dtype=np.float64)
            if box.shape[0] != 6 or np.any(box[0::2] >= box[1::2]):
                raise ValueError("Outline needs to be specified as [x1, x2, y1, y2, z1, z2] "
                                 "with x2 > x1, y2 > y1, z2 > z1.")
            val = box
        elif key in ("no_pol", "use_hurb"):
            check_type(key, val, bool)
        super().__setattr__(key, val)

    @property
    def extent(self):
        """The outline box as a tuple."""
        return tuple(self.outline.tolist())

    @property
    def pos(self):
        """Centre of the outline's front face."""
        x0, x1, y0, y1, z0, _ = self.outline
        return 0.5 * (x0 + x1), 0.5 * (y0 + y1), z0

    def clear(self) -> None:
        super().clear()
        self.rays.__init__()

    # ---- change detection (raytracer.py:129-179) ------------------------------------------------------
    _SNAP_LISTS = (("Lenses", "lenses"), ("Filters", "filters"), ("Apertures", "apertures"), ("RaySources", "ray_sources"))

    def tracing_snapshot(self, writeable: list = None) -> dict:
        """State of everything a trace depends on, as nested lists / tuples of plain values (compared, not hashed).
        `writeable`: a list that collects the arrays met that can still be edited in place (`BaseClass.crepr`)."""
        rays = self.rays
        if writeable is not None and self.outline.flags.writeable:
            writeable.append(self.outline)
        snap = {"Rays": [rays.N, rays.Nt, rays.no_pol],
                "Ambient": [tuple(self.outline), self.n0.crepr(writeable)],
                "TraceSettings": [self.no_pol, self.use_hurb, self.HURB_FACTOR]}
        for key, attr in self._SNAP_LISTS:
            snap[key] = [el.crepr(writeable) for el in getattr(self, attr)]
        return snap

    def property_snapshot(self) -> dict:
        """The tracing snapshot plus the detectors (they matter to images, not to the rays)."""
        snap = self.tracing_snapshot()
        snap["Detectors"] = [det.crepr() for det in self.detectors]
        snap["Markers"] = [m.crepr() for m in self.markers]
        snap["Volumes"] = []  # plot-only elements of the reference: none here, the key for its callers
        return snap

    def compare_property_snapshot(self, h1: dict, h2: dict) -> dict:
        """Which groups differ between two snapshots; "Any" sums up, and new lenses also count as a change of the
        ambient (their n2 takes part in it)."""
        changed = {key: h1[key] != h2[key] for key in h1}
        changed["Ambient"] |= changed["Lenses"]
        changed["Any"] = any(changed.values())
        return changed

    def check_if_rays_are_current(self) -> bool:
        last = self._last_trace_snapshot
        return last is not None and not self.compare_property_snapshot(last, self.tracing_snapshot())["Any"]

    # ---- messages (raytracer.py:181-244) ----------------------------------------------------------------
    _EVENT_TEXT = {
        "TIR": "with total inner reflection at surface {s} ({n}), treating as absorbed.",
        "ABSORB_MISSING": "missing lens surface {s} ({n}), set to absorbed",
        "ILL_COND": "are ill-conditioned for numerical hit finding at surface {s} ({n}). "
                    "Where and whether they intersect might be wrong.",
        "OUTLINE_INTERSECTION": "hitting outline after surface {s} ({n}), set to absorbed.",
        "HURB_NEG_DIR": "have negative z-direction after ray bending at surface {s} ({n}), set to absorbed.",
    }

    def _show_messages(self, N) -> None:
        """One warning per non-zero event counter (raytracer.py:207-244)."""
        if not global_options.show_warnings or not self._msgs.any():
            return
        names = SectionTable(self).names()
        for kind, sec in zip(*np.nonzero(self._msgs)):
            count = self._msgs[kind, sec]
            warning(f"{count} rays ({100*count/N:.3g}% of all rays) "
                    + self._EVENT_TEXT[self.INFOS(kind).name].format(s=sec, n=names[sec]))

    # ---- geometry checks (raytracer.py:510-664) ---------------------------------------------------------
    def _pretrace_check(self, N: int, key: str) -> bool:
        check_type("N", N, int)
        if N < 1:
            raise ValueError(f"Ray number N needs to be at least 1, but is {N}.")
        # the checks sample every surface pair on a 100 x 100 grid (host NumPy); skip them while nothing that
        # they depend on changed (`key`: `_geometry_key`) since they last passed (chunked rendering calls trace() many times)
        if self._checked_key is None or key != self._checked_key or self.geometry_error:
            self._geometry_checks()
            self._checked_key = key if not self.geometry_error else None
        if self.geometry_error and not self._ignore_geometry_error:  # (flag of the reference's test suite)
            warning("ABORTED TRACING")
            return True
        return False

    def _geometry_key(self, snap: dict = None):
        snap = dict(self.tracing_snapshot() if snap is None else snap)
        snap.pop("Rays", None)
        return repr(snap)

    def _geometry_checks(self) -> None:
        """Scene validation (checks.py): sets `geometry_error` / `fault_pos` and warns about the first finding."""
        finding = _checks.find_geometry_error(self, tracing_elements(self))
        self.geometry_error = finding is not None
        if finding is not None:
            text, where = finding
            warning(text)
            if where is not None:
                self.fault_pos = where

    @staticmethod
    def check_collision(front, back, res: int = 100):
        """Is `front` anywhere behind `back` where both are defined?  -> (collision, x, y, z) of the offending sample
        positions on a res x res grid (raytracer.py:580-664); see checks.collision_points."""
        return _checks.collision_points(front, back, res)

    # ---- scene upload --------------------------------------------------------------------------------------
    def _compile(self, key: str) -> CompiledScene:
        """Flatten the scene and upload its tables; reused while `_geometry_key` is unchanged."""
        lib = _capi.load_library()
        if self._scene is not None and self._scene_handle is not None and key == self._scene_key:
            return self._scene
        self._release_scene()
        self._scene = CompiledScene(self)
        self._check_media()
        handle = C.c_void_p()
        _capi.check(lib.ot_scene_create(C.byref(self._scene.desc), C.byref(handle)))
        self._scene_ref = SceneRef(handle)
        self._scene_handle = handle
        # Nothing reads the index plane or the polarisation planes on the way from a trace to an image, a spectrum or a
        # focus: the kernels leave them unwritten (20 of 48 B per section) and the storage fills them when `n_list` /
        # `pol_list` is asked for (RayStorage._ensure_index, _ensure_pol).  Position and weight before the last two sections
        # are read by inspection and analysis, not by a detector behind the stack: left out as well (28 B per section) and
        # written by a repeat of the trace when they are read (RayStorage._ensure_sections, detector.rays_for)
        _capi.check(lib.ot_scene_set_deferred_planes(handle, _capi.OT_DEFER_INDEX | _capi.OT_DEFER_POL
                                                     | _capi.OT_DEFER_SECTIONS))
        self._scene_key = key
        return self._scene

    def _check_media(self) -> None:
        """RefractionIndex.__call__ raises for n < 1 (refraction_index.py:165-167) and for wavelengths outside a
        tabulated range (:152-156); the tracing kernel cannot raise per ray, so every medium is evaluated once per
        scene over the wavelengths the sources can emit (device evaluation through RefractionIndex.__call__)."""
        from .scene import discrete_lines
        lines = discrete_lines(self.ray_sources)
        wl = lines.astype(np.float64) if lines is not None else np.linspace(*global_options.wavelength_range, 201)
        seen = set()
        for n in [self.n0] + [L.n for L in self.lenses] + [L.n2 for L in self.lenses if L.n2 is not None]:
            if id(n) not in seen:
                seen.add(id(n))
                n(wl)

    def _release_scene(self) -> None:
        # (destroyed with its last holder: a storage whose index plane is not filled yet keeps the scene that traced it)
        self._scene_ref = None
        self._scene_handle = None
        self._scene_key = None

    def __del__(self):
        try:
            self._release_scene()
        except Exception:
            pass

    # ---- tracing (raytracer.py:262-415) -----------------------------------------------------------------
    def _structure(self) -> tuple:
        """Identity of everything in the tracing lists (list edits do not pass through __setattr__)."""
        return (tuple(map(id, self.lenses)), tuple(map(id, self.apertures)), tuple(map(id, self.filters)),
                tuple(map(id, self.ray_sources)))

    def _scene_unchanged(self) -> bool:
        """Is everything the last full trace established (checks passed, compiled scene, source table) still valid?  One
        integer comparison, the identities of the list members and the bytes of the few small writeable arrays."""
        rec = self._record
        return (rec is not None and rec.epoch == _base.mutation_epoch() and rec.structure == self._structure()
                and not self.geometry_error and all(a.tobytes() == b for a, b in rec.watch))

    def trace(self, N: int, _initial_rays: tuple = None, _hurb_normals: np.ndarray = None, _N_list=None,
              _chunk: int = 0, _power_scale: float = 1.0, _tail: TailStorage = None, _tail_room: int = 0) -> None:
        """Trace N rays through the current geometry.

        Geometry errors are reported as warnings and set `geometry_error` instead of raising, like the
        reference.  `_initial_rays` = (p, s, pols, w, wl), `_N_list` (rays per source) and `_hurb_normals`
        (2*n_hurb, N) inject recorded inputs for parity tests; normally rays are generated inside the
        tracing kernel and the remainder of the per-source split is drawn at random like the reference does.
        `_power_scale`: share of the source powers these rays carry (a rank's shard, distributed.py).
        `_tail`: render-only trace (`iterative_render`, every chunk but the last): no section is stored and `self.rays`
        stays as it is; the last section of every ray still alive behind the last surface goes to that `TailStorage`
        (`ot_generate_and_trace_tail`).  Counters and warnings as for a stored trace.  `_tail_room`: slots for that many
        further rays (`TailStorage.append_living`).

        The reference re-reads the whole object graph on every call (raytracer.py:246-278).  Here everything
        derived from it -- geometry checks, the compiled scene, the source table, the snapshot -- is kept while
        nothing changed: every tracked object reports assignments to a global counter (base.mutation_epoch), so
        an unchanged scene is recognised by one integer comparison, the identities of the list members and the bytes of
        the few small arrays that are still writeable (large ones are read-only or switch the shortcut off).  All but the
        source table (`_source_cache`, keyed by content) is one `_TraceRecord`, replaced as a whole on a change.
        """
        if _tail is not None and _initial_rays is not None:
            raise ValueError("a render-only trace generates its rays on the device")
        shortcut = self._scene_unchanged()
        if shortcut:
            check_type("N", N, int)
            if N < 1:
                raise ValueError(f"Ray number N needs to be at least 1, but is {N}.")
            rec, publish = self._record, False
        else:
            self._record = None
            writeable = []
            snap = self.tracing_snapshot(writeable)  # taken once: geometry key and the post-trace record
            key = self._geometry_key(snap)
            if self._pretrace_check(N, key):
                return
            # large arrays that can still change in place: no shortcut next time; small ones: their bytes are compared
            # before every shortcut (assignments move the counter, an edit in place like `RS.s[0] = 0.1` does not)
            publish = all(a.size < _base.SMALL_ARRAY for a in writeable)
            rec = _TraceRecord(snap, self._compile(key), [(a, a.tobytes()) for a in writeable] if publish else [])
            rec.z_last = SectionTable(self).z_last()
        lib = _capi.load_library()
        dev = require_device()

        nt = rec.scene.nt
        if _tail is None and self.rays.storage_size(N, nt, self.no_pol) > self.MAX_RAY_STORAGE_RAM:
            raise RuntimeError(f"More than {self.MAX_RAY_STORAGE_RAM*1e-9:.1f} GB RAM requested. Either decrease"
                               " the number of rays, surfaces or do an iterative render. If your system can handle"
                               " more RAM usage, increase the Raytracer.MAX_RAY_STORAGE_RAM parameter.")

        split = rec.splits.get(N)
        if split is None:
            split = rec.splits[N] = RayStorage.split_rays(self.ray_sources, N)
        # a split without a remainder to draw (and none given) has the same range records every time
        ranges_key = (N, _power_scale) if not split[1] and _N_list is None else None
        rng = None  # draws the remainder of the split: a seeded tracer repeats it with the seed
        if self.seed is not None and split[1]:
            rng = np.random.RandomState((int(self.seed) + 1000003 * int(_chunk)) % 2 ** 32)
        rays_obj = self.rays
        if _tail is not None:  # the split, the ranges and the powers live in a storage object without buffers
            if rec.book is None:
                rec.book = RayStorage()
            rays_obj = rec.book
        rays_obj.init(self.ray_sources, N, nt, self.no_pol, _N_list=_N_list, _rng=rng, _power_scale=_power_scale,
                      _split=split, _ranges=rec.ranges.get(ranges_key), _alloc=_tail is None)
        # (the trace writes the buffers: no fill of what the trace before it left out)
        rays = rays_obj._rays_struct(tail_only=True) if _tail is None else None
        # a seeded tracer repeats itself call for call; the chunks of one iterative render must differ
        seed = int(np.random.randint(0, 2 ** 31 - 1)) if self.seed is None else int(self.seed) + 1000003 * int(_chunk)

        n_msgs = len(self.INFOS) * nt + 1
        if self._msgs_host is None or self._msgs_host.shape[0] != n_msgs:
            self._msgs_host = np.zeros(n_msgs, dtype=np.int64)
        msgs_h = self._msgs_host
        if _initial_rays is None:
            if rays_obj._has_function_orientation:  # per-trace orientation arrays: nothing to reuse
                tab = rays_obj._source_table(seed)
            else:
                cache = self._source_cache
                if not shortcut or cache is None or cache[2] != _power_scale:
                    skey = (repr(rec.snap["RaySources"]), tuple(rays_obj._powers))
                    if cache is None or cache[0] != skey:
                        self._source_cache = cache = (skey, rays_obj._source_table(), _power_scale)
                tab = cache[1]
            rng_c = rays_obj._source_ranges()
            if ranges_key is not None:
                rec.ranges[ranges_key] = rng_c
            # one synchronous call: launch, wait, counters in host memory (no device-to-host copy)
            if _tail is not None:
                _tail.ensure(int(lib.ot_tail_capacity(N + _tail_room)))
                mb_t, mb = mailbox()
                _capi.check(lib.ot_generate_and_trace_tail(self._scene_handle, tab.handle, rng_c, len(rng_c), seed, N,
                                                           C.byref(_tail._rays_struct()), ptr(_tail._dev["fill"]),
                                                           C.c_void_p(mb_t.data_ptr()), msgs_h.ctypes.data, stream_ptr()))
                _tail.N, _tail.alive, _tail.traced = int(mb[0]), int(mb[1]), N
            else:
                rays_obj._index_pending(self._scene_ref, N)
                rays_obj._pol_pending(self._scene_ref, tab, rng_c, seed, N)
                rays_obj._sections_pending(self._scene_ref, tab, rng_c, seed, N)
                _capi.check(lib.ot_generate_and_trace_host(self._scene_handle, tab.handle, rng_c, len(rng_c), seed,
                                                           C.byref(rays), msgs_h.ctypes.data, stream_ptr()))
        else:
            rays_obj.set_initial_rays(*_initial_rays)
            hn = None
            if _hurb_normals is not None:
                rows = np.ascontiguousarray(_hurb_normals, dtype=np.float64).reshape(-1, N)
                if rays_obj._Np > N:  # one row per (aperture, component), laid out with the storage's plane stride
                    rows = np.pad(rows, ((0, 0), (0, rays_obj._Np - N)))
                hn = torch.from_numpy(np.ascontiguousarray(rows).reshape(-1)).to(dev)
            msgs = torch.zeros(n_msgs, dtype=torch.int64, device=dev)
            rays_obj._index_pending(self._scene_ref, rays_obj._Np)  # (ot_trace walks the whole stride)
            rays_obj._pol_pending(None, None, None, 0, 0)  # (and stores the polarisation planes itself)
            rays_obj._sections_pending(None, None, None, 0, 0)  # (and every section)
            _capi.check(lib.ot_trace(self._scene_handle, C.byref(rays), ptr(hn), seed, ptr(msgs), stream_ptr()))
            msgs_h = msgs.cpu().numpy()  # (synchronises the stream)

        if _tail is None:
            rays_obj.lock()
        if self._kernel_ms_log is not None:  # (the caller switched the scene's event pair on: ot_scene_set_timing)
            ms = C.c_double()
            _capi.check(lib.ot_scene_last_trace_ms(self._scene_handle, C.byref(ms)))
            self._kernel_ms_log.append(ms.value)
        if msgs_h[-1]:
            raise TimeoutError("Timeout after 200 iterations in hit finding. Try retracing.")
        self._msgs = msgs_h[:-1].reshape(len(self.INFOS), nt).astype(int)
        if self._msgs[self.INFOS.HURB_NEG_DIR, 0]:  # generation reports directions with s_z <= 0 in this cell
            self._msgs[self.INFOS.HURB_NEG_DIR, 0] = 0
            raise RuntimeError("All ray divergences s need to be in positive z-divergence")
        self._show_messages(N)
        if _tail is None and _initial_rays is None:
            rays_obj._tail_proof(rec.z_last + self.N_EPS, bool(self._msgs[self.INFOS.OUTLINE_INTERSECTION].any()))
        if _tail is None:  # (a render-only trace leaves `self.rays` and what is known about them alone)
            self._last_trace_snapshot = {**rec.snap, "Rays": [rays_obj.N, rays_obj.Nt, rays_obj.no_pol]}
        if publish and _initial_rays is None and not rays_obj._has_function_orientation:
            # read the counter last: objects this call created itself (the end aperture of the element list) count too
            rec.epoch, rec.structure = _base.mutation_epoch(), self._structure()
            self._record = rec

    # ---- detector (raytracer.py:881-1098) ----------------------------------------------------------------
    # ---- shared argument checks of the post-processing entry points ------------------------------------------
    def _need_rays(self) -> None:
        if not self.rays.N:
            raise RuntimeError("No rays traced.")

    def _need_current(self, hint: str = "") -> None:
        """The stored rays must belong to the present geometry (raytracer.py:903-913)."""
        if self._rays_known_current or self.check_if_rays_are_current():
            return
        raise RuntimeError(f"Tracing geometry/properties changed{hint}. Please retrace first.")

    def _ray_range(self, source_index) -> tuple:
        """[first, end) of the rays of one source, or of all rays for None."""
        if source_index is None:
            return 0, int(self.rays.N)
        if not 0 <= source_index < len(self.ray_sources):
            raise IndexError("Invalid source_index.")
        return int(self.rays.B_list[source_index]), int(self.rays.B_list[source_index + 1])

    def _stored_range(self, source_index) -> tuple:
        """`_ray_range` for what reads the stored rays of a source: there are sources, rays, and they are current."""
        if not self.ray_sources:
            raise RuntimeError("Ray Sources Missing.")
        self._need_rays()
        Ns, Ne = self._ray_range(source_index)
        self._need_current()
        return Ns, Ne

    @staticmethod
    def _rays_tag(source_index) -> str:
        return "all rays" if source_index is None else f"{RaySource.abbr}{source_index}"

    def _warn_ill(self, ill_count: int, detector_index: int) -> None:
        if ill_count:
            warning(f"{ill_count} rays ({100*ill_count/self.rays.N:.3g}% of all rays) were ill-conditioned for "
                    f"numerical hit finding at detector {detector_index}. "
                    "Where and whether they intersect might be wrong.")

    def _detector_requests(self, specs: list, rays=None, no_rays: bool = False) -> list:
        """Checks of `_hit_detector` (raytracer.py:897-920) and, per spec, the `detector.DetectorRequest` the device calls
        take.  specs: dicts with detector_index, source_index, extent, projection_method and optionally pos (the detector is
        moved there first, as `iterative_render` does position by position, raytracer.py:1244), auto_extent (`_auto_extents`),
        want_z, compact, weights_only; or requests made already, which come back as they are.
        `rays`: a `TailStorage` to take the rays from instead of `self.rays` (all its slots, no per-source ranges);
        `no_rays`: no storage yet (`_plan_renders` before the first trace): nothing about rays is checked or recorded."""
        if specs and isinstance(specs[0], _detector.DetectorRequest):
            return specs
        if not self.detectors:
            raise RuntimeError("Detector Missing")
        if rays is None and not no_rays:
            self._need_rays()
        ranges = []
        for sp in specs:  # all indices first: nothing is moved or launched for a bad request
            if no_rays:  # (a plan made before the rays exist: it ranges over the whole of whatever storage it is launched on)
                ranges.append((0, None))
            else:
                Ns, Ne = self._ray_range(sp.get("source_index")) if rays is None else (0, int(rays.N))
                ranges.append((Ns, Ne - Ns))
            if not 0 <= sp.get("detector_index", 0) < len(self.detectors):
                raise IndexError("Invalid detector_index.")
        if rays is None and not no_rays:
            self._need_current()

        out = []
        for sp, (first, count) in zip(specs, ranges):
            k = sp.get("detector_index", 0)
            det = self.detectors[k]
            if sp.get("pos") is not None:
                # (a detector and its own surface are untracked: the next trace of an iterative render keeps its shortcut)
                det.move_to(sp["pos"])
            dsurf = det.surface

            method = sp.get("projection_method", "Equidistant")
            projection = None
            if isinstance(dsurf, SphericalSurface) and method is not None:
                if method not in SphericalSurface.sphere_projection_methods:
                    raise ValueError(f"Invalid projection_method {method}, "
                                     f"must be one of {SphericalSurface.sphere_projection_methods}.")
                projection = method

            extent = sp.get("extent")
            if not (extent is None or isinstance(extent, (list, np.ndarray))):
                raise ValueError(f"Invalid extent '{extent}'.")
            # An automatic extent crops like a user extent.  One of ALL the hits loses none by that; one taken from a sample of
            # the rays or agreed with other ranks then treats the first chunk of an iterative render like the later ones, which
            # are cropped to this very extent (`_extent0`, raytracer.py:1262) -- without the crop the margin `_fix_extent` adds
            # around it (and the band a line-like image is widened to) would collect hits of the first chunk only
            crop = sp.get("auto_extent")
            if extent is not None:
                crop = np.asarray_chkfinite(np.array(extent, dtype=np.float64), dtype=np.float64)
            elif crop is not None:
                crop = np.asarray(crop, dtype=np.float64)
            title = f": {det.desc}" if det.desc else ""
            out.append(_detector.DetectorRequest(
                first, count, dsurf._desc(), projection, crop, k, sp.get("source_index"),
                f"{Detector.abbr}{k}{title} at z = {det.pos[2]:.5g} mm", bool(sp.get("want_z", False)),
                bool(sp.get("compact", False)), bool(sp.get("weights_only", False))))
        return out

    def _hit_detectors(self, specs: list) -> list:
        """Device hit search for several (detector, position) pairs in one pass over the ray sections.

        specs: as for `_detector_requests`.  -> per spec a `detector.DetectorHits`: device tensors of the selected ray range
        (xy: the x and y planes, the z plane as well with want_z; dense: rays without a valid hit carry weight 0), the extent
        actually used, the projection name, the ill-conditioned count and the detector's description at that position."""
        reqs = self._detector_requests(specs)
        out = [None] * len(reqs)
        for part, rqs in _detector.batches(reqs):
            Ns, count = rqs[0].first, rqs[0].count
            # rays outside a user extent are dropped (raytracer.py:1036-1040): the hit kernel gives them weight 0
            res = _detector.detector_hits_multi(self.rays, Ns, count, rqs)
            for n, rq, hl in zip(part, rqs, res):
                extent_out = rq.crop
                if extent_out is None:
                    extent_out = hl.extent if np.all(np.isfinite(hl.extent)) else rq.centre
                wl = self.rays._dev["wl"][Ns:Ns + count] if hl.wl is None else hl.wl
                out[n] = _detector.DetectorHits(hl.ph, hl.hw, wl, extent_out, rq.projection, hl.ill_count, rq.label, hl.fill)
        return out

    def _render_detectors(self, specs: list, limits: list, into: list = None, rays=None, weight_scale: float = 1.0,
                          **kwargs) -> list:
        """Detector images whose extents are known beforehand (every spec carries a user extent, or the automatic
        one of `_auto_extents` as "auto_extent"): hit search and
        binning in ONE pass over the ray sections (`ot_detector_images`), up to 8 images per pass; the hit positions
        are never written to memory.  into: per spec a (Ny, Nx, 4) device histogram to add to, or None.
        `rays`: a `TailStorage` (render-only chunk) instead of `self.rays`; `weight_scale`: every hit's weight times this (in
        f64) before it is added -- the chunks of an iterative render bin straight into one image with rays_step / N each.
        -> RenderImages (raytracer.py:1053-1098 for each spec)."""
        plan = self._plan_renders(specs, limits, into=into, rays=rays)
        self._launch_renders(plan, rays=rays, weight_scale=weight_scale)
        images = plan["images"]
        if not kwargs.get("_dont_filter", False):
            for img in images:
                if img._limit is not None:
                    img._apply_rayleigh_filter()
        return images

    def _plan_renders(self, specs: list, limits: list, into: list = None, rays=None, whole_storage: bool = False) -> dict:
        """Everything `_render_detectors` does on the host before the launch: checks, the detectors moved to their positions,
        one `RenderImage` per spec on its fixed grid, the histograms (one zero-filled allocation for all images that have
        none yet) and with them the image grid of every request.  `whole_storage`: the requests range over
        whatever storage `_launch_renders` is given (no source_index) -- `iterative_render` plans once, before its first trace
        where the extents are known, and launches the plan chunk after chunk.  -> dict(images, requests)"""
        reqs = self._detector_requests(specs, rays, no_rays=whole_storage)
        images = []
        dev = require_device()
        for n, (rq, limit) in enumerate(zip(reqs, limits)):  # (the image extent is the crop: the user or the automatic extent)
            img, rq.Nx, rq.Ny = RenderImage.on_grid(rq.crop, rq.projection, rq.image_label, limit)
            rq.extent = img.extent
            tgt = None if into is None else into[n]
            if tgt is not None:
                if tuple(tgt.shape) != (rq.Ny, rq.Nx, 4):
                    raise ValueError("histogram to accumulate into has the wrong shape")
                rq.hist = tgt.view(-1)
            images.append(img)
        # the new histograms: ONE zero-filled allocation, sliced (six images of an iterative render: one fill kernel)
        sizes = [rq.Ny * rq.Nx * 4 if rq.hist is None else 0 for rq in reqs]
        pool = alloc_retry(lambda: torch.zeros(sum(sizes), dtype=torch.float64, device=dev)) if sum(sizes) else None
        off = 0
        for img, rq, size in zip(images, reqs, sizes):
            if rq.hist is None:
                rq.hist = pool[off:off + size]
                off += size
            img._attach(rq.hist, rq.Nx, rq.Ny)
        return dict(images=images, requests=reqs)

    def _launch_renders(self, plan: dict, rays=None, weight_scale: float = 1.0) -> None:
        """`ot_detector_images` for a plan of `_plan_renders`, on `rays` (a `TailStorage`) or `self.rays`."""
        src_rays = self.rays if rays is None else rays
        for _, rqs in _detector.batches(plan["requests"]):
            first, count = rqs[0].first, rqs[0].count if rqs[0].count is not None else int(src_rays.N)
            if count <= 0:  # (a render-only chunk none of whose rays survived)
                continue
            for rq in rqs:
                rq.weight_scale = weight_scale
            for rq, ill_count in zip(rqs, _detector.detector_images(src_rays, first, count, rqs)):
                self._warn_ill(ill_count, rq.detector_index)

    def _auto_extents(self, specs: list, agree=None, sample_rays: int = None, rays=None) -> list:
        """Automatic extents (raytracer.py:1042-1049) of the specs without a user extent, from an extent-only pass over
        the ray sections (no hit list: `detector.detector_extents`, up to 8 detectors per pass).  `agree`: callable
        mapping the (n, 4) array of raw extents (+-inf where no ray hits) to the one every rank uses
        (distributed.py); an extent no ray reaches collapses to the detector centre.  `sample_rays`: the extents of
        about that many evenly spread rays instead of all (ITER_EXTENT_RAYS).  -> specs with "auto_extent" set."""
        todo = [n for n, sp in enumerate(specs) if sp.get("extent") is None]
        if not todo:
            return specs
        reqs = self._detector_requests(specs, rays)
        src_rays = self.rays if rays is None else rays
        # (a render-only chunk holds the living rays of `traced` generated ones: the sample keeps the stride that
        # `sample_rays` of the GENERATED rays would have)
        traced = None if rays is None else int(rays.traced)
        raw = np.empty((len(todo), 4), dtype=np.float64)
        raw[:] = [np.inf, -np.inf, np.inf, -np.inf]
        rest = []  # rows of `raw` that take the pass over all rays
        for m, n in enumerate(todo):
            rq = reqs[n]
            if rq.count < 1:
                continue
            n_gen = rq.count if traced is None else traced
            if sample_rays and n_gen >= 2 * sample_rays and _capi.fused_ok(rq.surf, rq.proj_id):
                raw[m] = _detector.detector_extent_sample(src_rays, rq.first, rq.count, rq.surf, rq.proj_id,
                                                          n_gen // sample_rays)
                continue
            rest.append(m)
        for part, rqs in _detector.batches([reqs[todo[m]] for m in rest]):
            res = _detector.detector_extents(src_rays, rqs[0].first, rqs[0].count, rqs)
            for i, (ext4, _) in zip(part, res):
                raw[rest[i]] = ext4
        if agree is not None:
            raw = np.asarray(agree(raw), dtype=np.float64).reshape(len(todo), 4)
        out = [dict(sp) for sp in specs]
        for m, n in enumerate(todo):
            out[n]["auto_extent"] = raw[m].copy() if np.all(np.isfinite(raw[m])) else reqs[n].centre
        return out

    def _hit_detector(self, info: str, detector_index: int = 0, source_index: int = None, extent=None,
                      projection_method: str = "Equidistant"):
        """One detector: (ph, hw, wl, extent_out, projection, ill_count), see `_hit_detectors`."""
        return self._hit_detectors([dict(detector_index=detector_index, source_index=source_index, extent=extent,
                                         projection_method=projection_method, want_z=True)])[0][:6]

    def _image_from_hits(self, hits, rq, limit, **kwargs) -> RenderImage:
        """Bin one hit list of `_hit_detectors` (`hits`, for the request `rq`) into a RenderImage."""
        image = RenderImage(extent=hits.extent, projection=hits.projection, long_desc=rq.image_label)
        image.render(hits.xy, hits.w, hits.wl, limit=limit, _fill=hits.fill, **kwargs)
        self._warn_ill(hits.ill_count, rq.detector_index)
        return image

    def detector_image(self, detector_index: int = 0, source_index: int = None, extent=None,
                       limit: float = None, projection_method: str = "Equidistant", **kwargs) -> RenderImage:
        """Render the image on a detector for the traced rays (raytracer.py:1053-1098)."""
        if limit is not None and extent is not None and "_dont_filter" not in kwargs:
            warning("Using the limit parameter in combination with a user defined extent"
                    " will produce an incorrect detector image, as the rays outside the extent"
                    " are not included in the convolution calculation.")
        # extent known: one pass, no hit positions in memory -- except for long bundles on a spherical detector whose
        # projection has a transcendental (`ot_detector_images` would send that request through the chain with a dense hit
        # list; the chain over a compact list of the hits inside the extent is faster, C3 1.55 -> 1.4 ms)
        projected = (0 <= detector_index < len(self.detectors) and self.rays.N >= self.COMPACT_HITS_FROM
                     and isinstance(self.detectors[detector_index].surface, SphericalSurface)
                     and projection_method in ("Equidistant", "Equal-Area", "Stereographic"))
        # (long bundles: a hit list holds the valid hits only, gathered piece-wise -- a third of the bytes for C4)
        rq = self._detector_requests([dict(
            detector_index=detector_index, source_index=source_index, extent=extent, projection_method=projection_method,
            compact=(extent is None or projected) and self.rays.N >= self.COMPACT_HITS_FROM)])[0]
        unfused = kwargs.pop("_unfused", False)
        if extent is not None and not unfused and not projected:
            return self._render_detectors([rq], [limit], **kwargs)[0]
        # Automatic extent: hit list first, then the binning.  (Measured against an extent-only pass followed by the
        # fused kernels, `_auto_extents` + `_render_detectors`, profiles/r3/detector_full_size.txt: C4 5.7 against 5.8 ms,
        # C5 3.7 / 3.6, and slower where the fused entry point falls back to this chain anyway -- spherical detectors, C3
        # 3.0 against 1.9 ms -- or the image is point-like, C2 1.3 against 0.9 ms: the sections are read twice either
        # way.  The extent-only pass serves where hit lists would have to be kept or exchanged: the first chunk of
        # `iterative_render` and the sharded forms in distributed.py.)
        # Long bundles, detectors with a closed-form hit: the sections are read once, the hits are sorted on a provisional
        # tile grid while their extent is found (`_auto_image_one_pass`; None: not applicable, the chain below runs)
        if not unfused and self.rays.N >= self.AUTO_ONE_PASS_FROM:
            img = self._auto_image_one_pass(rq, limit, **kwargs)
            if img is not None:
                return img
        return self._image_from_hits(self._hit_detectors([rq])[0], rq, limit, **kwargs)

    @staticmethod
    def _auto_grid(e0, limit, projection, margins):
        """Provisional tile grid for an image whose final extent E contains the sample extent e0 (`_auto_image_one_pass`).
        Tiles are 60 x 60 pixels of e0's OWN image (after `RenderImage._fix_extent` with `limit`); E's image has pixels at
        least that large, because its sides are at least e0's and its pixel counts at most those assumed here (the long
        side's count is taken for a side ratio 20 % beyond e0's, `RenderImage._pixel_counts` snaps at 2 and 4).
        -> ((X0, Y0, tile_w, tile_h, tiles_x, tiles_y), tile_w, tile_h), or None for point- / line-like and very
        elongated sample extents and where no margin of `margins` ((fraction of e0's sides, most tiles), ...) fits."""
        sx0, sy0 = e0[1] - e0[0], e0[3] - e0[2]
        MR, side = RenderImage.MAX_IMAGE_RATIO, RenderImage.MAX_IMAGE_SIDE
        if min(sx0, sy0) <= 0 or max(sx0, sy0) / min(sx0, sy0) > MR / 1.2:
            return None
        sx, sy = RenderImage.on_grid(np.array(e0, dtype=np.float64), projection, limit=limit)[0].s
        n_long = side * min(MR, 1 + 2 * int(1.2 * max(sx, sy) / min(sx, sy) / 2))
        Nx0, Ny0 = (n_long, side) if sx > sy else (side, n_long)
        tw, th = 60 * sx / Nx0, 60 * sy / Ny0
        for margin, most in margins:
            tx = int(np.ceil((1 + 2 * margin) * sx0 / tw)) + 1
            ty = int(np.ceil((1 + 2 * margin) * sy0 / th)) + 1
            if tx * ty <= most:  # (up to 1024 tiles: the tile kernel's faster form, two rays per thread)
                return (e0[0] - margin * sx0, e0[2] - margin * sy0, tw, th, tx, ty), tw, th
        return None

    def _auto_image_one_pass(self, rq, limit, **kwargs):
        """Image with an automatic extent (raytracer.py:1042-1049, 1053-1098) of the request `rq` in one pass over the ray
        sections (`detector.AutoImage`, csrc/ot_detector_fused.hpp last section).  The extent E0 of the hits of a sample of the
        rays lies inside the final extent E, so the pixels of E's image are at least as large as those of E0's own
        image; tiles of 60 such pixels therefore fit 64 x 64 windows of the final grid.  -> RenderImage, or None where
        this form does not apply (detector with a numeric hit search or a sphere projection, no hit in the sample,
        point- / line-like or very elongated sample extent, too many hits outside the provisional grid): the caller
        takes the hit-list chain."""
        Ns, count, sd, proj = rq.first, rq.count, rq.surf, rq.proj_id
        if count < 1 or not _capi.fused_ok(sd, proj):
            return None
        e0 = _detector.detector_extent_sample(self.rays, Ns, count, sd, proj, self.AUTO_SAMPLE_STRIDE)
        if not np.all(np.isfinite(e0)):
            return None
        plan = self._auto_grid(e0, limit, rq.projection, self.AUTO_MARGINS)
        if plan is None:
            return None
        grid, tw, th = plan

        try:
            auto = _detector.AutoImage(self.rays, Ns, count, sd, proj, grid)
        except _capi.BackendError as err:
            if getattr(err, "status", 0) == _capi.ERR_UNSUPPORTED:  # e.g. no room for the records: the chain needs less
                return None
            raise
        if auto.escaped > auto.escape_capacity or not np.all(np.isfinite(auto.extent)):
            auto.cancel()
            return None
        img, Nx, Ny = RenderImage.on_grid(auto.extent.copy(), rq.projection, rq.image_label, limit)
        if tw * Nx / img.s[0] > 61 or th * Ny / img.s[1] > 61:  # a tile would not fit its window (ratio snapped further)
            auto.cancel()
            return None
        hist = alloc_retry(lambda: torch.zeros(Ny * Nx * 4, dtype=torch.float64, device=require_device()))
        auto.finish(img.extent, Nx, Ny, hist)
        img._attach(hist, Nx, Ny)
        if limit is not None and not kwargs.get("_dont_filter", False):
            img._apply_rayleigh_filter()
        return img

    def detector_spectrum(self, detector_index: int = 0, source_index: int = None, extent=None,
                          **kwargs) -> LightSpectrum:
        """Spectrum of the light hitting a detector (raytracer.py:1100-1132); hit search and histogram on the GPU."""
        # long bundles: a compact list of the valid hits' weights and wavelengths (no positions: 8 B per valid hit written
        # instead of 28 B per ray, and the two histogram passes read those alone)
        compact = self.rays.N >= self.COMPACT_HITS_FROM
        hits = self._hit_detectors([dict(detector_index=detector_index, source_index=source_index, extent=extent,
                                         projection_method="Equidistant", want_z=not compact, compact=compact,
                                         weights_only=compact)])[0]
        prefix = "Spectrum at " if source_index is None else f"Spectrum of RS{source_index} at "
        spec = LightSpectrum.render(hits.wl, hits.w, _fill=hits.fill, long_desc=prefix + hits.label, **kwargs)
        self._warn_ill(hits.ill_count, detector_index)
        return spec

    def spot_analysis(self, detector_index: int = 0, source_index: int = None, extent=None,
                      projection_method: str = "Equidistant", n_radii: int = 256, frequencies=None) -> SpotAnalysis:
        """Centroid, RMS size, encircled energy and geometric MTF of the hits on a detector (no counterpart in optrace):
        hit search as for `detector_image`, then reductions over the hit list on the GPU (spot.py).  n_radii: radial bins of
        the encircled energy; frequencies: where the transfer function is wanted, in cycles per length unit (default: 65
        values up to 1 / RMS radius)."""
        freq = _spot.check_arguments(n_radii, frequencies)
        require_device()  # (said before anything about the rays: without a device there are none)
        # (long bundles: the list of the valid hits only, as for the detector image)
        rq = self._detector_requests([dict(detector_index=detector_index, source_index=source_index, extent=extent,
                                           projection_method=projection_method,
                                           compact=self.rays.N >= self.COMPACT_HITS_FROM)])[0]
        hits = self._hit_detectors([rq])[0]
        sa = _spot.analyse(hits.xy, hits.w, rq.count, hits.fill, hits.extent, n_radii, freq,
                           long_desc="Spot at " + rq.image_label)
        self._warn_ill(hits.ill_count, detector_index)
        return sa

    def wavefront_analysis(self, source_index: int = 0, section: int = None, focus=None, radius: float = None,
                           n_zernike: int = 15, n_grid: int = 64, pupil_radius: float = None) -> WavefrontAnalysis:
        """Optical path difference of one source's rays (None: all rays) against a reference sphere, its RMS and
        peak-to-valley, Zernike coefficients and a pupil map (no counterpart in optrace): reductions over the stored sections
        on the GPU (wavefront.py).  section: the ray section whose lines meet the sphere, default the space behind the last
        surface; focus, radius: centre and signed radius of the sphere, default the point closest to all ray lines and its
        distance from the mean start of the section; n_zernike: Noll polynomials fitted; n_grid: cells per side of the map;
        pupil_radius: radius of the unit disc in units of |radius|, default the largest distance from the pupil centre."""
        table = SectionTable(self)
        focus, radius, pupil_radius = _wavefront.check_arguments(table.nt, section, focus, radius, n_zernike, n_grid, pupil_radius)
        Ns, Ne, k, origin, label = self._section_bundle(table, source_index, section, "the wavefront figures hold")
        return _wavefront.analyse(self.rays, Ns, Ne - Ns, k, origin, focus, radius, n_zernike, n_grid, pupil_radius,
                                  long_desc=f"Wavefront of {label} behind section {k}")

    def huygens_psf(self, source_index: int = 0, section: int = None, focus=None, radius: float = None, n_px: int = 64,
                    size: float = None, dz: float = 0.0) -> HuygensPSF:
        """Diffraction image of a point from one source's rays (None: all rays), no counterpart in optrace: every ray sends a
        spherical wavelet from its place on the reference sphere of `wavefront_analysis`, with the phase of its optical path, and
        the wavelets are added coherently on the GPU (psf.py).  section, focus, radius: as for `wavefront_analysis`; n_px: image
        points per side; size: side length of the square of image points about the focus in the plane z = focus z + dz, default
        ten mean wavelengths over the pupil radius (about eight Airy diameters in air).  For a source of several wavelengths or
        several planes: `huygens_stack`."""
        table = SectionTable(self)
        focus, radius, size, dz = _psf.check_arguments(table.nt, section, focus, radius, n_px, size, dz)
        Ns, Ne, k, origin, label = self._section_bundle(table, source_index, section, "the point spread function holds")
        return _psf.analyse(self.rays, Ns, Ne - Ns, k, origin, focus, radius, n_px, size, dz,
                            long_desc=f"Huygens PSF of {label} behind section {k}")

    def huygens_stack(self, source_index: int = 0, section: int = None, focus=None, radius: float = None, n_px: int = 64,
                      size: float = None, dz=0.0, bands="lines") -> HuygensStack:
        """`huygens_psf` for a source of several wavelengths, on one plane or a through-focus series: rays of one band of
        wavelengths add coherently, the bands add in intensity, each with the weight of its power and (n / lambda)^2 (psf.py).
        dz: a number or up to 64 of them, plane z lies at focus z + dz[z].  bands: "lines", every distinct wavelength a band of its
        own (32 at the most); an int K, that many equal bands over the used rays' wavelengths; or K + 1 ascending edges in nm,
        the last band closed above.  The other arguments as for `huygens_psf`.  The result also gives the diffraction MTF
        (`HuygensStack.mtf`)."""
        table = SectionTable(self)
        focus, radius, size, dz, bands = _psf.check_stack_arguments(table.nt, section, focus, radius, n_px, size, dz, bands)
        Ns, Ne, k, origin, label = self._section_bundle(table, source_index, section, "the point spread function holds")
        return _psf.analyse_stack(self.rays, Ns, Ne - Ns, k, origin, focus, radius, n_px, size, dz, bands,
                                  long_desc=f"Huygens PSF stack of {label} behind section {k}")

    def footprints(self, source_index: int = None, n_px: int = None) -> Footprints:
        """Beam footprint and power budget at every surface, of one source's rays or of all (None), no counterpart in optrace:
        per section of the stored trace the rays alive and arriving with their power, and centroid, extent, RMS size and largest
        distance from the surface's axis of where the living rays cross the surface, reduced on the GPU from the position and
        weight planes (footprint.py).  n_px: cells per side of a power map of every footprint (`Footprints.image`), 1 to 1024;
        None: no maps."""
        _footprint.check_arguments(source_index, n_px)
        require_device()  # (said before anything about the rays: without a device there are none)
        Ns, Ne = self._stored_range(source_index)
        table, who = SectionTable(self), self._rays_tag(source_index)
        axis, radii = table.axes_and_radii(source_index)
        labels = table.labels("sources" if source_index is None else who)
        return _footprint.analyse(self.rays, Ns, Ne - Ns, axis, n_px, labels, radii, long_desc=f"Footprints of {who}")

    def chromatic_analysis(self, source_index: int = 0, section: int = None, bands="lines", z: float = None,
                           reference: float = None) -> ChromaticAnalysis:
        """Chromatic focal shift and lateral colour of one source's rays (None: all rays), no counterpart in optrace: per band of
        wavelengths the point closest to the band's ray lines, and centroid, RMS size and largest radius of where the band
        crosses a common plane, reduced on the GPU from the position, weight and wavelength planes of one section (chromatic.py).
        section: as for `wavefront_analysis`; bands: as for `huygens_stack`, "lines", a number of equal bands or ascending edges
        in nm, 32 bands at the most; z: absolute z of the plane, default the focus z of the reference band; reference: a
        wavelength in nm, the band with rays whose mean wavelength lies nearest to it is the one the shifts refer to, default
        the power-weighted mean wavelength of the used rays."""
        table = SectionTable(self)
        bands, z, reference = _chromatic.check_arguments(table.nt, section, bands, z, reference)
        Ns, Ne, k, origin, label = self._section_bundle(table, source_index, section, "the chromatic figures hold")
        return _chromatic.analyse(self.rays, Ns, Ne - Ns, k, origin, bands, z, reference,
                                  long_desc=f"Chromatic analysis of {label} behind section {k}")

    def field_analysis(self, sources=None, section: int = None, bands="lines", z: float = None, reference: float = None,
                       reference_field: int = 0, paraxial: str = "tma") -> FieldAnalysis:
        """How the image changes across the field, no counterpart in optrace: every chosen ray source is a field point, and per
        field point and band of wavelengths the tangential, sagittal and best-RMS focus (astigmatism, field curvature), the
        centroid on a common plane against its paraxial image (distortion), the spot size and the power (relative illumination)
        are reduced on the GPU in one call, from the position, weight and wavelength planes of one section (field.py).
        sources: None for every ray source or 1 to 64 distinct source indices, the field points in that order; section: as for
        `wavefront_analysis`; bands, reference: as for `chromatic_analysis`, the bands assigned over the used rays of all chosen
        fields together; reference_field: index into `sources` of the field the curvatures and the illumination refer to; z:
        absolute z of the common plane, default the best-RMS focus of the reference field in the reference band; paraxial: "tma"
        for paraxial image points from the transfer matrix analysis of the geometry (NaN where it has none), None for none."""
        table = SectionTable(self)
        sources, bands, z, reference = _field.check_arguments(table.nt, len(self.ray_sources), sources, section, bands, z, reference,
                                                              reference_field, paraxial)
        ranges, k, axis, positions, tangents, field, power = self._field_points(table, sources, section)

        def matrix_at(wl, z_g, z_b):
            try:
                return self.tma(wl).matrix_at(z_g, z_b)
            except Exception:  # (no lenses, no symmetry, a plane inside a lens: no paraxial image, which the result says with NaN)
                return None

        return _field.analyse(self.rays, ranges, k, table.origin(k, None), bands, z, reference, reference_field, sources, field,
                              power, positions, tangents, matrix_at if paraxial == "tma" else None, axis,
                              long_desc=f"Field analysis of {', '.join(self._rays_tag(s) for s in sources)} behind section {k}")

    def _field_points(self, table: SectionTable, sources, section):
        """What the analyses per field point share, after their argument checks: the device, current rays, and per chosen source
        its ray range, its position relative to the optical axis, its direction tangents (NaN without a constant orientation),
        its field vector and its power.  -> (ranges, k, axis, positions, tangents, field, power)"""
        require_device()  # (said before anything about the rays: without a device there are none)
        ranges = []
        for s in sources:
            Ns, Ne = self._stored_range(s)
            ranges.append((Ns, Ne - Ns))
        k = table.nt - 2 if section is None else section
        axis = np.array(self.lenses[0].pos[:2], dtype=np.float64) if self.lenses else np.zeros(2)
        positions, tangents, field, power = [], [], [], []
        for s in sources:
            rs = self.ray_sources[s]
            pos = np.array(rs.pos, dtype=np.float64) - [axis[0], axis[1], 0.0]
            sv = np.array(rs.s, dtype=np.float64)
            with np.errstate(invalid="ignore", divide="ignore"):
                tan = sv[:2] / sv[2] if rs.orientation == "Constant" else np.full(2, np.nan)
            positions.append(pos)
            tangents.append(tan)
            field.append(pos[:2] if np.any(pos[:2] != 0) else tan)
            power.append(float(rs.power))
        return ranges, k, axis, positions, tangents, field, power

    def mtf_analysis(self, sources=None, section: int = None, bands="lines", frequencies=None, z: float = None, dz=None,
                     reference: float = None, reference_field: int = 0) -> MTFAnalysis:
        """Geometric MTF across the field and through focus, no counterpart in optrace: every chosen ray source is a field point,
        and per field point, band of wavelengths, plane and spatial frequency the contrast along the tangential direction of the
        field and across it is reduced on the GPU in one call, from the position, weight and wavelength planes of one section
        (mtf.py); the result adds the bands to the polychromatic MTF of every field and finds the through-focus peak.
        sources, section, bands, reference, reference_field, z: as for `field_analysis`, z by default the best-RMS focus of the
        reference field in the reference band; dz: None for the plane z alone or 1 to 65 strictly increasing offsets, the planes
        lie at z + dz; frequencies: 1 to 64 values of 0 or above in cycles per mm, default 17 equal steps from 0 to one over the
        RMS radius of the reference field in the reference band on the plane z."""
        table = SectionTable(self)
        sources, bands, z, reference = _field.check_arguments(table.nt, len(self.ray_sources), sources, section, bands, z, reference,
                                                              reference_field, None)
        frequencies, dz = _mtf.check_arguments(frequencies, dz)
        ranges, k, axis, positions, tangents, field, power = self._field_points(table, sources, section)
        return _mtf.analyse(self.rays, ranges, k, table.origin(k, None), bands, frequencies, z, dz, reference, reference_field, sources,
                            field, power,
                            long_desc=f"MTF analysis of {', '.join(self._rays_tag(s) for s in sources)} behind section {k}")

    def spot_diagram(self, sources=None, section: int = None, bands="lines", z: float = None, dz=None, n_px: int = 64,
                     size: float = None, centre="centroid", reference: float = None, reference_field: int = 0) -> SpotDiagram:
        """Spot diagrams across the field and through focus, no counterpart in optrace: every chosen ray source is a field point,
        and per field point, band of wavelengths and plane the rays are binned on the GPU in one call into a power map of n_px x
        n_px cells about a centre, all tiles at one common scale, from the position, weight and wavelength planes of one section
        (spot_diagram.py); with the rays outside a tile, their power, and the largest and the RMS distance from the centre.
        sources, section, bands, reference, reference_field, z: as for `field_analysis`; dz: as for `mtf_analysis`; n_px: 1 to
        1024 cells per side; size: the side of every tile in mm, default slightly above twice the largest distance of any ray
        from the centre of its tile; centre: what every tile is drawn about, per field and plane -- "centroid": the
        power-weighted mean of the rays of all bands, "band": each band's own centroid, "reference": the centroid of the
        reference band, or an array (F, 2) of absolute points, the same on every plane."""
        table = SectionTable(self)
        sources, bands, z, reference = _field.check_arguments(table.nt, len(self.ray_sources), sources, section, bands, z, reference,
                                                              reference_field, None)
        _, dz = _mtf.check_arguments(None, dz)
        n_px, size, centre = _spot_diagram.check_arguments(n_px, size, centre, len(sources))
        ranges, k, axis, positions, tangents, field, power = self._field_points(table, sources, section)
        return _spot_diagram.analyse(self.rays, ranges, k, table.origin(k, None), bands, z, dz, n_px, size, centre, reference,
                                     reference_field, sources, field, power,
                                     long_desc=f"Spot diagram of {', '.join(self._rays_tag(s) for s in sources)} behind section {k}")

    def wavefront_field(self, sources=None, section: int = None, bands="lines", n_zernike: int = 15, sphere: str = "field",
                        focus=None, radius=None, pupil_radius: float = None, reference: float = None,
                        reference_field: int = 0) -> WavefrontField:
        """Wavefront error across the field and the bands of wavelengths, no counterpart in optrace: every chosen ray source is a
        field point, and per field point and band the optical path difference against a reference sphere, its RMS, extremes and
        Strehl ratio and the Zernike coefficients of a least-squares fit on a pupil common to the bands of a field are reduced on
        the GPU in one call (wavefront_field.py).  sources, section, bands, reference, reference_field: as for `field_analysis`;
        n_zernike: Noll polynomials fitted, 1 to 36; sphere: "field" -- all bands of a field share the sphere of the field's
        reference band, so that axial colour shows as defocus (Z4) and lateral colour as tilt (Z2, Z3) -- or "band", every cell
        against its own sphere; the sphere of a cell is that of `wavefront_analysis`, the point closest to its ray lines and its
        signed distance from their mean start, and a collimated cell has none (its rays are counted in `n_no_sphere`); focus
        (F, 3), radius (F,) or one number: centre and signed radius per field for all its bands, in place of the found ones;
        pupil_radius: radius of the unit disc in units of |radius|, default per field the largest distance from the pupil
        centre."""
        table = SectionTable(self)
        sources, bands, _, reference = _field.check_arguments(table.nt, len(self.ray_sources), sources, section, bands, None, reference,
                                                              reference_field, None)
        focus, radius, pupil_radius = _wavefront_field.check_arguments(len(sources), n_zernike, sphere, focus, radius, pupil_radius)
        ranges, k, axis, positions, tangents, field, power = self._field_points(table, sources, section)
        if table.ideal_before(k):
            warning(f"An ideal lens lies before section {k}: the optical path through an ideal lens is not defined, "
                    f"the wavefront figures hold up to what it would add.")
        return _wavefront_field.analyse(self.rays, ranges, k, table.origin(k, None), bands, n_zernike, sphere, focus, radius,
                                        pupil_radius, reference, reference_field, sources, field,
                                        long_desc=f"Wavefront of {', '.join(self._rays_tag(s) for s in sources)} behind section {k}")

    def huygens_field(self, sources=None, section: int = None, bands="lines", n_px: int = 64, size: float = None, dz=0.0,
                      focus=None, radius=None, frequencies=None, reference: float = None,
                      reference_field: int = 0) -> HuygensField:
        """Huygens PSF and diffraction MTF across the field, no counterpart in optrace: every chosen ray source is a field point, and
        per field point the polychromatic through-focus diffraction image of `huygens_stack` about a reference sphere of the
        field's own is summed on the GPU in one call for all fields, bands and planes, with its transfer function along the
        field's tangential direction and across it (psf_field.py).  sources, section, bands, reference, reference_field: as for
        `field_analysis`; n_px, dz: as for `huygens_stack`, the planes of a field lie at its focus z + dz; size: the side of every
        tile in mm, default the largest over the fields of ten mean wavelengths over the pupil radius; focus (F, 3), radius (F,)
        or one number: centre and signed radius of the sphere per field, default that of `wavefront_field(sphere="field")`, the
        sphere of the field's reference band for all its bands -- axial colour shows as each band's defocus, lateral colour as
        its offset inside the tile --, and a collimated field has none (its rays are counted in `n_no_sphere`); frequencies: 1
        to 64 values of 0 or above in cycles per mm, none above the sampling limit n_px / (2 size), default 17 equal steps from 0
        to that limit.  `HuygensField.grid()` is what `ot.convolve_field` takes."""
        table = SectionTable(self)
        sources, bands, _, reference = _field.check_arguments(table.nt, len(self.ray_sources), sources, section, bands, None, reference,
                                                              reference_field, None)
        size, dz, focus, radius, frequencies = _psf_field.check_arguments(table.nt, len(sources), section, n_px, size, dz, focus, radius,
                                                                          frequencies)
        ranges, k, axis, positions, tangents, field, power = self._field_points(table, sources, section)
        if table.ideal_before(k):
            warning(f"An ideal lens lies before section {k}: the optical path through an ideal lens is not defined, "
                    f"the wavefront figures hold up to what it would add.")
        return _psf_field.analyse(self.rays, ranges, k, table.origin(k, None), bands, n_px, size, dz, focus, radius, frequencies,
                                  reference, reference_field, sources, field,
                                  long_desc=f"Huygens PSF of {', '.join(self._rays_tag(s) for s in sources)} behind section {k}")

    def ray_fans(self, source_index: int = 0, section: int = None, bands="lines", focus=None, radius: float = None,
                 n_bins: int = 32, slab: float = 0.1, pupil_radius: float = None) -> RayFans:
        """Ray aberration fans of one source's rays (None: all rays), no counterpart in optrace: per band of wavelengths the
        transverse ray aberration in the plane of the focus and the optical path difference against the pupil coordinate, along
        the tangential and the sagittal cut of the pupil, and the band's own wavefront and spot figures, reduced on the GPU
        (fans.py).  section, focus, radius, pupil_radius: as for `wavefront_analysis`, one reference sphere and one pupil for all
        bands; bands: as for `chromatic_analysis`; n_bins: bins over the pupil coordinate -1 .. 1, 1 to 256; slab: half width of
        a cut in units of the pupil radius, above 0 and at most 1."""
        table = SectionTable(self)
        bands, focus, radius, slab, pupil_radius = _fans.check_arguments(table.nt, section, bands, focus, radius, n_bins, slab,
                                                                         pupil_radius)
        Ns, Ne, k, origin, label = self._section_bundle(table, source_index, section, "the ray fans hold")
        return _fans.analyse(self.rays, Ns, Ne - Ns, k, origin, bands, focus, radius, n_bins, slab, pupil_radius,
                             long_desc=f"Ray fans of {label} behind section {k}")

    def _section_bundle(self, table: SectionTable, source_index, section, holds: str):
        """What the analyses of a stored section share, after their own argument checks against `table.nt`: the device, current
        rays, the ray range of the source, the section (default: the space behind the last surface), a point near its start and a
        label.  Warns of an ideal lens before the section.  -> (Ns, Ne, k, origin, label)"""
        if source_index is not None:
            check_type("source_index", source_index, int)
        require_device()  # (said before anything about the rays: without a device there are none)
        Ns, Ne = self._stored_range(source_index)
        k = table.nt - 2 if section is None else section
        if table.ideal_before(k):
            warning(f"An ideal lens lies before section {k}: the optical path through an ideal lens is not defined, "
                    f"{holds} up to what it would add.")
        return Ns, Ne, k, table.origin(k, source_index), self._rays_tag(source_index)

    # ---- source side (raytracer.py:1281-1352) ---------------------------------------------------------------
    def _hit_source(self, info: str, source_index: int = 0):
        """Section-0 device views of one source's rays: ((x, y), w, wl, extent)  (raytracer.py:1281-1309)."""
        Ns, Ne = self._stored_range(int(source_index))
        N, nt, d = self.rays._Np, self.rays.Nt, self.rays._dev  # (N: the plane stride of the storage)
        # element (ray r, section i, component c) of p lives at r + N * (i + nt * c); section 0 here
        xy = d["p"][Ns:Ne], d["p"][N * nt + Ns:N * nt + Ne]
        return xy, d["w"][Ns:Ne], d["wl"][Ns:Ne], self.ray_sources[source_index].extent[:4]

    def _source_label(self, source_index: int) -> str:
        source = self.ray_sources[source_index]
        title = f": {source.desc}" if source.desc else ""
        return f"{RaySource.abbr}{source_index}{title} at z = {source.pos[2]:.5g} mm"

    def source_spectrum(self, source_index: int = 0, **kwargs) -> LightSpectrum:
        """Spectrum emitted by a source, from its traced rays (raytracer.py:1311-1329)."""
        _, w, wl, _ = self._hit_source("Source Spectrum", source_index)
        return LightSpectrum.render(wl, w, long_desc="Spectrum of " + self._source_label(source_index), **kwargs)

    def source_image(self, source_index: int = 0, limit: float = None, **kwargs) -> RenderImage:
        """Image of a source's emitting area, from its traced rays (raytracer.py:1331-1352)."""
        xy, w, wl, extent = self._hit_source("Source Image", source_index)
        image = RenderImage(long_desc=self._source_label(source_index), extent=extent, projection=None)
        image.render(xy, w, wl, limit=limit, **kwargs)
        return image

    # ---- focus search (raytracer.py:1354-1640) ----------------------------------------------------------------
    focus_search_methods = ['RMS Spot Size', 'Irradiance Variance', 'Image Sharpness', 'Image Center Sharpness']

    def focus_search(self, method: str, z_start: float, source_index: int = None, return_cost: bool = False,
                     _z_samples: np.ndarray = None):
        """Find the focal position around `z_start` (raytracer.py:1463-1640).

        The search region is the gap between the tracing surfaces (or sources / outline) around z_start.
        Per ray the section crossing that gap is turned into the line ph(z) = pa + sb * z on the device
        (`ot_focus_prepare`); every cost evaluation -- the 320 samples of the cost curve as well as each step
        of SciPy's scalar optimisers -- is a chain of streaming kernels over those lines (`ot_focus_cost`).
        `_z_samples` injects the sample positions of the cost curve (parity runs against recorded reference
        samples); by default they are stratified draws from NumPy's global RNG like the reference's.
        Returns (scipy OptimizeResult, dict(pos, bounds, z, cost, N))."""
        import scipy.optimize

        z_lo, z_hi = self.outline[4:]
        if z_start < z_lo or z_start > z_hi:
            raise ValueError(f"Starting position z_start={z_start} outside raytracer"
                             f" z-outline range {self.outline[4:]}.")
        if method not in self.focus_search_methods:
            raise ValueError(f"Invalid method '{method}', should be one of {self.focus_search_methods}.")
        self._need_rays()
        n_src = len(self.rays.N_list)
        if source_index is not None and source_index < 0:
            raise IndexError(f"source_index needs to be >= 0, but is {source_index}")
        if n_src == 0 or (source_index is not None and source_index >= n_src):
            raise IndexError(f"source_index={source_index} larger than number of simulated sources "
                             f"({len(self.rays.N_list)}. "
                             "Either the source was not added or the new geometry was not traced.")
        self._need_current(" or last trace had errors")

        # the search runs in the free gap around z_start: from the last surface (or source end) before it to the
        # first surface (or the outline's far face) behind it
        bounds = SectionTable(self).gap(z_start, self.outline[5], self.N_EPS)

        Nt = 320  # cost function sampling points
        Ns, Ne = self._ray_range(source_index)
        n = Ne - Ns

        lib = _capi.load_library()
        dev = require_device()
        pasb = torch.empty(4 * n, dtype=torch.float64, device=dev)
        w = torch.empty(n, dtype=torch.float32, device=dev)
        n_use_d = torch.empty(1, dtype=torch.int64, device=dev)
        rays = self.rays._rays_struct()
        _capi.check(lib.ot_focus_prepare(C.byref(rays), Ns, n, bounds[0] + self.N_EPS, ptr(pasb), ptr(w), ptr(n_use_d),
                                         stream_ptr()))
        N_use = int(n_use_d.item())
        if N_use < 1000:
            warning(f"WARNING: Less than 1000 rays for focus_search ({N_use}).")
        if N_use <= 1:  # nothing to focus: an empty result with the reference's keys
            nan_curve = np.full(Nt, np.nan)
            return scipy.optimize.OptimizeResult(), dict(pos=[np.nan] * 3, bounds=bounds, z=nan_curve,
                                                         cost=nan_curve.copy(), N=N_use)

        mode = self.focus_search_methods.index(method)
        # image side grows with sqrt(N) (raytracer.py:1381-1385), odd
        N_px = 100 * int(1 + np.sqrt(N_use) / 1500)
        N_px = N_px if N_px % 2 else N_px + 1
        ws = torch.empty(_capi.FOCUS_WS + N_px * N_px, dtype=torch.float64, device=dev)

        # weighted moments of the hit lines: mean line, direct RMS solution, and the whole RMS cost curve
        sums = torch.empty(16, dtype=torch.float64, device=dev)
        _capi.check(lib.ot_focus_moments(n, ptr(pasb), ptr(w), bounds[0], bounds[1], ptr(sums), stream_ptr()))
        sm = sums.cpu().numpy()

        def cost_at(zs: np.ndarray) -> np.ndarray:
            zs = np.ascontiguousarray(zs, dtype=np.float64)
            if mode == 0:
                # RMS spot size sqrt(var_x + var_y) with np.cov(aweights) normalisation (raytracer.py:1376-1379):
                # the centred second moments are quadratic in z, one pass over the rays serves every z
                dz = zs - 0.5 * (bounds[0] + bounds[1])
                fact = sm[0] - sm[7] / sm[0]
                var = (sm[8] + sm[11] + 2 * dz * (sm[9] + sm[12]) + dz ** 2 * (sm[10] + sm[13])) / fact
                return np.sqrt(np.maximum(var, 0.0))
            out = torch.empty(zs.shape[0], dtype=torch.float64, device=dev)
            _capi.check(lib.ot_focus_cost(n, ptr(pasb), ptr(w), mode,
                                          zs.ctypes.data_as(C.POINTER(C.c_double)), zs.shape[0], N_px, ptr(ws), ptr(out),
                                          stream_ptr()))
            return out.cpu().numpy()

        r = vals = None
        needs_curve = mode >= 2  # the sharpness methods start their optimiser at the best sample of the curve
        if return_cost or needs_curve:
            if _z_samples is not None:
                r = np.asarray(_z_samples, dtype=np.float64)
            else:  # random.stratified_interval_sampling(b0, b1, Nt, shuffle=False), random.py:48-67
                dba = (bounds[1] - bounds[0]) / Nt
                r = np.linspace(bounds[0], bounds[1] - dba, Nt) + np.random.uniform(0., dba, Nt)
            vals = cost_at(r)

        if mode == 0:
            # RMS spot size: direct solution, extended by ray weights (raytracer.py:1420-1460)
            z_best = -sm[6] / sm[5] if sm[5] else 0.5 * (bounds[0] + bounds[1])
            z_best = float(min(max(z_best, bounds[0]), bounds[1]))
            res = scipy.optimize.OptimizeResult(x=z_best, fun=float(cost_at(np.array([z_best]))[0]))
        else:
            def scalar_cost(z, *_):
                return float(cost_at(np.array([z[0]]))[0])

            # same optimisers and limits as the reference: Nelder-Mead from the middle of the gap for the irradiance
            # variance, COBYLA from the best curve sample for the sharpness methods
            if mode == 1:
                start, solver, steps = 0.5 * (bounds[0] + bounds[1]), "Nelder-Mead", 100
            else:
                start, solver, steps = r[int(np.argmin(vals))], "COBYLA", 30
            res = scipy.optimize.minimize(scalar_cost, start, method=solver, bounds=[bounds], tol=None, callback=None,
                                          options=dict(maxiter=steps))
            res.x = res.x[0]

        rrl = (res.x - bounds[0]) < 10 * (bounds[1] - bounds[0]) / Nt
        rrr = (bounds[1] - res.x) < 10 * (bounds[1] - bounds[0]) / Nt
        if rrl or rrr:
            warning("Found minimum near search bounds, "
                    "this can mean the focus is outside of the search range.")

        # weighted mean ray position at the focus; the z component of pa + sb * z is z itself
        pos = (float((sm[1] + sm[3] * res.x) / sm[0]), float((sm[2] + sm[4] * res.x) / sm[0]), float(res.x))
        if not return_cost:
            r = vals = None
        return res, {"pos": pos, "bounds": bounds, "z": r, "cost": vals, "N": N_use}

    # ---- iterative rendering (raytracer.py:1134-1279) -------------------------------------------------------
    def _render_only_applies(self, detector_index: list, pos: list) -> bool:
        """May the chunks of an iterative render be traced without storing their sections (`ITER_RENDER_ONLY`)?  A
        detector sees a ray through the section that crosses it (raytracer.py:929-985); behind the last tracing surface
        that is the ray's last section, which is all a render-only trace keeps."""
        if any(rs.orientation == "Function" for rs in self.ray_sources):  # (their generation needs a position pre-pass)
            return False
        z_last = SectionTable(self).z_last()
        for k, p in zip(detector_index, pos):
            if not 0 <= k < len(self.detectors):  # (reported by the detector pass, after the trace like the reference)
                return False
            surf = self.detectors[k].surface
            if float(p[2]) + (surf.z_min - surf.pos[2]) <= z_last + self.N_EPS:
                return False
        return True

    def _chunk_plan(self, N: int, n_sec: int, render_only: bool) -> list:
        """Ray counts of the chunks of an iterative render of N rays (raytracer.py:1216-1217, 1238-1239): with
        ITER_RAYS_STEP set, the reference's rule; otherwise chunks sized by storage -- with render-only chunks: as large as
        ITER_STORAGE_BYTES of tail storage and one launch allow, then one stored chunk of ITER_LAST_RAYS."""
        rays_step = self.ITER_RAYS_STEP  # None: sized by storage
        if rays_step is not None:  # the reference's rule (raytracer.py:1216-1217, 1238-1239)
            iterations = max(N // rays_step, 1)
            chunks = [rays_step] * (iterations - 1) + [N - (iterations - 1) * rays_step]
        elif render_only and N > self.ITER_LAST_RAYS:
            # one stored chunk of ITER_LAST_RAYS at the end; before it render-only chunks as large as ITER_STORAGE_BYTES
            # of tail storage (60 B per ray at most) and one launch (2^28 rays) allow
            rest = N - self.ITER_LAST_RAYS
            most = min(1 << 28, self.ITER_STORAGE_BYTES // 60) // 1024 * 1024
            k = -(-rest // most)
            step = -(-(-(-rest // k)) // 1024) * 1024
            chunks = [step] * (k - 1) + [rest - (k - 1) * step] + [self.ITER_LAST_RAYS]
        else:
            # chunk = what ITER_STORAGE_BYTES of ray storage hold (the reference's 1 M rays are sized for a few GB of
            # host RAM, raytracer.py:40); chunks of equal size, at least 1 M rays
            step_max = max(1_000_000, self.rays.max_rays_for_size(self.ITER_STORAGE_BYTES, n_sec, self.no_pol))
            iterations = -(-N // step_max)
            rays_step = -(-N // iterations)
            if iterations > 1:
                # a multiple of 1024 rays: the planes of the storage then start on 128-byte lines.  With an odd count
                # every wave's store straddles a line it shares with its neighbour (C4: 66 666 667 rays traced in 4.8
                # ms, 66 666 688 in 3.4 ms); the last chunk takes what is left
                rays_step = -(-rays_step // 1024) * 1024
            chunks = [rays_step] * (iterations - 1) + [N - (iterations - 1) * rays_step]
        return chunks

    def iterative_render(self, N, detector_index=0, limit=None, projection_method="Equidistant", pos=None,
                         extent=None, _power_scale: float = 1.0, _agree_extents=None, _finish: bool = True) -> list:
        """Render detector images from N rays traced in chunks of ITER_RAYS_STEP; images of all chunks
        are summed (the extent of the first chunk fixes later ones)."""
        if not self.ray_sources:
            raise RuntimeError("Ray Source(s) Missing.")
        if not self.detectors:
            raise RuntimeError("Detector(s) Missing.")
        if (N := int(N)) <= 0:
            raise ValueError(f"Ray number N_rays needs to be a positive int, but is {N}.")

        # one image per detector position: scalars are repeated, lists must have one entry per position
        if pos is None:
            if isinstance(detector_index, list):
                raise ValueError("detector_index list needs to have the same length as pos list")
            pos = [np.array(self.detectors[detector_index].pos)]
        elif not isinstance(pos[0], (list, np.ndarray)):
            pos = [pos]
        n_img = len(pos)

        def per_image(value, name, is_list):
            if not is_list:
                return [value] * n_img
            if len(value) != n_img:
                raise ValueError(f"{name} list needs to have the same length as pos list")
            return list(value)

        detector_index = per_image(detector_index, "detector_index", isinstance(detector_index, list))
        limit = per_image(limit, "limit", isinstance(limit, list))
        projection_method = per_image(projection_method, "projection_method", isinstance(projection_method, list))
        # (an extent is itself a list of numbers: only a list of extents counts as one)
        extentc = per_image(extent, "extent", isinstance(extent, list) and not isinstance(extent[0], (int, float)))

        n_sec = SectionTable(self).nt
        if not self._scene_unchanged() and self._pretrace_check(min(N, 1000), self._geometry_key()):
            raise RuntimeError("Geometry checks failed. Tracing aborted. Check the warnings.")
        # Only the rays of the LAST chunk stay in the tracer (raytracer.py:1235-1267).  Every chunk before it is traced
        # render-only where the scene and the detector positions allow it: no section is stored, the living rays' last
        # sections go to a compact storage the detector passes read (`trace(_tail=...)`, TailStorage)
        render_only = self.ITER_RENDER_ONLY and self._render_only_applies(detector_index, pos)
        chunks = self._chunk_plan(N, n_sec, render_only)
        tail = TailStorage() if render_only and len(chunks) > 1 else None

        nt = n_sec
        msgs_cum = np.zeros((len(self.INFOS), n_sec), dtype=int)

        # Up to 8 positions are intersected in one pass over the sections, hit search and binning fused (`ot_detector_images`);
        # the extents are given by the caller or fixed by the first chunk (raytracer.py:1262).  The reference scales every
        # chunk's image by rays_step / N and adds it (raytracer.py:1257-1264); here the factor rides with the weights into the
        # binning (`weight_scale`, applied in f64), so that every chunk is binned straight into the one image of its position:
        # no second set of histograms, no passes over them.  The host side of a group of positions -- detectors moved, images
        # with their grids, one zero-filled allocation, the request records -- is a PLAN made once (`_plan_renders`): before
        # the first trace where the caller gave the extents, right after it otherwise, and launched chunk after chunk (the
        # gap between a trace and its binning was 0.15-0.3 ms of host work per chunk: a fifth of a rank's time when 2e8 rays
        # are sharded over eight GPUs).
        groups = [list(range(j0, min(j0 + self.ITER_GROUP, len(pos)))) for j0 in range(0, len(pos), self.ITER_GROUP)]
        plans = [None] * len(groups)
        images = [None] * len(pos)

        def specs_of(group):
            return [dict(detector_index=detector_index[j], extent=extentc[j], projection_method=projection_method[j],
                         pos=pos[j]) for j in group]

        def make_plan(gi, specs):
            plans[gi] = self._plan_renders(specs, [limit[j] for j in groups[gi]], whole_storage=True)
            for g, j in enumerate(groups[gi]):
                images[j] = plans[gi]["images"][g]
                extentc[j] = images[j]._extent0

        for gi, group in enumerate(groups):
            if all(extentc[j] is not None for j in group):
                make_plan(gi, specs_of(group))

        # The LAST chunk goes through the ray storage (its rays stay in the tracer), but not through a binning pass of its
        # own: it is traced FIRST, the last sections of its living rays later join the tail of the final render-only chunk
        # (weights scaled to that chunk's rays: x n_last / n_i), and the two are binned together -- for 2^20 rays the fixed
        # costs of the tile chain were most of the pass (0.3-0.4 ms per render).  Automatic extents are those of this
        # stored chunk's hits (the reference takes its first iteration's, 1 M rays as well, raytracer.py:1262): its rays
        # have the order of generation, so a seeded render finds the same extents every time -- the slots of a tail
        # storage are filled in the order the waves happen to finish
        merged = tail is not None and self.ITER_MERGE_LAST

        def bin_chunk(n_i, src):
            self._rays_known_current = True  # traced a moment ago: skip the snapshot comparison per image
            try:
                for gi, group in enumerate(groups):
                    if plans[gi] is None:  # automatic extents: those of this, the first chunk (an extent-only pass or a sample)
                        make_plan(gi, self._auto_extents(specs_of(group), agree=_agree_extents,
                                                         sample_rays=self.ITER_EXTENT_RAYS, rays=src))
                    if n_i:
                        self._launch_renders(plans[gi], rays=src, weight_scale=n_i / N)
            finally:
                self._rays_known_current = False

        if merged:
            n_last = chunks[-1]
            with global_options.no_warnings():
                self.trace(N=n_last, _chunk=len(chunks) - 1, _power_scale=_power_scale)
                msgs_cum += self._msgs
            bin_chunk(0, None)  # (plans with automatic extents only; nothing is binned yet)
        for i, n_i in enumerate(chunks):  # one chunk of rays per iteration (raytracer.py:1235-1267)
            last = i == len(chunks) - 1
            if merged and last:
                break  # (traced at the start, binned with the chunk before it)
            src = tail if (tail is not None and not last) else None
            with global_options.no_warnings():
                if merged and i == len(chunks) - 2:
                    self.trace(N=n_i, _chunk=i, _power_scale=_power_scale, _tail=src, _tail_room=n_last + 64)
                    msgs_cum += self._msgs
                    src.append_living(self.rays, n_last / n_i)
                else:
                    self.trace(N=n_i, _chunk=i, _power_scale=_power_scale, _tail=src)
                    msgs_cum += self._msgs
            bin_chunk(n_i, src)
        if tail is not None:
            tail.release()

        self._msgs = msgs_cum
        if not _finish:  # distributed.sharded_iterative_render: histograms still on the device, summed over the ranks first
            return images
        for i, img in enumerate(images):
            img._sync_host()
            if limit[i] is not None:
                img._apply_rayleigh_filter()

        self._show_messages(N)
        return images
