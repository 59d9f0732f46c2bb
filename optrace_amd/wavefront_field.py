"""Wavefront across the field: per field point (the rays of one source) and band of wavelengths the optical path difference against
a reference sphere, its RMS and peak-to-valley, the Strehl ratio and a Zernike decomposition on a pupil common to the bands of a
field -- coma against field, axial colour as a defocus term per line --, reduced on the device in one call for all fields and
bands.

`Raytracer.wavefront_field` has no counterpart in optrace.  Definition: DESIGN.md, "Wavefront across the field".  Kernels:
csrc/ot_wavefield.hpp behind `ot_wavefield_*`; fields, used rays, bands and the reference band are those of the field analysis
(`field.band_records`), the sphere of a cell and the solve of its normal equations those of the wavefront analysis
(`wavefront.closest_point`, `wavefront.unpack_normal_equations`).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from . import chromatic as _chromatic
from . import field as _field
from . import wavefront as _wavefront
from ._warn import warning
from .base import BaseClass, check_type, check_not_below, check_not_above

SPHERES = ("field", "band")
NAMED = dict(tilt=(2, 3), defocus=(4,), astigmatism=(5, 6), coma=(7, 8), spherical=(11,))  # Noll indices of the named terms


def check_arguments(n_fields: int, n_zernike, sphere, focus, radius, pupil_radius):
    """Argument checks of `Raytracer.wavefront_field` beyond `field.check_arguments`, host only; n_fields: the chosen sources.
    -> (focus (F, 3) float64 or None, radius (F,) float64 or None, pupil_radius as a float or None)."""
    check_type("n_zernike", n_zernike, int)
    check_not_below("n_zernike", n_zernike, 1)
    check_not_above("n_zernike", n_zernike, _capi.WF_MAX_J)
    if sphere not in SPHERES:
        raise ValueError(f"Property 'sphere' needs to be 'field' or 'band', but is '{sphere}'.")

    def real_array(key, val, shape):
        check_type(key, val, (list, tuple, np.ndarray))
        a = np.asarray(val)
        if not (np.issubdtype(a.dtype, np.floating) or np.issubdtype(a.dtype, np.integer)):
            raise TypeError(f"Property '{key}' needs to hold real numbers, but holds {a.dtype}.")
        if a.shape != shape:
            raise ValueError(f"Property '{key}' needs the shape {shape}, one entry per field, but has {a.shape}.")
        a = np.array(a, dtype=np.float64)
        if not np.all(np.isfinite(a)):
            raise ValueError(f"Property '{key}' needs to hold finite values only.")
        return a

    if focus is not None:
        focus = real_array("focus", focus, (n_fields, 3))
    if radius is not None:
        if isinstance(radius, (int, float, np.integer, np.floating)):
            radius = np.full(n_fields, _wavefront._finite_number("radius", radius, nonzero=True))
        else:
            radius = real_array("radius", radius, (n_fields,))
            if np.any(radius == 0):
                raise ValueError("Property 'radius' needs to hold non-zero values only.")
    if pupil_radius is not None:
        pupil_radius = _wavefront._finite_number("pupil_radius", pupil_radius, positive=True)
    return focus, radius, pupil_radius


def cell_sphere(sums, origin, focus=None, radius=None):
    """(c (3), signed R) of one cell from its 17 sums of `ot_wavefield_focus`, float64 host arithmetic: `wavefront.closest_point`
    behind the rank test of the chromatic analysis (`chromatic.band_foci`: a cell of one ray, or of rays of one direction, has no
    closest point, though rounding may leave the solver a pivot) and the radius rule of `wavefront.reference_sphere`, without
    their errors -- a cell without rays, a singular cell (a collimated bundle) or a focus in the mean start has four NaN.  focus,
    radius: the caller's, where given."""
    f = np.asarray(sums, dtype=np.float64)
    none = np.full(3, np.nan), np.nan
    if focus is None or radius is None:
        if not f[0] > 0:
            return none
    if focus is None:
        focus = _chromatic.band_foci(f[None], origin)[0]
        if not np.all(np.isfinite(focus)):
            return none
    if radius is None:
        with np.errstate(all="ignore"):
            d = focus - (origin + f[2:5] / f[0])
            radius = float(np.linalg.norm(d))
            if not (np.isfinite(radius) and radius > 0):
                return none
            if not d @ f[5:8] > 0:
                radius = -radius
    return np.array(focus, dtype=np.float64), float(radius)


def sphere_table(sums, origin, sphere: str, reference_band: int, focus=None, radius=None):
    """sums (F, K, 17) -> spheres (F, K, 4) = (c, R) per cell, NaN where there is none.  sphere "band": every cell its own;
    "field": all bands of a field that of the field's band `reference_band` (none there, or no reference band: none in the field).
    focus (F, 3), radius (F,): the caller's, for every band of the field."""
    sums = np.asarray(sums, dtype=np.float64)
    F, K = sums.shape[:2]
    out = np.full((F, K, 4), np.nan)
    for f in range(F):
        fo, ra = (None if focus is None else focus[f]), (None if radius is None else radius[f])
        for b in range(K):
            if fo is not None and ra is not None:
                out[f, b, :3], out[f, b, 3] = fo, ra
                continue
            src = b if sphere == "band" else reference_band
            if src < 0:
                continue
            c, R = cell_sphere(sums[f, src], origin, fo, ra)
            out[f, b, :3], out[f, b, 3] = c, R
    return out


class WavefrontField(BaseClass):
    """Result of `Raytracer.wavefront_field`; lengths in mm, wavelengths in nm, powers in W.  F field points, K bands of
    wavelengths; arrays have the shape (F, K) unless said otherwise.

    sources (F): the ray sources that are the field points; field (F, 2), t (F, 2): as in `FieldAnalysis`.  section: the section
    analysed.  band_edges (K + 1) or None for bands="lines".  n_zernike: the polynomials fitted, J.  sphere: "field" or "band".
    moments (F, K, 9), pupil (F, 4), normal (F, K, J (J + 1) / 2 + J): what the device returned (include/optrace_amd.h,
    ot_wavefield_moments and ot_wavefield_zernike).
    band_N, band_power: rays of a cell that met its sphere, and their power; n_missed: used rays whose line misses the sphere;
    n_no_sphere: used rays of a cell without a sphere (a collimated cell: pass `focus` and `radius`), which enter nothing else.
    wavelengths (K): power-weighted mean per band over all fields.  reference_band: as in `FieldAnalysis`, -1 when there is none.
    focus (F, K, 3), radius: centre and signed radius of the cell's reference sphere, NaN where it has none.
    opl_mean: weighted mean path to the sphere; opd_rms, opd_min, opd_max, opd_pv: weighted RMS, extremes and peak-to-valley of
    the path difference against that mean, the RMS exactly 0 for one ray; rms_waves, pv_waves: in units of the cell's own mean
    wavelength; strehl: exp(-(2 pi rms_waves)^2).  pupil_centre (F, 2), pupil_radius (F): the disc the polynomials live on, common
    to the bands of a field, in units of |radius|.  zernike (F, K, J): Noll-ordered orthonormal coefficients of the weighted
    least-squares fit in mm, zernike_waves: in units of the cell's mean wavelength; NaN for a singular cell.  rms_waves_all,
    strehl_all (F): polychromatic, sqrt(sum_b P_b rms_waves_b^2 / sum_b P_b) and sum_b P_b strehl_b / sum_b P_b over the bands
    with rays, P the band's power.
    A cell without a ray has band_N = band_power = 0 and NaN elsewhere."""

    _tracked = False

    def __init__(self, moments, counts, normal, pupil, spheres, n_zernike: int, reference_band: int, reference_field: int,
                 section: int, sources, field, sphere: str = "field", pupil_radius=None, band_edges=None, **kwargs) -> None:
        super().__init__(**kwargs)
        self.sources = np.array(sources, dtype=np.int64).reshape(-1)
        F = self.sources.shape[0]
        if not 1 <= F <= _capi.FIELD_MAX_FIELDS:
            raise ValueError(f"1 to {_capi.FIELD_MAX_FIELDS} fields, but there are {F}.")
        mom = np.array(moments, dtype=np.float64).reshape(F, -1, _capi.WFF_M)
        K = mom.shape[1]
        if not 1 <= K <= _capi.CHROM_MAX_BANDS:
            raise ValueError(f"1 to {_capi.CHROM_MAX_BANDS} bands, but the records hold {K}.")
        check_type("n_zernike", n_zernike, (int, np.integer))
        J = int(n_zernike)
        if not 1 <= J <= _capi.WF_MAX_J:
            raise ValueError(f"1 to {_capi.WF_MAX_J} polynomials, but there are {J}.")
        T = J * (J + 1) // 2 + J
        self.moments = mom
        self.normal = np.array(normal, dtype=np.float64).reshape(F, K, T)
        self.pupil = np.array(pupil, dtype=np.float64).reshape(F, _capi.WFF_PUPIL_M)
        counts = np.array(counts, dtype=np.int64).reshape(F, K, 2)
        spheres = np.array(spheres, dtype=np.float64).reshape(F, K, 4)
        self.band_edges = None if band_edges is None else np.array(band_edges, dtype=np.float64).reshape(-1)
        if self.band_edges is not None and self.band_edges.shape[0] != K + 1:
            raise ValueError(f"{K} bands need {K + 1} edges, but there are {self.band_edges.shape[0]}.")
        check_type("reference_band", reference_band, (int, np.integer))
        check_type("reference_field", reference_field, (int, np.integer))
        if not -1 <= reference_band < K:
            raise ValueError(f"Reference band {reference_band} out of range for {K} bands.")
        if not 0 <= reference_field < F:
            raise ValueError(f"Reference field {reference_field} out of range for {F} fields.")
        if sphere not in SPHERES:
            raise ValueError(f"Property 'sphere' needs to be 'field' or 'band', but is '{sphere}'.")
        self.n_fields, self.n_bands, self.n_zernike, self.section, self.sphere = F, K, J, int(section), sphere
        self.reference_band, self.reference_field = int(reference_band), int(reference_field)
        self.field = np.array(field, dtype=np.float64).reshape(F, 2)
        self.t = _field.directions(self.field)

        self.band_N, self.band_power = mom[:, :, 1].astype(np.int64), mom[:, :, 0].copy()
        self.n_missed, self.n_no_sphere = counts[:, :, 0].copy(), counts[:, :, 1].copy()
        self.focus, self.radius = spheres[:, :, :3].copy(), spheres[:, :, 3].copy()
        some, single = self.band_N > 0, self.band_N == 1
        nan = np.nan
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            W = np.where(some, self.band_power, nan)
            self.wavelengths = np.where(self.band_N.sum(axis=0) > 0, mom[:, :, 5].sum(axis=0) / mom[:, :, 0].sum(axis=0), nan)
            lam = mom[:, :, 5] / W * 1e-6  # the cell's own mean wavelength, mm
            self.opl_mean = mom[:, :, 2] / W
            self.opd_rms = np.where(single, 0.0, np.sqrt(mom[:, :, 8] / W))
            self.opd_min = np.where(some, mom[:, :, 6] - self.opl_mean, nan)
            self.opd_max = np.where(some, mom[:, :, 7] - self.opl_mean, nan)
            self.opd_pv = self.opd_max - self.opd_min
            self.rms_waves, self.pv_waves = self.opd_rms / lam, self.opd_pv / lam
            self.strehl = np.exp(-(2 * np.pi * self.rms_waves) ** 2)
            any_ray = some.any(axis=1)
            self.pupil_centre = np.where(any_ray[:, None], self.pupil[:, :2], nan)
            given = pupil_radius is not None
            self.pupil_radius = np.where(any_ray, float(pupil_radius) if given else self.pupil[:, 3], nan)
            P = np.where(some, self.band_power, 0.0)
            Pf = np.where(any_ray, P.sum(axis=1), nan)
            self.rms_waves_all = np.sqrt((P * np.where(some, self.rms_waves, 0.0) ** 2).sum(axis=1) / Pf)
            self.strehl_all = (P * np.where(some, self.strehl, 0.0)).sum(axis=1) / Pf

        self.zernike = np.full((F, K, J), nan)
        singular = False
        for f in range(F):
            for b in range(K):
                if not some[f, b]:
                    continue
                G, g = _wavefront.unpack_normal_equations(self.normal[f, b], J)
                try:
                    with np.errstate(all="ignore"):
                        a = np.linalg.solve(G, g)
                except np.linalg.LinAlgError:
                    a = None
                if a is None or not np.all(np.isfinite(a)):
                    singular = True
                else:
                    self.zernike[f, b] = a
        if singular:
            warning("The Zernike fit of at least one cell is singular (fewer distinct rays than polynomials): no coefficients there.")
        self.zernike_waves = self.zernike / lam[:, :, None]
        self.lock()

    def coefficient(self, j: int):
        """Coefficient of Noll's Z_j, 1 <= j <= n_zernike, in mm: (F, K)."""
        check_type("j", j, (int, np.integer))
        if not 1 <= j <= self.n_zernike:
            raise IndexError(f"Z_{j} is none of the {self.n_zernike} polynomials of the fit.")
        return self.zernike[:, :, j - 1].copy()

    def named(self) -> dict:
        """The classical terms, each (F, K) in mm: tilt = hypot(Z2, Z3), defocus = Z4, astigmatism = hypot(Z5, Z6), coma =
        hypot(Z7, Z8), spherical = Z11; NaN where the fit has fewer polynomials than the term needs."""
        out = {}
        for name, js in NAMED.items():
            if max(js) > self.n_zernike:
                out[name] = np.full((self.n_fields, self.n_bands), np.nan)
            elif len(js) == 1:
                out[name] = self.coefficient(js[0])
            else:
                out[name] = np.hypot(self.coefficient(js[0]), self.coefficient(js[1]))
        return out


def _empty(section: int, bands, n_zernike: int, sphere: str, reference_field: int, sources, field, pupil_radius=None,
           **kwargs) -> WavefrontField:
    """(the rule of `spot._empty`: what the caller fixed stays; bands given as edges keep them, else one band without a ray)"""
    edges = bands if isinstance(bands, np.ndarray) else None
    F, K, T = len(sources), 1 if edges is None else edges.shape[0] - 1, n_zernike * (n_zernike + 1) // 2 + n_zernike
    mom = np.zeros((F, K, _capi.WFF_M))
    mom[:, :, 8] = np.nan
    return WavefrontField(mom, np.zeros((F, K, 2), dtype=np.int64), np.zeros((F, K, T)), np.full((F, 4), np.nan),
                          np.full((F, K, 4), np.nan), n_zernike, -1, reference_field, section, sources, field, sphere, pupil_radius,
                          edges, **kwargs)


class Planes:
    """The dense planes of `launch` over the span of the fields, entry i ray lo + i: u, v, opl (float64), w (float32), key (uint8)
    on the device; not used: w = 0 and NaN elsewhere."""
    __slots__ = ("lo", "u", "v", "opl", "w", "key")


def launch(rays, flat, F: int, lo: int, span: int, gaps: bool, section: int, key8, K: int, spheres, n_zernike: int, pupil_radius):
    """`ot_wavefield_paths`, `_moments` and `_zernike` for the fields `flat` with the sphere table `spheres` (F, K, 4) on the host.
    -> (moments (F, K, 9), counts (F, K, 2) int64, normal (F, K, T), pupil (F, 4) on the host -- one read --, Planes)."""
    import torch
    from ._device import require_device, ptr, stream_ptr
    lib = _capi.load_library()
    dev = require_device()
    st = stream_ptr()
    J, cells = n_zernike, F * K
    T = J * (J + 1) // 2 + J
    R = rays._rays_struct()
    rays._dev["n"]  # (the index plane is written when it is read: this fills it if the trace left it stale)
    wl = rays._dev["wl"][lo:lo + span]
    P = Planes()
    P.lo, P.key = lo, key8
    # (entries of no field are left alone by the device: with gaps between the fields they are set here)
    planes = torch.full((3 * span,), np.nan, dtype=torch.float64, device=dev) if gaps else torch.empty(3 * span, dtype=torch.float64, device=dev)
    P.u, P.v, P.opl = planes[:span], planes[span:2 * span], planes[2 * span:]
    P.w = torch.zeros(span, dtype=torch.float32, device=dev) if gaps else torch.empty(span, dtype=torch.float32, device=dev)
    sizes = [cells * _capi.WFF_M, cells * 2, cells * T, F * _capi.WFF_PUPIL_M]
    res = torch.zeros(sum(sizes), dtype=torch.float64, device=dev)
    mom, counts, normal, pupil = res.split(sizes)
    d_sph = torch.as_tensor(np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1), device=dev)
    ws = torch.empty(max(1, lib.ot_wavefield_workspace(flat, F, K, J)), dtype=torch.float64, device=dev)
    _capi.check(lib.ot_wavefield_paths(C.byref(R), flat, F, section, ptr(key8), lo, K, ptr(d_sph), ptr(P.u), ptr(P.v), ptr(P.opl),
                                       ptr(P.w), ptr(counts), st))
    _capi.check(lib.ot_wavefield_moments(flat, F, ptr(P.u), ptr(P.v), ptr(P.opl), ptr(P.w), ptr(wl), ptr(key8), lo, K, ptr(ws),
                                         ptr(mom), ptr(pupil), st))
    pr = np.nan if pupil_radius is None else pupil_radius
    _capi.check(lib.ot_wavefield_zernike(flat, F, ptr(P.u), ptr(P.v), ptr(P.opl), ptr(P.w), ptr(key8), lo, K, ptr(mom), ptr(pupil),
                                         pr, J, ptr(ws), ptr(normal), st))
    h = res.cpu().numpy()
    m, c, g, p = np.split(h, np.cumsum(sizes)[:-1])
    return m.reshape(F, K, -1), c.view(np.int64).reshape(F, K, 2), g.reshape(F, K, T), p.reshape(F, -1), P


def analyse(rays, ranges, section: int, origin, bands, n_zernike: int, sphere: str, focus, radius, pupil_radius, reference,
            reference_field: int, sources, field, **kwargs) -> WavefrontField:
    """Figures of the fields `ranges` [(first, count), ...] of the storage `rays` behind section `section`; origin: the point the
    device subtracts before it sums positions; the other arguments as the checks returned them.  Reads of the device: those of
    `field.band_records` (fields, used rays, bands and the reference band are the field analysis'), one for the focus sums unless
    focus and radius are both given, one for everything else."""
    import torch
    from ._device import require_device, ptr, stream_ptr
    fixed = dict(reference_field=reference_field, sources=sources, field=field, pupil_radius=pupil_radius)
    front = _field.band_records(rays, ranges, section, origin, bands, reference)
    if front is None:
        return _empty(section, bands, n_zernike, sphere, **fixed, **kwargs)
    lib = _capi.load_library()
    dev = require_device()
    F, K, lo, keep = front.F, front.K, front.lo, front.keep
    some = [(a, n) for a, n in ranges if n > 0]
    span = max(a + n for a, n in some) - lo
    gaps = sum(n for _, n in some) != span
    ref = front.reference_band + keep.start if front.reference_band >= 0 else -1  # among the bands of the launch
    if focus is None or radius is None:
        d_sums = torch.zeros(F * K * _capi.WF_FOCUS_M, dtype=torch.float64, device=dev)
        ws = torch.empty(max(1, lib.ot_wavefield_workspace(front.flat, F, K, n_zernike)), dtype=torch.float64, device=dev)
        _capi.check(lib.ot_wavefield_focus(C.byref(front.R), front.flat, F, section, ptr(front.key8), lo, K,
                                           (C.c_double * 3)(*front.origin), ptr(ws), ptr(d_sums), stream_ptr()))
        sums = d_sums.cpu().numpy().reshape(F, K, -1)
    else:
        sums = np.zeros((F, K, _capi.WF_FOCUS_M))
    spheres = sphere_table(sums, front.origin, sphere, ref, focus, radius)
    mom, counts, normal, pupil, _ = launch(rays, front.flat, F, lo, span, gaps, section, front.key8, K, spheres, n_zernike,
                                           pupil_radius)
    return WavefrontField(mom[:, keep], counts[:, keep], normal[:, keep], pupil, spheres[:, keep], n_zernike, front.reference_band,
                          reference_field, section, sources, field, sphere, pupil_radius, front.edges, **kwargs)
