"""Huygens PSF across the field: per field point (the rays of one source) the polychromatic through-focus diffraction image about
a reference sphere of the field's own, and its transfer function along the field's tangential and sagittal directions, summed on
the device in one call for all fields, bands and planes.

`Raytracer.huygens_field` has no counterpart in optrace.  Definition: DESIGN.md, "Huygens PSF across the field".  Kernels:
csrc/ot_psf_field.hpp behind `ot_psf_field_*`; fields, used rays, bands and the reference band are those of the field analysis
(`field.band_records`), the sphere of a field and the paths to it those of `wavefront_field(sphere="field")`
(`wavefront_field.sphere_table`, `ot_wavefield_paths`, `ot_wavefield_moments`), a ray's arithmetic at the image points that of
`huygens_stack` (psf.py).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from . import field as _field
from . import mtf as _mtf
from . import psf as _psf
from . import wavefront_field as _wavefront_field
from .base import BaseClass, check_type, check_not_below, check_not_above
from .image import GrayscaleImage

N_FREQ = 17  # frequencies of the default list, equal steps from 0 to the sampling limit


def sampling_limit(n_px: int, size: float) -> float:
    """n_px / (2 size): the largest frequency in cycles / mm that pixels of size / n_px carry."""
    return n_px / (2 * size)


def check_frequencies(frequencies, n_px: int, size: float) -> None:
    """ValueError for a frequency above the sampling limit."""
    limit = sampling_limit(n_px, size)
    if np.any(frequencies > limit):
        raise ValueError(f"Property 'frequencies' needs to lie in 0 .. {limit} cycles / mm, the sampling limit n_px / (2 size), but "
                         f"holds {frequencies.max()}.")


def check_arguments(nt: int, n_fields: int, section, n_px, size, dz, focus, radius, frequencies):
    """Argument checks of `Raytracer.huygens_field` beyond `field.check_arguments`, host only; nt: sections per ray of the geometry,
    n_fields: the chosen sources.  -> (size as a float or None, dz as a float64 array (Z,), focus (F, 3) or None, radius (F,) or
    None, frequencies as a float64 array or None)."""
    _, _, size, dz, _ = _psf.check_stack_arguments(nt, section, None, None, n_px, size, dz, "lines")
    focus, radius, _ = _wavefront_field.check_arguments(n_fields, 1, "field", focus, radius, None)
    frequencies, _ = _mtf.check_arguments(frequencies, None)
    if frequencies is not None and size is not None:
        check_frequencies(frequencies, n_px, size)
    return size, dz, focus, radius, frequencies


def check_cap(n: int, F: int, K: int, n_px: int, Z: int) -> None:
    """The limits of `ot_psf_field_sum` on workspace plus field and on the chunks of a launch, said before anything of that size is
    asked of the device."""
    if _capi.psf_field_ws(n, F, K, n_px, Z) + F * Z * K * 2 * n_px * n_px > _capi.PSF_STACK_CAP:
        raise RuntimeError(f"{F} fields x {Z} planes x {K} bands x {n_px}^2 image points need more than {_capi.PSF_STACK_CAP} doubles "
                           "on the device: ask for fewer fields, planes, bands or image points per call.")
    if _capi.psf_field_chunks(n, F, K, n_px, Z) > _capi.PSFF_MAX_CHUNKS:
        raise RuntimeError(f"{n} rays of {F} fields need more than {_capi.PSFF_MAX_CHUNKS} chunks of records in one launch: ask for "
                           "fewer fields or trace fewer rays per call.")


def transfer(intensity, noise_floor: float, size: float, t, frequencies):
    """Step 4 of the definition in NumPy float64, in the order of the device (csrc/ot_psf_field.hpp, psf_field_otf_kernel) up to
    the sine and cosine, which here are NumPy's: intensity (n_px, n_px), t (2) -> (otf_t, otf_s complex (M,), mtf_t, mtf_s (M,)).
    Thread l of 256 adds the pixels l, l + 256, ...; the lanes of a wave fold 32, 16, .. 1 apart; the four waves add in order."""
    I = np.asarray(intensity, dtype=np.float64)
    n_px = I.shape[0]
    nu = np.asarray(frequencies, dtype=np.float64).reshape(-1)
    p = np.arange(n_px * n_px)
    step, half = size / float(n_px), 0.5 * float(n_px)
    x, y = ((p % n_px).astype(np.float64) + 0.5 - half) * step, ((p // n_px).astype(np.float64) + 0.5 - half) * step
    J = I.reshape(-1) - noise_floor
    tx, ty = float(t[0]), float(t[1])

    def fold(v):
        """(px, ...) terms -> their sum in the device's order"""
        lanes = np.zeros((256,) + v.shape[1:], dtype=v.dtype)
        for k in range(0, v.shape[0], 256):
            part = v[k:k + 256]
            lanes[:part.shape[0]] = lanes[:part.shape[0]] + part
        w = lanes.reshape((4, 64) + v.shape[1:])
        for o in (32, 16, 8, 4, 2, 1):  # (the lanes above 64 - o add what the shuffle hands them, and nothing reads them after)
            w = w.copy()
            w[:, :64 - o] = w[:, :64 - o] + w[:, o:]
        w = w[:, 0]
        return ((w[0] + w[1]) + w[2]) + w[3]

    def along(u):
        ph = nu[None, :] * u[:, None]
        r = 2.0 * (ph - np.rint(ph))
        return fold(J[:, None] * np.cos(np.pi * r)) - 1j * fold(J[:, None] * np.sin(np.pi * r))

    otf_t, otf_s = along(tx * x + ty * y), along(tx * y - ty * x)
    j0 = abs(fold(J))
    with np.errstate(invalid="ignore", divide="ignore"):
        return otf_t, otf_s, np.sqrt(otf_t.real ** 2 + otf_t.imag ** 2) / j0, np.sqrt(otf_s.real ** 2 + otf_s.imag ** 2) / j0


class HuygensField(BaseClass):
    """Result of `Raytracer.huygens_field`: the Huygens PSF of every field point, through focus; lengths in mm, wavelengths in nm,
    frequencies in cycles / mm.  F field points, K bands of wavelengths, Z planes, M frequencies.

    sources (F), field (F, 2), t (F, 2), section, reference_band, reference_field, band_edges (K + 1) or None for bands="lines":
    as in `FieldAnalysis`; wavelengths (K): power-weighted mean per band over all fields.  dz (Z): the planes of field f lie at
    focus[f] z + dz.  size: side of every tile of n_px x n_px image points about its field's focus.  focus (F, 3), radius (F):
    centre and signed radius of a field's reference sphere, for all its bands, NaN where it has none.
    band_N, band_power (F, K): rays of a cell in the sum and their power; n_missed: used rays whose line misses the sphere;
    n_no_sphere: used rays of a field without a sphere (a collimated field: pass `focus` and `radius`), which enter nothing else.
    band_weight (F, K): W kappa_mean^2 over its sum within the field; cutoff (F, K): 2 rho kappa_mean, the frequency beyond which
    a band transfers nothing, rho the field's pupil radius in units of |radius|.
    intensity (F, Z, n_px, n_px), band_strehl (F, Z, K), strehl (F, Z), noise_floor (F): per field as in `HuygensStack`; peak
    (F, Z); best_focus (F): dz of the first largest strehl.  frequencies (M); otf_t, otf_s (F, Z, M) complex: the Fourier
    transform of intensity - noise_floor along t and along s = (-t_y, t_x) about the focus; mtf_t, mtf_s: its modulus over that
    at frequency 0.
    A field without a usable ray has band_N = band_power = 0 and NaN elsewhere."""

    _tracked = False

    def __init__(self, sources, field, section: int, reference_band: int, reference_field: int, band_edges, wavelengths, dz,
                 size: float, focus, radius, band_N, band_power, n_missed, n_no_sphere, band_weight, cutoff, intensity, band_strehl,
                 strehl, noise_floor, frequencies, otf_t, otf_s, mtf_t, mtf_s, **kwargs) -> None:
        super().__init__(**kwargs)
        self.sources = np.array(sources, dtype=np.int64).reshape(-1)
        F = self.sources.shape[0]
        if not 1 <= F <= _capi.FIELD_MAX_FIELDS:
            raise ValueError(f"1 to {_capi.FIELD_MAX_FIELDS} fields, but there are {F}.")
        self.field = np.array(field, dtype=np.float64).reshape(F, 2)
        self.t = _field.directions(self.field)
        self.dz = np.array(dz, dtype=np.float64).reshape(-1)
        Z = self.dz.shape[0]
        self.band_N = np.array(band_N, dtype=np.int64).reshape(F, -1)
        K = self.band_N.shape[1]
        if not 1 <= K <= _capi.PSF_MAX_BANDS:
            raise ValueError(f"1 to {_capi.PSF_MAX_BANDS} bands, but there are {K}.")
        self.band_edges = None if band_edges is None else np.array(band_edges, dtype=np.float64).reshape(-1)
        if self.band_edges is not None and self.band_edges.shape[0] != K + 1:
            raise ValueError(f"{K} bands need {K + 1} edges, but there are {self.band_edges.shape[0]}.")
        check_type("reference_band", reference_band, (int, np.integer))
        check_type("reference_field", reference_field, (int, np.integer))
        if not -1 <= reference_band < K:
            raise ValueError(f"Reference band {reference_band} out of range for {K} bands.")
        if not 0 <= reference_field < F:
            raise ValueError(f"Reference field {reference_field} out of range for {F} fields.")
        self.n_fields, self.n_bands, self.section = F, K, int(section)
        self.reference_band, self.reference_field = int(reference_band), int(reference_field)
        self.wavelengths = np.array(wavelengths, dtype=np.float64).reshape(K)
        self.size = float(size)
        self.focus = np.array(focus, dtype=np.float64).reshape(F, 3)
        self.radius = np.array(radius, dtype=np.float64).reshape(F)
        self.band_power = np.array(band_power, dtype=np.float64).reshape(F, K)
        self.n_missed = np.array(n_missed, dtype=np.int64).reshape(F, K)
        self.n_no_sphere = np.array(n_no_sphere, dtype=np.int64).reshape(F, K)
        self.band_weight = np.array(band_weight, dtype=np.float64).reshape(F, K)
        self.cutoff = np.array(cutoff, dtype=np.float64).reshape(F, K)
        self.intensity = np.array(intensity, dtype=np.float64)
        if self.intensity.ndim != 4 or self.intensity.shape[:2] != (F, Z) or self.intensity.shape[2] != self.intensity.shape[3]:
            raise ValueError(f"intensity needs the shape ({F}, {Z}, n_px, n_px), but has {self.intensity.shape}.")
        self.n_px = self.intensity.shape[2]
        self.band_strehl = np.array(band_strehl, dtype=np.float64).reshape(F, Z, K)
        self.strehl = np.array(strehl, dtype=np.float64).reshape(F, Z)
        self.noise_floor = np.array(noise_floor, dtype=np.float64).reshape(F)
        self.frequencies = np.array(frequencies, dtype=np.float64).reshape(-1)
        M = self.frequencies.shape[0]
        self.otf_t, self.otf_s = (np.array(a, dtype=np.complex128).reshape(F, Z, M) for a in (otf_t, otf_s))
        self.mtf_t, self.mtf_s = (np.array(a, dtype=np.float64).reshape(F, Z, M) for a in (mtf_t, mtf_s))
        some = self.band_N.sum(axis=1) > 0
        self.peak = np.full((F, Z), np.nan)
        self.best_focus = np.full(F, np.nan)
        for f in np.nonzero(some)[0]:
            self.peak[f] = self.intensity[f].max(axis=(1, 2))
            if not np.all(np.isnan(self.strehl[f])):
                self.best_focus[f] = self.dz[int(np.nanargmax(self.strehl[f]))]  # (of equal values the first; NaN planes passed over)
        self.lock()

    def _index(self, name: str, val, n: int) -> int:
        check_type(name, val, (int, np.integer))
        check_not_below(name, val, 0)
        check_not_above(name, val, n - 1)
        return int(val)

    def psf(self, field: int, plane: int = 0) -> _psf.HuygensPSF:
        """The image of field `field` (an index into `sources`) on plane `plane` as a `HuygensPSF`."""
        f, z = self._index("field", field, self.n_fields), self._index("plane", plane, self.dz.shape[0])
        N, P = int(self.band_N[f].sum()), float(self.band_power[f].sum())
        with np.errstate(invalid="ignore", divide="ignore"):
            wl = float((self.band_power[f] * self.wavelengths)[self.band_N[f] > 0].sum() / P) if N else np.nan
        return _psf.HuygensPSF(N, P, int(self.n_missed[f].sum()), self.section, self.focus[f], self.radius[f], wl, self.size,
                               self.dz[z], self.intensity[f, z], self.strehl[f, z], self.noise_floor[f], long_desc=self.long_desc)

    def to_image(self, field: int, plane: int = 0) -> GrayscaleImage:
        """`HuygensPSF.to_image` of field `field` on plane `plane`."""
        return self.psf(field, plane).to_image()

    def grid(self, plane: int = 0, shape=None) -> list:
        """The nested list [Gy][Gx] of `HuygensPSF` that `ot.convolve_field` takes, all on plane `plane`: one row in the order of
        `sources`, or, with shape = (Gy, Gx), Gy rows of Gx filled row by row, which must hold exactly the F fields."""
        F = self.n_fields
        if shape is None:
            shape = (1, F)
        else:
            check_type("shape", shape, (list, tuple, np.ndarray))
            shape = tuple(np.asarray(shape).tolist())
            if len(shape) != 2 or not all(isinstance(v, int) and v >= 1 for v in shape):
                raise ValueError(f"Property 'shape' needs to be (Gy, Gx), two numbers of 1 or above, but is {shape}.")
            if shape[0] * shape[1] != F:
                raise ValueError(f"A grid of {shape[0]} x {shape[1]} nodes does not hold the {F} fields of the analysis.")
        return [[self.psf(b * shape[1] + a, plane) for a in range(shape[1])] for b in range(shape[0])]

    def diffraction_limit(self, nu, field: int, band: int):
        """The MTF of an aberration-free circular pupil at the frequencies `nu` for (field, band), the curve to draw beside the
        measured one: (acos x - x sqrt(1 - x^2)) / (pi / 2) with x = nu / cutoff[field, band], 0 from the cutoff on."""
        f, b = self._index("field", field, self.n_fields), self._index("band", band, self.n_bands)
        nu = np.asarray(nu, dtype=np.float64)
        with np.errstate(invalid="ignore", divide="ignore"):
            x = nu / self.cutoff[f, b]
            inside = x < 1
            xi = np.where(inside, x, 0.0)
            return np.where(inside, (np.arccos(xi) - xi * np.sqrt(1 - xi * xi)) / (np.pi / 2), np.where(np.isnan(x), np.nan, 0.0))


def _empty(section: int, bands, n_px: int, size, dz, focus, radius, frequencies, reference_field: int, sources, field,
           n_missed=None, n_no_sphere=None, **kwargs) -> HuygensField:
    """(the rule of `psf._empty_stack`: what the caller fixed stays; bands given as edges keep them, else one band without a ray)"""
    nan, Z, F = np.nan, dz.shape[0], len(sources)
    edges = bands if isinstance(bands, np.ndarray) else None
    K = 1 if edges is None else edges.shape[0] - 1
    if frequencies is None:
        frequencies = np.full(N_FREQ, nan) if size is None else np.linspace(0.0, sampling_limit(n_px, size), N_FREQ)
    M = frequencies.shape[0]
    zero = np.zeros((F, K), dtype=np.int64)
    return HuygensField(sources, field, section, -1, reference_field, edges, np.full(K, nan), dz, nan if size is None else size,
                        np.full((F, 3), nan) if focus is None else focus, np.full(F, nan) if radius is None else radius, zero,
                        np.zeros((F, K)), zero if n_missed is None else n_missed, zero if n_no_sphere is None else n_no_sphere,
                        np.full((F, K), nan), np.full((F, K), nan), np.full((F, Z, n_px, n_px), nan), np.full((F, Z, K), nan),
                        np.full((F, Z), nan), np.full(F, nan), frequencies, *(np.full((F, Z, M), nan) for _ in range(4)), **kwargs)


def result_parts(F: int, K: int, Z: int, n_px: int, M: int):
    """doubles of intensity | band_strehl | strehl | g | noise_floor | sums | otf | counts (int64) in the result buffer"""
    return [F * Z * n_px * n_px, F * Z * K, F * Z, F * K, F, F * Z * K * 5, F * Z * M * 6, F * K * 2]


def default_size(moments, pupil, some) -> float:
    """The largest over the fields `some` of 10 lambda_f / rho_f, the rule of `psf.default_size` per field: lambda_f the field's
    power-weighted mean wavelength from its moments (F, K, 9), rho_f the pupil radius of its pupil record (F, 4)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        lam = moments[:, :, 5].sum(axis=1) / moments[:, :, 0].sum(axis=1) * 1e-6
        sizes = 10 * lam / pupil[:, 3]
    return float(sizes[some].max())


def call_sum(grouped, starts, radius, F: int, K: int, n_px: int, size: float, dz, field, sums) -> None:
    """`ot_psf_field_sum` on grouped records: starts (F K + 1,) and radius (F,) on the host, field and sums on the device."""
    import torch
    from ._device import ptr, stream_ptr
    lib = _capi.load_library()
    n, Z, cells = int(starts[-1]), dz.shape[0], F * K
    check_cap(n, F, K, n_px, Z)
    ws = torch.empty(max(1, _capi.psf_field_ws(n, F, K, n_px, Z)), dtype=torch.float64, device=grouped.device)
    table = torch.empty(_capi.psf_field_table(cells), dtype=torch.int64, device=grouped.device)
    _capi.check(lib.ot_psf_field_sum(n, ptr(grouped), F, K, (C.c_int64 * (cells + 1))(*starts.tolist()),
                                     (C.c_double * F)(*radius.tolist()), n_px, size, Z, (C.c_double * Z)(*dz.tolist()), ptr(table),
                                     ptr(ws), ptr(field), ptr(sums), stream_ptr()))


def analyse(rays, ranges, section: int, origin, bands, n_px: int, size, dz, focus, radius, frequencies, reference,
            reference_field: int, sources, field, **kwargs) -> HuygensField:
    """The images of the fields `ranges` [(first, count), ...] of the storage `rays` behind section `section`; origin: the point
    the device subtracts before it sums positions; the other arguments as the checks returned them.  Reads of the device: those of
    `field.band_records`, one for the focus sums unless focus and radius are both given, one for the cell starts (with the moments,
    which give the default size), one for everything else."""
    import torch
    from ._device import require_device, ptr, stream_ptr
    F, Z, px = len(ranges), dz.shape[0], n_px * n_px
    fixed = dict(n_px=n_px, dz=dz, focus=focus, radius=radius, frequencies=frequencies, reference_field=reference_field,
                 sources=sources, field=field)
    K_least = bands.shape[0] - 1 if isinstance(bands, np.ndarray) else 1  # (the bands of "lines" and of a count are known later)
    check_cap(sum(n for _, n in ranges), F, K_least, n_px, Z)
    front = _field.band_records(rays, ranges, section, origin, bands, reference)
    if front is None:
        return _empty(section, bands, size=size, **fixed, **kwargs)
    lib = _capi.load_library()
    dev = require_device()
    st = stream_ptr()
    K, lo, keep, flat = front.K, front.lo, front.keep, front.flat
    cells = F * K
    some = [(a, n) for a, n in ranges if n > 0]
    span = max(a + n for a, n in some) - lo
    gaps = sum(n for _, n in some) != span
    ref = front.reference_band + keep.start if front.reference_band >= 0 else -1  # among the bands of the launch
    M = N_FREQ if frequencies is None else frequencies.shape[0]
    check_cap(span, F, K, n_px, Z)

    # the sphere of every field: that of wavefront_field(sphere="field")
    if focus is None or radius is None:
        d_sums = torch.zeros(cells * _capi.WF_FOCUS_M, dtype=torch.float64, device=dev)
        ws = torch.empty(max(1, lib.ot_wavefield_workspace(flat, F, K, 1)), dtype=torch.float64, device=dev)
        _capi.check(lib.ot_wavefield_focus(C.byref(front.R), flat, F, section, ptr(front.key8), lo, K, (C.c_double * 3)(*front.origin),
                                           ptr(ws), ptr(d_sums), st))
        sums17 = d_sums.cpu().numpy().reshape(F, K, -1)
    else:
        sums17 = np.zeros((F, K, _capi.WF_FOCUS_M))
    spheres = _wavefront_field.sphere_table(sums17, front.origin, "field", ref, focus, radius)
    focus_f, radius_f = spheres[:, 0, :3].copy(), spheres[:, 0, 3].copy()

    # paths to the spheres and their moments, then the records against the mean path of every cell
    R = rays._rays_struct()
    rays._dev["n"]  # (the index plane is written when it is read: this fills it if the trace left it stale)
    wl = rays._dev["wl"][lo:lo + span]
    planes = torch.full((3 * span,), np.nan, dtype=torch.float64, device=dev) if gaps else torch.empty(3 * span, dtype=torch.float64, device=dev)
    u, v, opl = planes[:span], planes[span:2 * span], planes[2 * span:]
    w = torch.zeros(span, dtype=torch.float32, device=dev) if gaps else torch.empty(span, dtype=torch.float32, device=dev)
    parts = result_parts(F, K, Z, n_px, M)
    out = torch.zeros(sum(parts), dtype=torch.float64, device=dev)
    inten, bs, s, g, floor, sums, otf, counts = out.split(parts)
    mom = torch.zeros(cells * _capi.WFF_M + F * _capi.WFF_PUPIL_M, dtype=torch.float64, device=dev)
    pupil = mom[cells * _capi.WFF_M:]
    d_sph = torch.as_tensor(np.ascontiguousarray(spheres, dtype=np.float64).reshape(-1), device=dev)
    ws = torch.empty(max(1, lib.ot_wavefield_workspace(flat, F, K, 1)), dtype=torch.float64, device=dev)
    _capi.check(lib.ot_wavefield_paths(C.byref(R), flat, F, section, ptr(front.key8), lo, K, ptr(d_sph), ptr(u), ptr(v), ptr(opl), ptr(w),
                                       ptr(counts), st))
    _capi.check(lib.ot_wavefield_moments(flat, F, ptr(u), ptr(v), ptr(opl), ptr(w), ptr(wl), ptr(front.key8), lo, K, ptr(ws), ptr(mom),
                                         ptr(pupil), st))
    rec = torch.empty(_capi.PSF_REC * span, dtype=torch.float64, device=dev)
    _capi.check(lib.ot_psf_field_rays(C.byref(R), flat, F, section, ptr(front.key8), lo, span, K, ptr(d_sph), ptr(opl), ptr(mom),
                                      ptr(rec), st))

    # group by cell f K + b; the one read before the sum: the cell starts, and the moments behind them
    of_field = torch.full((span,), F, dtype=torch.int64, device=dev)
    for f, (a, n) in enumerate(ranges):
        if n > 0:
            of_field[a - lo:a - lo + n] = f
    live = rec[5 * span:] != 0  # (the plane of a)
    key = torch.where(live, of_field * K + front.key8.to(torch.int64), cells)
    grouped, starts, table, _ = _psf.group_records(rec, span, key, cells, mom)
    moments, pupil_h = table[:cells * _capi.WFF_M].reshape(F, K, -1), table[cells * _capi.WFF_M:].reshape(F, -1)
    band_N = np.diff(starts).reshape(F, K)
    has = band_N.sum(axis=1) > 0
    n = int(starts[-1])

    def host_counts(c):
        c = c.view(np.int64).reshape(F, K, 2)
        c = c[:, keep] if front.edges is not None or n else c.sum(axis=1, keepdims=True)
        return c[:, :, 0], c[:, :, 1]

    if not n:
        n_missed, n_no_sphere = host_counts(counts.cpu().numpy())
        fixed.update(focus=focus_f if focus is None else focus, radius=radius_f if radius is None else radius)
        return _empty(section, front.edges if front.edges is not None else "lines", size=size, n_missed=n_missed,
                      n_no_sphere=n_no_sphere, **fixed, **kwargs)
    if size is None:
        size = default_size(moments, pupil_h, has)
        if not (np.isfinite(size) and size > 0):
            raise RuntimeError("The used rays of a field meet its reference sphere in one place, which gives the image no scale: pass `size`.")
    if frequencies is None:
        frequencies = np.linspace(0.0, sampling_limit(n_px, size), N_FREQ)
    else:
        check_frequencies(frequencies, n_px, size)

    # the sum, the combine step per field and the transfer function; (a field without a sphere has no record: any radius serves)
    field_d = torch.empty(F * Z * K * 2 * px, dtype=torch.float64, device=dev)
    call_sum(grouped, starts, np.where(np.isfinite(radius_f), radius_f, 1.0), F, K, n_px, size, dz, field_d, sums)
    _capi.check(lib.ot_psf_field_combine(F, K, Z, n_px, ptr(field_d), ptr(sums), ptr(inten), ptr(bs), ptr(s), ptr(g), ptr(floor), st))
    t = _field.directions(field)
    _capi.check(lib.ot_psf_field_otf(F, Z, n_px, size, ptr(inten), ptr(floor), (C.c_double * (2 * F))(*t.reshape(-1).tolist()), M,
                                     (C.c_double * M)(*frequencies.tolist()), ptr(otf), st))
    h = out.cpu().numpy()
    inten, bs, s, g, floor, sums, otf, counts = np.split(h, np.cumsum(parts)[:-1])
    n_missed, n_no_sphere = host_counts(counts)
    sums = sums.reshape(F, Z, K, 5)[:, :, keep]
    otf = otf.reshape(F, Z, M, 6)
    nan = np.nan
    with np.errstate(invalid="ignore", divide="ignore"):
        W = sums[:, 0, :, 3]
        cutoff = np.where(W > 0, 2 * pupil_h[:, 3:4] * (sums[:, 0, :, 4] / W), nan)
        weight = np.where(has[:, None], g.reshape(F, K)[:, keep], nan)
        mk = moments[:, keep]
        wavelengths = np.where(band_N[:, keep].sum(axis=0) > 0, mk[:, :, 5].sum(axis=0) / mk[:, :, 0].sum(axis=0), nan)
    return HuygensField(sources, field, section, front.reference_band, reference_field, front.edges, wavelengths, dz, size, focus_f,
                        radius_f, band_N[:, keep], W, n_missed, n_no_sphere, weight, cutoff, inten.reshape(F, Z, n_px, n_px),
                        bs.reshape(F, Z, K)[:, :, keep], s.reshape(F, Z), floor, frequencies, otf[..., 0] + 1j * otf[..., 1],
                        otf[..., 2] + 1j * otf[..., 3], otf[..., 4], otf[..., 5], **kwargs)
