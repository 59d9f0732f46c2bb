"""Huygens point spread function: the diffraction image of a point, summed on the device from the optical paths of a traced
bundle to the reference sphere of the wavefront analysis.

`Raytracer.huygens_psf` has no counterpart in optrace.  Every used ray sends one spherical wavelet from its place on the sphere,
with the phase of its optical path, and the wavelets are added coherently at the points of an image plane around the focus.
Definition: DESIGN.md, "Huygens PSF".  Kernels: csrc/ot_psf.hpp behind `ot_psf_rays` and `ot_psf_sum`; the paths and their mean
come from `ot_wavefront_paths` and `ot_wavefront_moments` (wavefront.py).

`Raytracer.huygens_stack` (second half of this file) does the same for a source of several wavelengths on several planes: rays of
one band of wavelengths add coherently, bands add in intensity, behind `ot_psf_stack` and `ot_psf_combine`; `HuygensStack.mtf` is
the diffraction MTF.  Definition: DESIGN.md, "Polychromatic through-focus PSF".
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _capi
from . import wavefront as _wavefront
from ._warn import warning
from .base import BaseClass, check_type, check_not_below, check_not_above
from .image import GrayscaleImage, srgb_linear_to_srgb


def check_arguments(nt: int, section, focus, radius, n_px, size, dz):
    """Argument checks of `Raytracer.huygens_psf`, host only; nt: sections per ray of the geometry.
    -> (focus as a float64 array or None, radius, size as floats or None, dz as a float)."""
    check_type("n_px", n_px, int)
    check_not_below("n_px", n_px, 1)
    check_not_above("n_px", n_px, _capi.PSF_MAX_PX)
    if size is not None:
        size = _wavefront._finite_number("size", size, positive=True)
    dz = _wavefront._finite_number("dz", dz)
    focus, radius = _wavefront.check_sphere_arguments(nt, section, focus, radius)
    return focus, radius, size, dz


class HuygensPSF(BaseClass):
    """Result of `Raytracer.huygens_psf`; lengths in mm.

    N, power: rays used (weight > 0 in the section, met by the reference sphere) and their summed weight.  n_missed: rays alive in
    the section whose line does not meet the sphere.  section, focus (3), radius: as for `WavefrontAnalysis`.  wavelength:
    power-weighted mean, nm.  size, dz: side length of the square of image points about the focus and its distance from the
    focus along z.  intensity: (n_px, n_px), row index y, column index x, |U|^2 / (sum a)^2 with a = sqrt(weight): 1 at the focus
    of a perfect wave.  strehl: the same figure exactly on the axis, at focus + (0, 0, dz), where with an even n_px no pixel
    centre lies.  noise_floor: sum a^2 / (sum a)^2, the background that a sum over randomly placed rays carries everywhere
    (1 / N for equal weights): the reason to trace many rays.  peak: largest value of `intensity`.  Without a usable ray
    N = power = 0, `intensity` is all NaN and every other figure NaN."""

    _tracked = False

    def __init__(self, N: int, power: float, n_missed: int, section: int, focus, radius: float, wavelength: float, size: float,
                 dz: float, intensity, strehl: float, noise_floor: float, **kwargs) -> None:
        super().__init__(**kwargs)
        self.N = int(N)
        self.power = float(power)
        self.n_missed = int(n_missed)
        self.section = int(section)
        self.focus = np.array(focus, dtype=np.float64)
        self.radius = float(radius)
        self.wavelength = float(wavelength)
        self.size = float(size)
        self.dz = float(dz)
        self.intensity = np.array(intensity, dtype=np.float64)
        self.strehl = float(strehl)
        self.noise_floor = float(noise_floor)
        self.peak = float(self.intensity.max()) if self.N else np.nan
        self.lock()

    def to_image(self) -> GrayscaleImage:
        """`intensity / peak` as a grayscale image with side lengths [size, size], which `convolve` takes as its `psf`.  The
        values of a `GrayscaleImage` carry the sRGB gamma, as those of the preset PSFs do: `convolve` removes it and works on the
        intensity itself."""
        if not self.peak > 0:
            raise RuntimeError("No usable ray: there is no image of this point spread function.")
        return GrayscaleImage(srgb_linear_to_srgb(self.intensity / self.peak), s=[self.size, self.size], quantity="Intensity",
                              long_desc=self.long_desc)


def _empty(section: int, focus, radius, n_px: int, size, dz: float, n_missed: int = 0, **kwargs) -> HuygensPSF:
    """(the rule of `wavefront._empty`: what the caller fixed stays)"""
    nan = np.nan
    return HuygensPSF(0, 0.0, n_missed, section, np.full(3, nan) if focus is None else focus, nan if radius is None else radius, nan,
                      nan if size is None else size, dz, np.full((n_px, n_px), nan), nan, nan, **kwargs)


def default_size(moments) -> float:
    """10 lambda_mean / pupil_radius from the moments record (float64): in air about 8 Airy diameters."""
    m = np.asarray(moments, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return float(10 * (m[5] / m[0] * 1e-6) / m[10])


def figures(field, centre):
    """(intensity (n_px, n_px), strehl, noise_floor) from what `ot_psf_sum` returns: field (2, n_px, n_px), centre (4)."""
    A2 = centre[2] * centre[2]
    return (field[0] ** 2 + field[1] ** 2) / A2, (centre[0] ** 2 + centre[1] ** 2) / A2, centre[3] / A2


def analyse(rays, first: int, count: int, section: int, origin, focus, radius, n_px: int, size, dz: float, **kwargs) -> HuygensPSF:
    """The point spread function of the rays [first, first + count) of the storage `rays` behind section `section`.  origin: a
    point near the section's start that the device subtracts before it sums positions; the other arguments as `check_arguments`
    returned them.  The host reads the focus sums (where focus or radius is left to it), the moments record (where size is) and,
    at the end, one buffer with everything else."""
    import torch
    from ._device import ptr, stream_ptr
    lib = _capi.load_library()
    parts = [2 * n_px * n_px, 4, 2]  # field | centre | wl range
    S = _wavefront.sphere_stage(rays, first, count, section, origin, focus, radius, sum(parts))
    focus, radius = S.focus, S.radius
    if S.empty:
        return _empty(section, focus, radius, n_px, size, dz, **kwargs)
    st = stream_ptr()
    field, centre, wl_range = S.extra.split(parts)
    # (for the warning alone: the range of the used rays' wavelengths)
    used = S.w > 0
    wl_range[0] = torch.where(used, S.wl, torch.inf).amin()
    wl_range[1] = torch.where(used, S.wl, -torch.inf).amax()
    if size is None:
        m = S.mom.cpu().numpy()
        if not m[0] > 0:
            return _empty(section, focus, radius, n_px, size, dz, int(S.missed.cpu()[0]), **kwargs)
        size = default_size(m)
        if not (np.isfinite(size) and size > 0):
            raise RuntimeError("The used rays meet the reference sphere in one place, which gives the image no scale: pass `size`.")
    rec = torch.empty(_capi.PSF_REC * count, dtype=torch.float64, device=S.w.device)
    _capi.check(lib.ot_psf_rays(C.byref(S.R), first, count, section, (C.c_double * 3)(*focus), radius, ptr(S.opl), ptr(S.mom),
                                ptr(rec), st))
    psf_ws = torch.empty(_capi.psf_ws(count, n_px), dtype=torch.float64, device=S.w.device)
    _capi.check(lib.ot_psf_sum(count, ptr(rec), radius, n_px, size, dz, ptr(psf_ws), ptr(field), ptr(centre), st))
    m, n_missed, h = S.read()
    W = m[0]
    if not W > 0:
        return _empty(section, focus, radius, n_px, size, dz, n_missed, **kwargs)
    field, centre, wl_range = np.split(h, np.cumsum(parts)[:-1])
    if wl_range[0] != wl_range[1]:
        warning(f"The used rays carry wavelengths from {wl_range[0]:.6g} nm to {wl_range[1]:.6g} nm and are added coherently, each "
                "with its own: the point spread function is meaningful for a monochromatic source only.")
    intensity, strehl, noise_floor = figures(field.reshape(2, n_px, n_px), centre)
    return HuygensPSF(int(m[1]), W, n_missed, section, focus, radius, m[5] / W, size, dz, intensity, strehl, noise_floor, **kwargs)


# ---- polychromatic, through focus: Raytracer.huygens_stack ---------------------------------------------------------------------------
def check_stack_arguments(nt: int, section, focus, radius, n_px, size, dz, bands):
    """Argument checks of `Raytracer.huygens_stack`, host only.  -> (focus, radius, size as `check_arguments` returns them, dz as a
    float64 array (Z,), bands as "lines", an int or a float64 array of edges)."""
    if isinstance(dz, (list, tuple, np.ndarray)):
        planes = np.asarray(dz)
        if planes.ndim != 1:
            raise ValueError(f"Property 'dz' needs to be a number or a 1-D sequence, but has shape {planes.shape}.")
        if not 1 <= planes.shape[0] <= _capi.PSF_MAX_PLANES:
            raise ValueError(f"Property 'dz' needs to hold 1 to {_capi.PSF_MAX_PLANES} planes, but holds {planes.shape[0]}.")
        planes = np.array([_wavefront._finite_number("dz", v) for v in planes.tolist()], dtype=np.float64)
    else:
        planes = np.array([_wavefront._finite_number("dz", dz)])
    focus, radius, size, _ = check_arguments(nt, section, focus, radius, n_px, size, 0.0)
    return focus, radius, size, planes, check_bands(bands)


def check_bands(bands):
    """The checks of `bands`, for `huygens_stack` and `chromatic_analysis`.  -> "lines", an int or a float64 array of edges."""
    if isinstance(bands, str):
        if bands != "lines":
            raise ValueError(f"Property 'bands' needs to be 'lines', a number of bands or a sequence of edges, but is '{bands}'.")
    elif isinstance(bands, (list, tuple, np.ndarray)):
        edges = np.asarray(bands)
        if edges.ndim != 1:
            raise ValueError(f"Property 'bands' needs to be a 1-D sequence of edges, but has shape {edges.shape}.")
        if not 2 <= edges.shape[0] <= _capi.PSF_MAX_BANDS + 1:
            raise ValueError(f"Property 'bands' needs to hold 2 to {_capi.PSF_MAX_BANDS + 1} edges, but holds {edges.shape[0]}.")
        bands = np.array([_wavefront._finite_number("bands", v) for v in edges.tolist()], dtype=np.float64)
        if not np.all(np.diff(bands) > 0):
            raise ValueError("Property 'bands' needs to hold strictly ascending edges.")
    else:
        check_type("bands", bands, int)
        check_not_below("bands", bands, 1)
        check_not_above("bands", bands, _capi.PSF_MAX_BANDS)
    return bands


class DiffractionMTF(BaseClass):
    """Result of `HuygensStack.mtf`: f (n_f,) in cycles / mm, mtf_x and mtf_y (n_f,), the modulus of the Fourier transform of the
    line spread over x and over y, 1 at f = 0."""

    _tracked = False

    def __init__(self, f, mtf_x, mtf_y, **kwargs) -> None:
        super().__init__(**kwargs)
        self.f = np.array(f, dtype=np.float64)
        self.mtf_x = np.array(mtf_x, dtype=np.float64)
        self.mtf_y = np.array(mtf_y, dtype=np.float64)
        self.lock()


def diffraction_mtf(intensity, noise_floor: float, size: float, n_f: int = 65, f_max: float = None, **kwargs) -> DiffractionMTF:
    """MTF of one plane of intensity (n_px, n_px) over a square of side `size` about the focus ("Polychromatic
    through-focus PSF"): J = intensity - noise_floor, not clamped; its column sums are the line spread over x, its row sums the
    one over y; OTF(f) = sum_c LSF[c] exp(-2 pi i f x_c) at the pixel centres x_c; MTF = |OTF(f)| / |OTF(0)|.  f_max: None for
    the sampling limit n_px / (2 size), beyond which a ValueError is raised."""
    check_type("n_f", n_f, int)
    check_not_below("n_f", n_f, 1)
    n_px = intensity.shape[0]
    limit = n_px / (2 * size)
    if f_max is None:
        f_max = limit
    else:
        f_max = _wavefront._finite_number("f_max", f_max)
        if f_max < 0 or f_max > limit:
            raise ValueError(f"Property 'f_max' needs to lie in 0 .. {limit} cycles / mm, the sampling limit n_px / (2 size), but is {f_max}.")
    f = np.linspace(0.0, f_max, n_f)
    x = (np.arange(n_px) + 0.5 - n_px / 2) * (size / n_px)
    J = intensity - noise_floor
    kernel = np.exp(-2j * np.pi * f[:, None] * x[None])
    otf_x, otf_y = kernel @ J.sum(axis=0), kernel @ J.sum(axis=1)
    with np.errstate(invalid="ignore", divide="ignore"):  # (f[0] = 0: the first entry is OTF(0))
        return DiffractionMTF(f, np.abs(otf_x) / np.abs(otf_x[0]), np.abs(otf_y) / np.abs(otf_y[0]), **kwargs)


class HuygensStack(BaseClass):
    """Result of `Raytracer.huygens_stack`: the Huygens PSF of a source of several wavelengths on several planes; lengths in mm.

    Rays of one band add coherently, bands add in intensity ("Polychromatic through-focus PSF").  N, power: rays in
    some band and their summed weight.  n_missed: as for `HuygensPSF`.  n_out_of_band: used rays whose wavelength lies in no
    band.  section, focus (3), radius, size: as for `HuygensPSF`.  dz (Z,): the planes, at focus z + dz[z].  band_edges (K + 1,)
    in nm, None for bands="lines"; band_N, band_power, band_wavelength (power-weighted mean, nm), band_weight (K,): the band
    weight is W kappa_mean^2 over its sum, the share of a band's Strehl-normalised image in the irradiance.  intensity
    (Z, n_px, n_px): sum_b weight_b |U_b|^2 / A_b^2, 1 at the focus when every band is a perfect wave focused there.
    band_strehl (Z, K): |U_b|^2 / A_b^2 exactly on the axis (NaN for a band without a ray); strehl (Z,): its weighted sum.
    noise_floor: sum_b weight_b W_b / A_b^2.  peak (Z,).  best_focus: dz of the first largest strehl.  Without a usable ray
    N = power = 0, the arrays are NaN and every figure NaN."""

    _tracked = False

    def __init__(self, N: int, power: float, n_missed: int, n_out_of_band: int, section: int, focus, radius: float, size: float, dz,
                 band_edges, band_N, band_power, band_wavelength, band_weight, intensity, strehl, band_strehl, noise_floor: float,
                 **kwargs) -> None:
        super().__init__(**kwargs)
        self.N = int(N)
        self.power = float(power)
        self.n_missed = int(n_missed)
        self.n_out_of_band = int(n_out_of_band)
        self.section = int(section)
        self.focus = np.array(focus, dtype=np.float64)
        self.radius = float(radius)
        self.size = float(size)
        self.dz = np.array(dz, dtype=np.float64)
        self.band_edges = None if band_edges is None else np.array(band_edges, dtype=np.float64)
        self.band_N = np.array(band_N, dtype=np.int64)
        self.band_power = np.array(band_power, dtype=np.float64)
        self.band_wavelength = np.array(band_wavelength, dtype=np.float64)
        self.band_weight = np.array(band_weight, dtype=np.float64)
        self.intensity = np.array(intensity, dtype=np.float64)
        self.strehl = np.array(strehl, dtype=np.float64)
        self.band_strehl = np.array(band_strehl, dtype=np.float64)
        self.noise_floor = float(noise_floor)
        self.peak = self.intensity.max(axis=(1, 2)) if self.N else np.full(self.dz.shape[0], np.nan)
        self.best_focus = float(self.dz[int(np.argmax(self.strehl))]) if self.N else np.nan
        self.lock()

    @property
    def wavelength(self) -> float:
        """Power-weighted mean wavelength of the rays in some band, nm."""
        return float((self.band_power * self.band_wavelength)[self.band_N > 0].sum() / self.power) if self.N else np.nan

    def psf(self, z: int = 0) -> HuygensPSF:
        """Plane z as a `HuygensPSF`."""
        z = self._plane(z)
        return HuygensPSF(self.N, self.power, self.n_missed, self.section, self.focus, self.radius, self.wavelength, self.size,
                          self.dz[z], self.intensity[z], self.strehl[z], self.noise_floor, long_desc=self.long_desc)

    def to_image(self, z: int = 0) -> GrayscaleImage:
        """`HuygensPSF.to_image` of plane z."""
        return self.psf(z).to_image()

    def mtf(self, z: int = 0, n_f: int = 65, f_max: float = None) -> DiffractionMTF:
        """Diffraction MTF of plane z along x and y at n_f frequencies from 0 to f_max (None: the sampling limit n_px / (2 size));
        host arithmetic on `intensity[z]`, see `diffraction_mtf`."""
        return diffraction_mtf(self.intensity[self._plane(z)], self.noise_floor, self.size, n_f, f_max, long_desc=self.long_desc)

    def _plane(self, z) -> int:
        check_type("z", z, int)
        check_not_below("z", z, 0)
        check_not_above("z", z, self.dz.shape[0] - 1)
        return z


def _empty_stack(section: int, focus, radius, n_px: int, size, dz, bands, n_missed: int = 0, n_out_of_band: int = 0,
                 **kwargs) -> HuygensStack:
    """(the rule of `_empty`: what the caller fixed stays; bands given as edges keep them, else one band without a ray)"""
    nan, Z = np.nan, dz.shape[0]
    edges = bands if isinstance(bands, np.ndarray) else None
    K = 1 if edges is None else edges.shape[0] - 1
    return HuygensStack(0, 0.0, n_missed, n_out_of_band, section, np.full(3, nan) if focus is None else focus,
                        nan if radius is None else radius, nan if size is None else size, dz, edges, np.zeros(K), np.zeros(K),
                        np.full(K, nan), np.full(K, nan), np.full((Z, n_px, n_px), nan), np.full(Z, nan), np.full((Z, K), nan), nan,
                        **kwargs)


def assign_bands(wl, live, bands):
    """Band index per ray, on the device of `wl`.  wl: float32 wavelengths; live: which rays take part at all; bands: as
    `check_stack_arguments` returns them.  -> (key int64, K for rays in no band; K as asked for; table float64: the K + 1 edges,
    or for "lines" the 32 smallest lines padded with inf behind one slot that holds the number of lines)

    A wavelength is compared as float64 with float64 edges: band b holds e[b] <= wl < e[b + 1], the last band its upper edge too.
    An int K means K equal bands over [min, max] of the live rays; with min == max every live ray lies on the last edge and so
    in band K - 1, which `group_records`' caller reads as the one band there is."""
    import torch
    w64 = wl.to(torch.float64)
    if isinstance(bands, str):
        lines = torch.unique(wl[live]).to(torch.float64)  # ascending
        K = _capi.PSF_MAX_BANDS
        n_lines = lines.shape[0]
        table = torch.full((K + 1,), torch.inf, dtype=torch.float64, device=wl.device)
        table[0] = n_lines
        table[1:1 + min(n_lines, K)] = lines[:K]
        key = torch.searchsorted(table[1:].contiguous(), w64).clamp(max=K)  # (a live ray's wavelength is a line: found exactly)
        return torch.where(live, key, K), K, table
    if isinstance(bands, np.ndarray):
        edges = torch.as_tensor(bands, device=wl.device)
    else:
        lo = torch.where(live, w64, torch.inf).amin()
        hi = torch.where(live, w64, -torch.inf).amax()
        edges = lo + (hi - lo) * (torch.arange(bands + 1, dtype=torch.float64, device=wl.device) / bands)
        edges[-1] = hi
    K = edges.shape[0] - 1
    key = torch.bucketize(w64, edges, right=True) - 1  # e[key] <= wl < e[key + 1]; -1 below all, K from the last edge on
    key = torch.where(w64 == edges[-1], K - 1, key)
    return torch.where(live & (key >= 0) & (key < K), key, K), K, edges


def group_records(rec, count: int, key, K: int, table):
    """Stable group-by of the record planes rec (6 * count) by `key`: band b in ascending ray order, rays with key K dropped.  One
    read of the device: the K + 1 starts and `table`.  -> (grouped (6 * n) device, starts (K + 1,) int64 host, table host, the
    n grouped rays' indices device)"""
    import torch
    order = torch.sort(key, stable=True).indices
    counts = torch.bincount(key, minlength=K + 1)[:K]
    head = torch.cat([torch.zeros(1, dtype=torch.float64, device=key.device), counts.cumsum(0).to(torch.float64), table]).cpu().numpy()
    starts = head[:K + 1].astype(np.int64)
    order = order[:int(starts[-1])]
    return rec.view(_capi.PSF_REC, count)[:, order].contiguous().view(-1), starts, head[K + 1:], order


def settle_bands(bands, K: int, starts, table):
    """What the host makes of the starts and the table of `assign_bands` once it has read them.  -> (K, starts, band_edges): for
    "lines" the number of lines found (one band where there is no ray) and no edges, for an int the edges, or one band from
    min to max where they are equal.  More than 32 lines: RuntimeError."""
    if isinstance(bands, str):
        if table[0] > K:
            raise RuntimeError(f"The used rays carry {int(table[0])} distinct wavelengths, more than the {K} that bands='lines' "
                               "takes: pass band edges or a number of bands.")
        K = max(int(table[0]), 1)
        return K, starts[:K + 1], None
    if starts[-1] and not isinstance(bands, np.ndarray) and table[0] == table[-1]:
        return 1, starts[[0, -1]], table[[0, -1]]
    return K, starts, table


def check_cap(n: int, K: int, n_px: int, Z: int) -> None:
    """The limit of `ot_psf_stack` on workspace plus field, said before anything of that size is asked of the device."""
    if _capi.psf_stack_ws(n, K, n_px, Z) + Z * K * 2 * n_px * n_px > _capi.PSF_STACK_CAP:
        raise RuntimeError(f"{Z} planes x {K} bands x {n_px}^2 image points need more than {_capi.PSF_STACK_CAP} doubles on the device: "
                           "ask for fewer planes, bands or image points per call.")


def call_stack(grouped, starts, radius: float, n_px: int, size: float, dz, out) -> None:
    """`ot_psf_stack` and `ot_psf_combine` on grouped records, the figures into the device buffer `out` of `stack_parts(K, Z, n_px)`
    doubles."""
    import torch
    from ._device import ptr, stream_ptr
    lib = _capi.load_library()
    K, Z, n, st = starts.shape[0] - 1, dz.shape[0], int(starts[-1]), stream_ptr()
    parts = stack_parts(K, Z, n_px)
    check_cap(n, K, n_px, Z)
    inten, bs, s, g, floor, sums = out[:sum(parts)].split(parts)
    ws = torch.empty(_capi.psf_stack_ws(n, K, n_px, Z), dtype=torch.float64, device=grouped.device)
    field = torch.empty(Z * K * 2 * n_px * n_px, dtype=torch.float64, device=grouped.device)
    _capi.check(lib.ot_psf_stack(n, ptr(grouped), K, (C.c_int64 * (K + 1))(*starts.tolist()), radius, n_px, size, Z,
                                 (C.c_double * Z)(*dz.tolist()), ptr(ws), ptr(field), ptr(sums), st))
    _capi.check(lib.ot_psf_combine(K, Z, n_px, ptr(field), ptr(sums), ptr(inten), ptr(bs), ptr(s), ptr(g), ptr(floor), st))


def stack_parts(K: int, Z: int, n_px: int):
    """doubles of intensity | band_strehl | strehl | g | noise_floor | sums in the result buffer of `call_stack`"""
    return [Z * n_px * n_px, Z * K, Z, K, 1, Z * K * 5]


def analyse_stack(rays, first: int, count: int, section: int, origin, focus, radius, n_px: int, size, dz, bands, **kwargs) -> HuygensStack:
    """`analyse` for bands of wavelengths and several planes; the arguments as `check_stack_arguments` returned them.  Besides the
    reads of `analyse` before the sum, the host reads the band starts; everything else comes in one buffer at the end."""
    import torch
    from ._device import ptr, stream_ptr
    lib = _capi.load_library()
    Z = dz.shape[0]
    K_max = _capi.PSF_MAX_BANDS if isinstance(bands, str) else bands.shape[0] - 1 if isinstance(bands, np.ndarray) else bands
    check_cap(count, 1 if isinstance(bands, str) else K_max, n_px, Z)  # (with "lines" the bands are known later: `call_stack`)
    S = _wavefront.sphere_stage(rays, first, count, section, origin, focus, radius, sum(stack_parts(K_max, Z, n_px)) + K_max)
    focus, radius = S.focus, S.radius
    if S.empty:
        return _empty_stack(section, focus, radius, n_px, size, dz, bands, **kwargs)
    if size is None:
        m = S.mom.cpu().numpy()
        if not m[0] > 0:
            return _empty_stack(section, focus, radius, n_px, size, dz, bands, int(S.missed.cpu()[0]), **kwargs)
        size = default_size(m)
        if not (np.isfinite(size) and size > 0):
            raise RuntimeError("The used rays meet the reference sphere in one place, which gives the image no scale: pass `size`.")
    rec = torch.empty(_capi.PSF_REC * count, dtype=torch.float64, device=S.w.device)
    _capi.check(lib.ot_psf_rays(C.byref(S.R), first, count, section, (C.c_double * 3)(*focus), radius, ptr(S.opl), ptr(S.mom),
                                ptr(rec), stream_ptr()))
    live = rec[5 * count:] != 0  # (the plane of a)
    key, K, table = assign_bands(S.wl, live, bands)
    n_live = live.sum().to(torch.float64).reshape(1)
    grouped, starts, table, order = group_records(rec, count, key, K, torch.cat([table, n_live]))
    table, n_live = table[:-1], int(table[-1])
    n = int(starts[-1])
    K, starts, edges = settle_bands(bands, K, starts, table)
    if not n:
        n_missed = S.read()[1]
        return _empty_stack(section, focus, radius, n_px, size, dz, bands, n_missed, n_live, **kwargs)
    parts = stack_parts(K, Z, n_px)
    call_stack(grouped, starts, radius, n_px, size, dz, S.extra)
    if edges is not None:  # power-weighted mean wavelength per band: sum a^2 wl over its rays, behind the figures in the result buffer
        a2wl = grouped[5 * n:] ** 2 * S.wl.to(torch.float64)[order]
        for b in range(K):
            S.extra[sum(parts) + b] = a2wl[starts[b]:starts[b + 1]].sum()
    _, n_missed, h = S.read()
    inten, bs, s, g, floor, sums, band_wl = np.split(h[:sum(parts) + K], np.cumsum(parts))
    sums = sums.reshape(Z, K, 5)
    W = sums[0, :, 3]
    with np.errstate(invalid="ignore", divide="ignore"):
        band_wl = table[1:K + 1] if edges is None else band_wl / W  # (a line is its own mean)
    return HuygensStack(n, W.sum(), n_missed, n_live - n, section, focus, radius, size, dz, edges, np.diff(starts), W, band_wl, g,
                        inten.reshape(Z, n_px, n_px), s, bs.reshape(Z, K), floor[0], **kwargs)
