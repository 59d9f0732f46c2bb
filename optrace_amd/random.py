"""Sampling helpers: mirror of optrace/tracer/random.py (stratified_interval_sampling, stratified_rectangle_sampling,
stratified_ring_sampling, inverse_transform_sampling) and of color.random_wavelengths_from_srgb (srgb.py:513-553), on the
device.

These are the samplers of the ray generator (csrc/ot_generate.hpp) behind entry points of their own
(include/optrace_amd.h, `ot_sample_*`): the N samples of a call are cut into the stratification ranges `RayStorage` cuts the
rays of a source into (`ray_storage.stratification_blocks`), so a sample drawn here is the one the generator draws for the
ray with the same seed and index.  Differences to the reference: the strata are assigned by a keyed
permutation instead of a shuffle; a power-of-two count fills a full jittered grid in the 2-D samplers; and every function
takes two more keywords:

    seed    None: drawn from NumPy's global generator (as `RayStorage.generate` does); else the call repeats with the seed.
    device  False: float64 NumPy arrays; True: float64 torch tensors on the current device, without a host copy.  A device
            tensor given as `S` or `rgb` gives a device tensor as well.

N = 0 returns empty arrays; anything else needs a device and raises `BackendError` without one (no NumPy fallback).
"""
from __future__ import annotations

import ctypes as C

import numpy as np
import torch

from . import _capi
from ._device import require_device, stream_ptr, ptr
from .options import global_options as go
from .ray_storage import stratification_blocks

_WL_MIN0, _WL_MAX0 = 380., 780.  # color/tools.py:9-10


def _seed(seed) -> int:
    return int(np.random.randint(0, 2**31 - 1)) if seed is None else int(seed)


def _ranges(N: int, cut: bool = True):
    """ot_source_range records of N samples: the generator's blocks, or one uncut range."""
    blocks = stratification_blocks(0, int(N), 64) if cut else [(0, int(N))]
    rng = (_capi.SourceRange * len(blocks))()
    for r, (first, count) in zip(rng, blocks):
        r.source, r.first, r.count, r.ray_power = 0, first, count, 0.
    return rng


def _empty(device: bool, k: int = 1):
    if device:
        out = tuple(torch.empty(0, dtype=torch.float64, device=require_device()) for _ in range(k))
    else:
        out = tuple(np.array([], dtype=np.float64) for _ in range(k))
    return out if k > 1 else out[0]


def _result(t: torch.Tensor, device: bool):
    return t if device else t.cpu().numpy()


def _stratified(kind: int, flag: bool, bounds: list, N: int, seed, device: bool, cut: bool = True):
    N, two = int(N), kind != _capi.SAMPLE_INTERVAL
    if not N:
        return _empty(device, 2 if two else 1)
    lib = _capi.load_library()
    b = (C.c_double * 4)(*[float(v) for v in bounds], *([0.] * (4 - len(bounds))))
    rng = _ranges(N, cut)
    dev = require_device()
    out = torch.empty((2 if two else 1, N), dtype=torch.float64, device=dev)
    _capi.check(lib.ot_sample_stratified(kind, int(flag), b, rng, len(rng), _seed(seed), N, ptr(out[0]),
                                         ptr(out[1]) if two else None, stream_ptr()))
    return (_result(out[0], device), _result(out[1], device)) if two else _result(out[0], device)


def stratified_interval_sampling(a: float, b: float, N: int, shuffle: bool = True, *, seed: int = None, device: bool = False):
    """N values in [a, b], one per stratum of width (b - a) / N (random.py:48-67).  `shuffle=False`: ascending -- one
    uncut range with stratum i for sample i; otherwise the order is that of the generator's keyed permutation."""
    return _stratified(_capi.SAMPLE_INTERVAL, bool(shuffle), [a, b], N, seed, device, cut=bool(shuffle))


def stratified_rectangle_sampling(a: float, b: float, c: float, d: float, N: int, *, seed: int = None, device: bool = False):
    """(x, y) with N values each inside [a, b] x [c, d]: a jittered grid of floor(sqrt(N))^2 cells and N - floor(sqrt(N))^2
    uniform samples (random.py:8-45); a power-of-two block of samples fills a full grid instead."""
    return _stratified(_capi.SAMPLE_RECTANGLE, False, [a, b, c, d], N, seed, device)


def stratified_ring_sampling(ri: float, r: float, N: int, polar: bool = False, *, seed: int = None, device: bool = False):
    """(x, y), or (r, phi) with `polar`, of N positions uniform over the annulus ri <= r' <= r (ri = 0: a disc), by the
    equal-area map of the stratified square (random.py:70-110)."""
    return _stratified(_capi.SAMPLE_RING, bool(polar), [ri, r], N, seed, device)


def inverse_transform_sampling(x: np.ndarray, f: np.ndarray, S, kind: str = "continuous", *, seed: int = None,
                               device: bool = False):
    """Values distributed like the pdf f(x) (not necessarily normalised), random.py:113-159.  `S`: a number of samples,
    stratified, or an array of samples in [0, 1]; kind "continuous" (linear between the nodes) or "discrete"."""
    x, f = np.ascontiguousarray(x, dtype=np.float64).ravel(), np.ascontiguousarray(f, dtype=np.float64).ravel()
    if not f.sum():
        raise RuntimeError("Cumulated probability is zero.")
    elif f.min() < 0:
        raise RuntimeError("Got negative value in pdf.")
    given = isinstance(S, (np.ndarray, torch.Tensor))
    device = device or isinstance(S, torch.Tensor)
    shape = tuple(S.shape) if given else (int(S),)
    n = int(np.prod(shape))
    if not n:
        return _empty(device).reshape(shape)
    lib = _capi.load_library()
    k = _capi.SAMPLE_DISCRETE if kind == "discrete" else _capi.SAMPLE_CONTINUOUS
    xp, fp = x.ctypes.data_as(C.POINTER(C.c_double)), f.ctypes.data_as(C.POINTER(C.c_double))
    rng = None if given else _ranges(n)
    dev = require_device()
    Sd = None
    if isinstance(S, torch.Tensor):
        Sd = S.to(dev, torch.float64).contiguous()
    elif given:
        Sd = torch.from_numpy(np.ascontiguousarray(S, dtype=np.float64)).to(dev)
    out = torch.empty(shape, dtype=torch.float64, device=dev)
    _capi.check(lib.ot_sample_inverse(k, xp, fp, x.shape[0], ptr(Sd), n, rng, 0 if given else len(rng), _seed(seed),
                                      ptr(out), stream_ptr()))
    return _result(out, device)


def random_wavelengths_from_srgb(rgb, *, seed: int = None, device: bool = False):
    """One random wavelength in nm for every sRGB colour of `rgb` (N, 3), drawn from the mix of the three primaries'
    spectra that has this colour (srgb.py:513-553).  Black rows take the blue primary, as in the reference."""
    if _WL_MIN0 < go.wavelength_range[0] or _WL_MAX0 > go.wavelength_range[1]:
        raise RuntimeError(f"Wavelength range {go.wavelength_range} does not include range "
                           f"[{_WL_MIN0}, {_WL_MAX0}] needed for this feature.")
    on_device = isinstance(rgb, torch.Tensor)
    device = device or on_device
    if not on_device:
        rgb = np.ascontiguousarray(rgb, dtype=np.float64)
    if rgb.ndim != 2 or rgb.shape[1] != 3:
        raise ValueError("expected colours of shape (N, 3)")
    n = int(rgb.shape[0])
    if not n:
        return _empty(device)
    lib = _capi.load_library()
    rng = _ranges(n)
    dev = require_device()
    src = rgb.to(dev, torch.float64).contiguous() if on_device else torch.from_numpy(rgb).to(dev)
    out = torch.empty(n, dtype=torch.float64, device=dev)
    _capi.check(lib.ot_sample_srgb_wavelengths(ptr(src), n, rng, len(rng), _seed(seed), ptr(out), stream_ptr()))
    return _result(out, device)


def shape_positions(fields: dict, N: int, seed=None) -> np.ndarray:
    """`random_positions` of the source shapes (geometry/surfaces.py): (N, 3) float64 in Fortran order, the start positions
    the generator gives the N rays of a source with this shape.  `fields`: the shape fields of an `ot_source`."""
    N = int(N)
    if not N:
        return np.zeros((0, 3), dtype=np.float64, order="F")
    lib = _capi.load_library()
    s = _capi.Source()
    for key, val in fields.items():
        if isinstance(val, list):
            getattr(s, key)[:] = val
        else:
            setattr(s, key, val)
    rng = _ranges(N)
    dev = require_device()
    out = torch.empty((3, N), dtype=torch.float64, device=dev)
    _capi.check(lib.ot_sample_positions(C.byref(s), rng, len(rng), _seed(seed), N, ptr(out), stream_ptr()))
    return out.cpu().numpy().T
