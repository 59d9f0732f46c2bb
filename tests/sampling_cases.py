"""Inputs and figures shared by the fixture generator tests/golden/generate_golden_sampling.py (run on the reference) and
the sampler tests (tests/test_sampling_host.py, tests/test_gpu_sampling.py, run on ot.random): both sides bin and count with
the same code."""
from __future__ import annotations

import numpy as np

# ---- (a) inverse transform sampling with S given ----------------------------------------------------------------------


def discrete_case():
    """x, f, S: a pdf of 12 entries, three of them zero; S holds 0, 1, every cumulative value exactly and 500 random
    values."""
    rng = np.random.default_rng(20240611)
    x = np.array([405.5, 420.0, 433.25, 450.0, 486.1, 510.0, 546.07, 587.56, 610.0, 632.8, 656.27, 700.0])
    f = np.array([0.5, 0.0, 1.25, 2.0, 0.0, 0.75, 3.0, 0.125, 0.0, 1.5, 0.25, 1.0])
    F = np.cumsum(f[f > 0])
    S = np.concatenate(([0.0, 1.0], F / F[-1], rng.uniform(0, 1, 500)))
    return x, f, S


def continuous_case():
    """x, f, S: a pdf of 200 nodes with a stretch of zeros in it, 500 random S."""
    rng = np.random.default_rng(20240612)
    x = np.linspace(400.0, 700.0, 200)
    f = 1.0 + np.sin((x - 400.0) / 37.0) ** 2 + 0.3 * rng.uniform(0, 1, 200)
    f[80:110] = 0.0
    S = rng.uniform(0, 1, 500)
    return x, f, S


# ---- (b) wavelengths of sRGB colours ------------------------------------------------------------------------------------
COLOURS = {"red": (1.0, 0.0, 0.0), "green": (0.0, 1.0, 0.0), "blue": (0.0, 0.0, 1.0), "white": (1.0, 1.0, 1.0),
           "sky": (0.2, 0.5, 0.9), "amber": (0.9, 0.6, 0.1)}
EDGES = np.linspace(380.0, 780.0, 41)
N_WL = 65536
SEEDS = range(8)


def sampled_cdf(wl: np.ndarray, edges: np.ndarray = EDGES) -> np.ndarray:
    """Share of the samples at or below each edge."""
    return np.searchsorted(np.sort(wl), edges, side="right") / wl.shape[0]


# ---- (c) equal-area cell counts -----------------------------------------------------------------------------------------
RING = (1.0, 3.0)       # ri, r
RING_N = (1000, 4096)
RECT = (-2.0, 3.0, 1.0, 2.5)  # a, b, c, d
RECT_N = 1000


def ring_cell_deviation(x, y, ri: float, r: float, n_annuli: int = 8, n_sectors: int = 8) -> float:
    """max |count - mean| / mean over n_annuli equal-area annuli x n_sectors sectors of the ring ri .. r."""
    rr = x * x + y * y
    ia = np.clip((n_annuli * (rr - ri * ri) / (r * r - ri * ri)).astype(int), 0, n_annuli - 1)
    js = np.clip((n_sectors * (np.arctan2(y, x) + np.pi) / (2 * np.pi)).astype(int), 0, n_sectors - 1)
    counts = np.bincount(ia * n_sectors + js, minlength=n_annuli * n_sectors)
    mean = x.shape[0] / (n_annuli * n_sectors)
    return float(np.abs(counts - mean).max() / mean)


def rect_cell_counts(x, y, a: float, b: float, c: float, d: float, nx: int, ny: int) -> np.ndarray:
    """(ny, nx) counts of the samples in the cells of an nx x ny grid over [a, b] x [c, d]."""
    ix = np.clip((nx * (x - a) / (b - a)).astype(int), 0, nx - 1)
    iy = np.clip((ny * (y - c) / (d - c)).astype(int), 0, ny - 1)
    return np.bincount(iy * nx + ix, minlength=nx * ny).reshape(ny, nx)


def rect_cell_deviation(x, y, a: float, b: float, c: float, d: float, n: int = 10) -> float:
    counts = rect_cell_counts(x, y, a, b, c, d, n, n)
    mean = x.shape[0] / (n * n)
    return float(np.abs(counts - mean).max() / mean)
