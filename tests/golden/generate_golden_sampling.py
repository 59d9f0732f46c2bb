#!/usr/bin/env python3
"""tests/golden/sampling.npz: what the reference's sampling module (optrace/tracer/random.py) and
color.random_wavelengths_from_srgb give for the inputs of tests/sampling_cases.py.

Runs only where the reference is installed (imported through oracle/refload.py, its generators reseeded before every
draw); the .npz is committed, the reference is not.  Re-run with
    python tests/golden/generate_golden_sampling.py [output.npz]
The archive is written with fixed zip time stamps, so a second run reproduces the file byte for byte.

Keys
  inverse/discrete/x, /f, /S, /out        inverse_transform_sampling(x, f, S, kind="discrete"): deterministic with S given
  inverse/continuous/x, /f, /S, /out      the same, kind="continuous"
  srgb/edges                              41 wavelengths from 380 to 780 nm
  srgb/<colour>/rgb                       the colour; colours: sampling_cases.COLOURS
  srgb/<colour>/cdf                       the cumulative distribution of the colour's mixture of the three primaries at the
                                          edges: the primaries' cumulative trapezoids over wavelengths(5000), weighted as
                                          srgb.py:522-539 weights them, linear between the 5000 nodes
  srgb/<colour>/worst                     max over 8 seeds and the edges of |sampled cdf - cdf| for 65536 equal rows
  cells/ring/<N>                          max over 8 seeds of sampling_cases.ring_cell_deviation for stratified_ring_sampling
                                          (ri = 1, r = 3, N samples): 8 equal-area annuli x 8 sectors
  cells/rect/<N>                          the same for stratified_rectangle_sampling, 10 x 10 cells
  cells/rect/extra                        samples beyond one per cell of the 31 x 31 grid at N = 1000 (every cell is hit)
"""
from __future__ import annotations

import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from generate_golden_image_convert import ot, color, write_npz  # noqa: E402  (loads the reference)
import refload  # noqa: E402
import sampling_cases as sc  # noqa: E402
import optrace.tracer.random as rrandom  # noqa: E402
import optrace.tracer.color.srgb as rsrgb  # noqa: E402
import scipy.integrate  # noqa: E402


def mixture_cdf(rgb) -> np.ndarray:
    wl = color.wavelengths(5000)
    rgbl = color.srgb_to_srgb_linear(np.array([rgb], dtype=np.float64))[0]
    w = rgbl * np.array([rsrgb._SRGB_R_PRIMARY_POWER_FACTOR, 1.0, rsrgb._SRGB_B_PRIMARY_POWER_FACTOR])
    w = w / w.sum()
    cdf = np.zeros(sc.EDGES.shape[0])
    for wp, prim in zip(w, (color.srgb_r_primary, color.srgb_g_primary, color.srgb_b_primary)):
        F = scipy.integrate.cumulative_trapezoid(prim(wl), initial=0)
        cdf += wp * np.interp(sc.EDGES, wl, F / F[-1])
    return cdf


def main(path) -> None:
    out = {}
    for kind, case in (("discrete", sc.discrete_case), ("continuous", sc.continuous_case)):
        x, f, S = case()
        out[f"inverse/{kind}/x"], out[f"inverse/{kind}/f"], out[f"inverse/{kind}/S"] = x, f, S
        out[f"inverse/{kind}/out"] = np.asarray(rrandom.inverse_transform_sampling(x, f, S, kind=kind), dtype=np.float64)

    out["srgb/edges"] = sc.EDGES
    for name, rgb in sc.COLOURS.items():
        cdf = mixture_cdf(rgb)
        worst = 0.0
        for seed in sc.SEEDS:
            refload.reseed(ot, seed)
            wl = color.random_wavelengths_from_srgb(np.tile(np.array(rgb, dtype=np.float64), (sc.N_WL, 1)))
            worst = max(worst, float(np.abs(sc.sampled_cdf(wl) - cdf).max()))
        out[f"srgb/{name}/rgb"], out[f"srgb/{name}/cdf"], out[f"srgb/{name}/worst"] = np.array(rgb), cdf, np.float64(worst)
        print(f"srgb {name}: worst {worst:.3e} = {worst * sc.N_WL:.2f} / N")

    for N in sc.RING_N:
        worst = 0.0
        for seed in sc.SEEDS:
            refload.reseed(ot, seed)
            x, y = rrandom.stratified_ring_sampling(*sc.RING, N)
            worst = max(worst, sc.ring_cell_deviation(x, y, *sc.RING))
        out[f"cells/ring/{N}"] = np.float64(worst)
        print(f"ring N={N}: worst {worst:.4f}")
    worst, extra = 0.0, set()
    for seed in sc.SEEDS:
        refload.reseed(ot, seed)
        x, y = rrandom.stratified_rectangle_sampling(*sc.RECT, sc.RECT_N)
        worst = max(worst, sc.rect_cell_deviation(x, y, *sc.RECT))
        counts = sc.rect_cell_counts(x, y, *sc.RECT, 31, 31)
        assert counts.min() >= 1
        extra.add(int((counts - 1).sum()))
    assert extra == {39}, extra
    out[f"cells/rect/{sc.RECT_N}"] = np.float64(worst)
    out["cells/rect/extra"] = np.int64(39)
    print(f"rect N={sc.RECT_N}: worst {worst:.4f}")
    write_npz(path, out)


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE / "sampling.npz")
