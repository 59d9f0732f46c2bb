#!/usr/bin/env python3
"""Golden vectors for aspheres with more than 12 coefficients, from the upstream NumPy reference (whose AsphericSurface has
no upper bound on the number of coefficients).  Like generate_golden.py this runs only where the reference is installed;
the .npz files are committed, the reference is not.
    python tests/golden/generate_golden_asph_long.py

Files
  leaf_surfaces_asph_long.npz   find_hit / normals / mask / values per surface of scenes_asph_long.surface_zoo_long:
                                the keys and the ray recipe of generate_golden.gen_leaf_surfaces (that function itself
                                runs, on this zoo), 1500 rays and 1500 points per surface
  trace_asphere_long.npz        scenes_asph_long.asphere_long_scene, 2500 rays, polarisation on: the recording of
                                generate_golden.gen_trace
  trace_asphere_long_nopol.npz  the same scene with no_pol=True, 1500 rays

Conditions checked here before anything is written (the parameters, not the thresholds, are what to change if one
fails): the reference's geometry checks pass on the scene (no collision; z ranges are the reference's own estimates);
at least half of the traced rays reach the detector; per surface at least a quarter of the rays hit and at least a tenth
miss.  The parameter sets of scenes_asph_long.py met all of them as first written (A = 1e-3 throughout)."""
from __future__ import annotations

import numpy as np

import generate_golden as gg  # (imports the reference, tests/scenes.py and the oracle loader)

import scenes_asph_long as sal

ot = gg.ot
HERE = gg.HERE

LEAF_FILE = "leaf_surfaces_asph_long.npz"
TRACE_CASES = {"asphere_long": (sal.asphere_long_scene, 2500, 700, {}),
               "asphere_long_nopol": (sal.asphere_long_scene, 1500, 701, dict(no_pol=True))}


def gen_leaf():
    """gen_leaf_surfaces(3) with the long zoo in place of surface_zoo3, its own file name (the seed is that zoo's): the recipe
    stays the one every other leaf fixture was made with, without a copy of it here."""
    captured = {}
    orig_zoo, orig_save = gg.scenes.surface_zoo3, np.savez_compressed
    gg.scenes.surface_zoo3 = sal.surface_zoo_long
    np.savez_compressed = lambda fname, **out: captured.update(out)
    try:
        gg.gen_leaf_surfaces(3)
    finally:
        gg.scenes.surface_zoo3, np.savez_compressed = orig_zoo, orig_save
    names = [str(n) for n in captured["names"]]
    assert names == sal.NAMES, names
    for name in names:
        hit = captured[f"{name}/is_hit"]
        n = hit.shape[0]
        ncoeff = captured[f"{name}/param/coeff"].shape[0]
        assert n == 1500 and ncoeff > 12, (name, n, ncoeff)
        assert hit.sum() >= n / 4, f"{name}: only {hit.sum()} of {n} rays hit"
        assert (~hit).sum() >= n / 10, f"{name}: only {(~hit).sum()} of {n} rays miss"
        print(f"  {name}: ncoeff={ncoeff} hits={hit.sum()} misses={(~hit).sum()} ill={captured[f'{name}/ill'].sum()} "
              f"mask={captured[f'{name}/mask'].sum()} z=[{float(captured[f'{name}/param/z_min']):.6g}, "
              f"{float(captured[f'{name}/param/z_max']):.6g}]")
    np.savez_compressed(HERE / LEAF_FILE, **captured)
    print(LEAF_FILE, len(captured))


def gen_traces():
    for name, (builder, N, seed, rt_args) in TRACE_CASES.items():
        gg.gen_trace(name, builder, N, seed=seed, **rt_args)  # (asserts `not RT.geometry_error`)
        g = np.load(HERE / f"trace_{name}.npz")
        reached = g["det0/None/w"].shape[0]
        assert 2 * reached >= N, f"{name}: only {reached} of {N} rays reach the detector"
        print(f"  {name}: {reached} of {N} rays reach the detector")


if __name__ == "__main__":
    gen_leaf()
    gen_traces()
