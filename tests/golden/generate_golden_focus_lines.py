#!/usr/bin/env python3
"""tests/golden/focus_lines.npz: what the reference's focus-search cost function and direct RMS solution
(optrace/tracer/raytracer.py, Raytracer.__focus_search_cost_function and __focus_rms_spot_direct_solution) give for the
dyadic hit lines of tests/focus_cases.py.

Runs only where the reference is installed (imported through oracle/refload.py); the .npz is committed, the reference is
not.  Re-run with
    python tests/golden/generate_golden_focus_lines.py [output.npz]
The archive is written with fixed zip time stamps, so a second run reproduces the file byte for byte.

Keys, per case of focus_cases.FIXTURE_CASES (n = 2 with both weights > 0, n = 2 with one weight 0, 65, 1025, 5000, a fan
of 1025 lines in the plane y = 0)
  <case>/pa, /sb (n, 2) f64, /w (n,) f32   the lines as focus_cases.lines returns them, w = -1: left out
  <case>/z (3,)                            the sample positions 0, 3.125, 16
  <case>/cost (3, 4)                       cost at z[i] of method focus_cases.METHODS[j], from the rays with w >= 0
  <case>/x, /fun                           the direct solution for the bounds (0, 16)
"""
from __future__ import annotations

import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))

import refload  # noqa: E402
import focus_cases as fc  # noqa: E402

ot = refload.load(0)


def main(path) -> None:
    RT = ot.Raytracer(outline=[-5, 5, -5, 5, -5, 60])
    cost = RT._Raytracer__focus_search_cost_function
    direct = RT._Raytracer__focus_rms_spot_direct_solution
    out = {}
    for name, args in fc.FIXTURE_CASES.items():
        pa, sb, w = fc.lines(**args)
        pk, sk, wk = fc.kept(pa, sb, w)
        pa3, sb3 = np.column_stack([pk, np.zeros(len(wk))]), np.column_stack([sk, np.ones(len(wk))])  # (N, 3) as in focus_search
        with np.errstate(all="ignore"):
            c = np.array([[float(cost(float(z), m, pa3, sb3, wk)) for m in fc.METHODS] for z in fc.Z_SAMPLES])
            res = direct(pa3, sb3, wk, fc.BOUNDS)
        out[f"{name}/pa"], out[f"{name}/sb"], out[f"{name}/w"], out[f"{name}/z"] = pa, sb, w, fc.Z_SAMPLES
        out[f"{name}/cost"], out[f"{name}/x"], out[f"{name}/fun"] = c, np.float64(res.x), np.float64(res.fun)
        print(name, len(wk), "kept", c.tolist(), float(res.x), float(res.fun))
    fc.write_npz(path, out)


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main(sys.argv[1] if len(sys.argv) > 1 else HERE / "focus_lines.npz")
