#!/usr/bin/env python3
"""tests/golden/hit_step.npz: what the reference's find_hit gives for the rays of tests/hit_cases.py, and where those rays
meet the surface exactly.

Runs only where the reference is installed (imported through oracle/refload.py) and mpmath is; the .npz is committed, the
reference is not.  Re-run with
    python tests/golden/generate_golden_hit_step.py [output.npz]
The archive is written with fixed zip time stamps, so a second run reproduces the file byte for byte.

The inputs are not stored (p0 and s0 of 117 classes are 545 kB of incompressible doubles, which with the exact points would
not fit the 1 MiB of a committed file): hit_cases.inputs(surface, family) regenerates them from numpy's PCG64 stream and uniform(),
whose values NumPy keeps fixed across versions, and `<class>/checksum` ties them to the archive -- a test that draws other rays fails
at that assertion, before any comparison.
Keys, per surface `<s>` and class `<s>/<family>` with n rays:
  <s>/geom (8,)             centre, z_min, z_max and the tilted normal as the reference's surface carries them
  <class>/checksum
  <class>/hi (n, 3) f64, /lo (n, 3) f32    the exact point find_hit has to return: the hit, or the no-hit point
  <class>/t (n,) f64        its exact ray parameter (0 for a start behind the surface)
  <class>/hit (n,) bool     the exact verdict
  <class>/numeric (n,) bool the ray is decided by the numeric search (aspheres; rays that miss a tilted disc)
  <class>/ref_p (n, 3), /ref_hit, /ref_ill     the reference's find_hit
  <class>/ref_dev (3,)      the reference against the truth: worst error / bar, worst error in mm, wrong verdicts
  tangent:  <class>/cond (n,) f64          exact |B| / D
  rim:      <class>/delta (n,) f64         exact hit radius minus the edge of the mask, fl(r + N_EPS) (ring: the nearer edge)
            <class>/hit_hi, /hit_lo        conics: the exact intersection whether the mask takes it or not
  conic `wide` classes and every class of the near-hemisphere:
            <class>/n_hi (n, 3) f64, /n_lo (n, 3) f32   the exact unit normal at (hi_x, hi_y) of the rays that hit
  zoo_parab/geom, /idx, /hi, /lo, /t    scenes.surface_zoo's paraboloid: the rays of leaf_surfaces.npz whose reference hit is
                            farther from the exact one than hit_cases.ZOO_TOL (1 + |x|), and their exact hits
While it runs it asserts what hit_cases promises about verdicts: outside `rim` every exact hit radius is at least 1e-6 away
from the edges of the mask; inside `rim` at most half of the rays are undecided, and the reference's own verdicts on the
decided ones are the exact ones.
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
import hit_cases as hc  # noqa: E402

ot = refload.load(0)


def run_class(sf, ex, g, sn, fam) -> None:
    k = hc.key(sn, fam)
    d = hc.SURFACES[sn]
    inp = hc.inputs(sn, fam)
    n = inp["s0"].shape[0]
    hi, lo = np.zeros((n, 3)), np.zeros((n, 3), dtype=np.float32)
    hhi, hlo = np.full((n, 3), np.nan), np.full((n, 3), np.nan, dtype=np.float32)
    nhi, nlo = np.full((n, 3), np.nan), np.full((n, 3), np.nan, dtype=np.float32)
    t, hit, numeric, cond, delta = np.zeros(n), np.zeros(n, dtype=bool), np.zeros(n, dtype=bool), np.ones(n), np.zeros(n)
    edge = ex.mp.mpf(d["r"] + hc.N_EPS)
    want_normals = d["kind"] == "conic" and (fam == "wide" or sn == "hemi")
    for i in range(n):
        e = ex.hit(inp["p0"][i], inp["s0"][i])
        for c in range(3):
            hi[i, c], lo[i, c] = hc.split(e["point"][c])
            if "surface_point" in e:
                hhi[i, c], hlo[i, c] = hc.split(e["surface_point"][c])
        t[i], hit[i], numeric[i], cond[i] = float(e["t"]), e["hit"], e["numeric"], float(e["cond"])
        if e["radius"] is not None:
            dl = e["radius"] - edge
            if d["kind"] == "ring" and abs(e["radius"] - ex.mp.mpf(d["ri"] - hc.N_EPS)) < abs(dl):
                dl = e["radius"] - ex.mp.mpf(d["ri"] - hc.N_EPS)
            delta[i] = float(dl)
            if fam not in ("rim", "behind"):
                assert abs(dl) >= 1e-6, f"{k} ray {i}: exact radius within {float(dl):.1e} of the edge of the mask"
        elif fam == "rim":   # no root inside the z range at all (the surface has left it by more than N_EPS): decided, no hit
            delta[i] = np.inf
        if want_normals and e["hit"]:
            nv = ex.normal_at(ex.mp.mpf(hi[i, 0]), ex.mp.mpf(hi[i, 1]))
            for c in range(3):
                nhi[i, c], nlo[i, c] = hc.split(nv[c])
        if e["hit"]:
            assert abs(ex.residual(e["point"])) < 1e-40, k
    with np.errstate(all="ignore"):
        ref_p, ref_hit, ref_ill = sf.find_hit(np.asfortranarray(inp["p0"]), np.asfortranarray(inp["s0"]))
    ref_ill = np.zeros(n, dtype=bool) if len(ref_ill) == 0 else np.asarray(ref_ill, dtype=bool)
    g.update({f"{k}/checksum": np.array(hc.checksum(inp)), f"{k}/hi": hi, f"{k}/lo": lo, f"{k}/t": t, f"{k}/hit": hit,
              f"{k}/numeric": numeric, f"{k}/ref_p": np.ascontiguousarray(ref_p), f"{k}/ref_hit": np.asarray(ref_hit, dtype=bool),
              f"{k}/ref_ill": ref_ill})
    if fam == "tangent":
        g[f"{k}/cond"] = cond
    if fam == "rim":
        g[f"{k}/delta"] = delta
        if d["kind"] == "conic":
            g[f"{k}/hit_hi"], g[f"{k}/hit_lo"] = hhi, hlo
    if want_normals:
        g[f"{k}/n_hi"], g[f"{k}/n_lo"] = nhi, nlo
    res = hc.check(g, sn, fam, inp, ref_p, ref_hit)
    g[f"{k}/ref_dev"] = np.array([res["ratio"], res["err"], res["wrong"]])
    if fam == "rim":
        assert res["undecided"] <= n // 2, f"{k}: {res['undecided']} of {n} rays undecided"
        assert res["wrong"] == 0, f"{k}: the reference's verdict on a decided ray"
    print(f"{k:18s} hits {int(hit.sum()):3d}  numeric {int(numeric.sum()):3d}  undecided {res['undecided']:3d}   reference: "
          f"{res['err']:.1e} mm = {res['ratio']:.1e} of the bar, {res['wrong']} wrong verdicts", flush=True)


def zoo_parab(g) -> None:
    """The fixture rays of scenes.surface_zoo's paraboloid that the reference misses by more than hit_cases.ZOO_TOL."""
    import scenes
    sf = scenes.surface_zoo(ot)["conic_parab"]
    leaf = np.load(HERE / "leaf_surfaces.npz")
    p, s, ref = leaf["conic_parab/p"], leaf["conic_parab/s"], leaf["conic_parab/p_hit"]
    d = hc.SURFACES["zoo_parab"]
    assert (sf.r, sf.R, sf.k) == (d["r"], d["R"], d["k"])
    geom = hc.geometry(sf)
    ex = hc.Exact("zoo_parab", geom)
    idx, hi, lo, t = [], [], [], []
    for i in range(p.shape[0]):
        e = ex.hit(p[i], s[i])
        assert e["hit"] == bool(leaf["conic_parab/is_hit"][i]) or abs(e["radius"] - d["r"]) < 1e-6
        pt = [hc.split(v) for v in e["point"]]
        err = [abs(float(ex.mp.mpf(float(ref[i, c])) - e["point"][c])) for c in range(3)]
        if any(err[c] > hc.ZOO_TOL * (1 + abs(ref[i, c])) for c in range(3)):
            idx.append(i)
            hi.append([v[0] for v in pt])
            lo.append([v[1] for v in pt])
            t.append(float(e["t"]))
    g.update({"zoo_parab/geom": geom, "zoo_parab/idx": np.array(idx, dtype=np.int32), "zoo_parab/hi": np.array(hi),
              "zoo_parab/lo": np.array(lo, dtype=np.float32), "zoo_parab/t": np.array(t)})
    print(f"zoo conic_parab: the reference misses {len(idx)} of {p.shape[0]} fixture rays by more than {hc.ZOO_TOL:g}")


def main(path) -> None:
    g = {}
    for sn, fams in hc.PLAN.items():
        sf = hc.placed(ot, sn)
        geom = hc.geometry(sf)
        g[f"{sn}/geom"] = geom
        ex = hc.Exact(sn, geom)
        for fam in fams:
            run_class(sf, ex, g, sn, fam)
    zoo_parab(g)
    hc.write_npz(path, g)
    print(len(hc.CLASSES), "classes,", pathlib.Path(path).stat().st_size, "bytes")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main(sys.argv[1] if len(sys.argv) > 1 else HERE / "hit_step.npz")
