#!/usr/bin/env python3
"""tests/golden/refraction_step.npz: what the reference's refraction step (optrace/tracer/raytracer.py,
Raytracer.__refraction and __refraction_ideal_lens, with __compute_polarization inside) gives for the rays of
tests/refraction_cases.py, and what the same formulas give when they are evaluated exactly.

Runs only where the reference is installed (imported through oracle/refload.py) and mpmath is; the .npz is committed, the
reference is not.  Re-run with
    python tests/golden/generate_golden_refraction.py [output.npz]
The archive is written with fixed zip time stamps, so a second run reproduces the file byte for byte.

The inputs are not stored: refraction_cases.inputs(scene) regenerates them, `<scene>/checksum` ties them to the archive.
Keys, per scene of refraction_cases.scenes() with n rays:
  <scene>/checksum       refraction_cases.checksum of the inputs
  <scene>/normal (3,)    the unit normal of the tested surface as the surface classes carry it
  <scene>/w1    (n,) f32      weight behind the tested surface (the ideal lens leaves it alone)
  <scene>/pol1  (n, 3) f32    polarisation behind the tested surface
  <scene>/s1    (n, 3) f64    direction behind the tested surface (NaN after a total reflection; dead rays keep s0)
  <scene>/s_out (n, 3) f64    direction behind the element: after the plate's back face (z = +D2, normal (0, 0, 1), a second
                              call of __refraction on every ray that left the front with power), or behind the ideal lens.
                              Both normals are constant, so this is a function of the front's s' alone.
  <scene>/tir   (n,) bool, /tir_count   the total-reflection verdicts of the live rays at the tested surface
  <scene>/T_hi (n,) f64, /T_lo (n,) f32           the transmission of the reference's formulas evaluated exactly (mpmath,
  <scene>/pol_hi (n, 3) f64, /pol_lo (n, 3) f32   400 bits) on the binary values of the inputs; NaN where they have no
                              value: dead rays, total reflection, s' == s exactly (N == 1, or m == 0 in exact arithmetic)
While it runs it also checks that refraction_cases.reference_step / reference_ideal (the same lines in NumPy float64)
reproduce the reference's s', weights and float32 polarisation bit for bit, so that the host test may use that restatement
for the reference's own arithmetic error before the float32 store.
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
import refraction_cases as rc  # noqa: E402

ot = refload.load(0)


def same_bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def run_scene(RT, sc) -> dict:
    inp = rc.inputs(sc)
    n = inp["s0"].shape[0]
    live = inp["w0"] > 0
    p = np.zeros((n, 3, 3), order="F")
    p[:, 0] = inp["p0"]
    s = np.array(inp["s0"], order="F")
    w = np.zeros((n, 3), dtype=np.float32, order="F")
    w[:, 0] = w[:, 1] = inp["w0"]
    pols = np.zeros((n, 3, 3), dtype=np.float32, order="F")
    pols[:, 0] = pols[:, 1] = inp["pol0"]
    msg = np.zeros((len(RT.INFOS), 3), dtype=int)
    n1, n2 = np.full(n, sc.n1), np.full(n, sc.n2)
    T_hi, T_lo = np.full(n, np.nan), np.full(n, np.nan, dtype=np.float32)
    pol_hi, pol_lo = np.full((n, 3), np.nan), np.full((n, 3), np.nan, dtype=np.float32)

    if sc.D is not None:
        disc = ot.CircularSurface(r=rc.IDEAL_R)
        disc.move_to([0, 0, 0])
        p[:, 1], hit, _ = disc.find_hit(p[:, 0], s)
        assert np.all(hit)
        RT._Raytracer__refraction_ideal_lens(disc, sc.D, p, s, pols, live, 0, msg)
        re = rc.reference_ideal(sc.D, disc.pos, p[:, 1], inp["s0"], inp["pol0"])
        assert same_bits(re["s_"][live], s[live]) and same_bits(re["pol_"].astype(np.float32)[live], pols[live, 1])
        for r in np.nonzero(live)[0]:
            ex = rc.exact_ideal(sc.D, disc.pos, p[r, 1], inp["s0"][r], inp["pol0"][r])
            if ex is not None:
                for c in range(3):
                    pol_hi[r, c], pol_lo[r, c] = rc.split(ex[c])
        tir = np.zeros(n, dtype=bool)
        s1 = s.copy()
    else:
        front, back = rc.front_surface(ot, sc), ot.CircularSurface(r=rc.R_PLATE)
        front.move_to([0, 0, -rc.D1])
        back.move_to([0, 0, rc.D2])
        p[:, 1], hit, _ = front.find_hit(p[:, 0], s)
        assert np.all(hit)
        normal = front.normals(p[:1, 1, 0], p[:1, 1, 1])[0]
        assert same_bits(normal, rc.unit_normal(sc.normal))
        with np.errstate(all="ignore"):
            RT._Raytracer__refraction(front, p, s, w, n1, n2, pols, live, 0, msg)
        re = rc.reference_step(normal, inp["s0"], inp["pol0"], sc.n1, sc.n2)
        w1 = (inp["w0"] * re["T"]).astype(np.float32)
        assert same_bits(re["s_"][live], s[live]) and same_bits(w1[live], w[live, 1])
        assert same_bits(re["pol_"].astype(np.float32)[live], pols[live, 1])
        s1 = s.copy()
        tir = np.zeros(n, dtype=bool)
        tir[live] = re["tir"][live]
        assert msg[RT.INFOS.TIR, 0] == np.count_nonzero(tir) and np.all(w[tir, 1] == 0)
        for r in np.nonzero(live & ~tir)[0]:
            ex = rc.exact_step(normal, inp["s0"][r], inp["pol0"][r], sc.n1, sc.n2)
            if ex is not None:
                T_hi[r], T_lo[r] = rc.split(ex[0])
                for c in range(3):
                    pol_hi[r, c], pol_lo[r, c] = rc.split(ex[1][c])
        # the back face, for every ray that still has power (whether it would meet the disc or not: the normal is constant)
        on = w[:, 1] > 0
        w[:, 2], pols[:, 2], p[:, 2] = w[:, 1], pols[:, 1], p[:, 1]
        if np.any(on):
            with np.errstate(all="ignore"):
                RT._Raytracer__refraction(back, p, s, w, n2, n1, pols, on, 1, msg)
    k = sc.name
    return {f"{k}/checksum": np.array(rc.checksum(inp)), f"{k}/normal": rc.unit_normal(sc.normal), f"{k}/w1": w[:, 1], f"{k}/pol1": pols[:, 1], f"{k}/s1": s1, f"{k}/s_out": s,
            f"{k}/tir": tir, f"{k}/tir_count": np.int64(np.count_nonzero(tir)), f"{k}/T_hi": T_hi, f"{k}/T_lo": T_lo,
            f"{k}/pol_hi": pol_hi, f"{k}/pol_lo": pol_lo}


def main(path) -> None:
    RT = ot.Raytracer(outline=[-12, 12, -12, 12, -12, 40])
    out, total = {}, 0
    for sc in rc.scenes():
        res = run_scene(RT, sc)
        out.update(res)
        n = res[f"{sc.name}/w1"].shape[0]
        total += n
        print(f"{sc.name:16s} {n:5d} rays, {int(res[f'{sc.name}/tir_count']):3d} TIR, "
              f"{int(np.count_nonzero(np.isfinite(res[f'{sc.name}/pol_hi'][:, 0]))):5d} with exact values", flush=True)
    rc.write_npz(path, out)
    print(total, "rays,", pathlib.Path(path).stat().st_size, "bytes")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main(sys.argv[1] if len(sys.argv) > 1 else HERE / "refraction_step.npz")
