#!/usr/bin/env python3
"""Golden values for the paraxial analysis (TMA), from the upstream NumPy reference.  Like generate_golden.py this runs
only where the reference is installed; tma.npz is committed, the reference is not.
    python tests/golden/generate_golden_tma.py

tma.npz
  sys/...                        six arrays that hold, packed (scenes_tma.pack / unpack), for all systems:
  systems                        names of scenes_tma.systems
  <system>/attr/<name>           every public attribute as float64 (tuples: shape (2,), abcd: (2, 2)), /type/<name> its type
  <system>/z, /<method>, /err/<method>   image_position, image_magnification, object_position, object_magnification at
                                 scenes_tma.arguments()["z"]: value (NaN where it raised) and class name raised or "none"
  <system>/zz, /matrix_at        matrix_at at pairs of planes;  /zs, /pupil_position, /pupil_magnification: per stop
  raises/<case>                  class name of what tma_cases.cases raises, or "none"
  ideal/<one|two>/...            off-axis point imaged by ideal lenses: image plane and point after the analysis, largest
                                 distance of a traced hit from that point (spread), rays traced
  focus/<scene>/...              thin collimated beam: injected initial rays, focal_points[1], position found by
                                 focus_search("RMS Spot Size") started there, search bounds, rays used

Printed, for the tolerances of tests/test_tma_host.py: the reference's own largest deviation between an evaluation and
the same system with the lens list reversed and, where wl is a whole number, wl given as int."""
from __future__ import annotations

import numpy as np

import generate_golden as gg  # (imports the reference, tests/scenes.py and the oracle loader)

import scenes_tma as st
import tma_cases

ot = gg.ot
HERE = gg.HERE

ATTRS = ("wl", "vertex_points", "n1", "n2", "abcd", "principal_points", "nodal_points", "focal_points", "focal_lengths",
         "ffl", "bfl", "d", "efl", "efl_n", "focal_lengths_n", "powers", "powers_n", "optical_center")
POINT_METHODS = ("image_position", "image_magnification", "object_position", "object_magnification")


def record(tma, lenses: list) -> dict:
    out = {}
    for name in ATTRS:
        v = getattr(tma, name)
        out[f"attr/{name}"] = np.array(v, dtype=np.float64)
        out[f"type/{name}"] = type(v).__name__
        if isinstance(v, tuple):
            assert len(v) == 2 and all(type(e) is float for e in v), (name, v)
    args = st.arguments(lenses)
    out.update(args)
    with np.errstate(all="ignore"):
        for method in POINT_METHODS:
            vals, errs = [], []
            for z in args["z"]:
                try:
                    v = getattr(tma, method)(float(z))
                    assert type(v) is float, (method, type(v))
                    vals.append(v)
                    errs.append("none")
                except Exception as err:  # noqa: BLE001
                    vals.append(np.nan)
                    errs.append(type(err).__name__)
            out[method], out[f"err/{method}"] = np.array(vals), np.array(errs)
        out["matrix_at"] = np.array([tma.matrix_at(float(a), float(b)) for a, b in args["zz"]])
        pos = [tma.pupil_position(float(z)) for z in args["zs"]]
        mag = [tma.pupil_magnification(float(z)) for z in args["zs"]]
        assert all(type(e) is float for t in pos + mag for e in t) and all(type(t) is tuple for t in pos + mag)
        out["pupil_position"], out["pupil_magnification"] = np.array(pos), np.array(mag)
    return out


def deviation(a: dict, b: dict) -> tuple[float, float]:
    """Largest deviation between two recordings: abcd relative to max |abcd|; everything else relative, element by element
    (positions where both are NaN or equal infinities count as equal, a differing pattern as inf)."""
    d_abcd = float(np.abs(a["attr/abcd"] - b["attr/abcd"]).max() / np.abs(a["attr/abcd"]).max())
    worst = 0.
    for key, x in a.items():
        if key.startswith(("type/", "err/")) or key in ("attr/abcd", "attr/wl", "z", "zz", "zs"):
            continue
        x, y = np.asarray(x, dtype=np.float64), np.asarray(b[key], dtype=np.float64)
        same = (np.isnan(x) & np.isnan(y)) | (x == y)
        if np.any(~same & ~(np.isfinite(x) & np.isfinite(y))):
            return d_abcd, np.inf
        if np.any(~same):
            worst = max(worst, float((np.abs(x - y)[~same] / np.abs(x)[~same]).max()))
    return d_abcd, worst


def gen_systems(out: dict) -> None:
    names = list(st.systems(ot))
    packed = {"systems": np.array(names)}
    worst = {False: [0., 0.], True: [0., 0.]}
    for name in names:
        entry = st.systems(ot)[name]
        tma, lenses = st.analysis(ot, entry)
        rec = record(tma, lenses)
        if name.startswith("plate"):
            assert tma.abcd[1, 0] == 0.0, "the afocal case must be an exact zero"
        for k, v in rec.items():
            packed[f"{name}/{k}"] = v
        variants = [dict(reverse=True)] + ([dict(int_wl=True)] if float(entry[2]).is_integer() else [])
        for kw in variants:
            other = record(*st.analysis(ot, entry, **kw))
            for k in rec:
                if k.startswith(("type/", "err/")) and k != "type/wl":
                    assert np.array_equal(rec[k], other[k]), (name, k)
            d = deviation(rec, other)
            w = worst[name in st.NEAR_AFOCAL]
            w[0], w[1] = max(w[0], d[0]), max(w[1], d[1])
        print(f"  {name}: C={tma.abcd[1, 0]:.6g} efl={tma.efl:.9g}")
    out.update(st.pack(packed, "sys"))
    print(f"reference against itself (reversed list, int wl), all but {st.NEAR_AFOCAL}: "
          f"abcd {worst[False][0]:.3g} of max|abcd|, derived values {worst[False][1]:.3g} relative")
    print(f"reference against itself, {st.NEAR_AFOCAL}: abcd {worst[True][0]:.3g}, derived values {worst[True][1]:.3g}")


def gen_raises(out: dict) -> None:
    for name, case in tma_cases.cases(ot).items():
        out[f"raises/{name}"] = tma_cases.outcome(case)
        print(f"  raises/{name}: {out[f'raises/{name}']}")


IDEAL_N = 200_000


def gen_ideal(out: dict) -> None:
    for j, which in enumerate(("one", "two")):
        gg.refload.reseed(ot, 1200 + j)
        RT, zb, point = st.ideal_imaging_scene(ot, which)
        RT.trace(IDEAL_N)
        assert not RT.geometry_error
        hits, alive = st.plane_hits(RT.rays, zb)
        assert alive.all(), "every ray has to reach the image plane"
        spread = float(np.hypot(hits[:, 0] - point[0], hits[:, 1] - point[1]).max())
        out[f"ideal/{which}/zb"], out[f"ideal/{which}/point"] = zb, np.array(point)
        out[f"ideal/{which}/spread"], out[f"ideal/{which}/N"] = spread, IDEAL_N
        print(f"ideal lenses ({which}): image plane z={zb:.12g}, point {point}, largest distance of {IDEAL_N} hits: "
              f"{spread:.3g} mm")


FOCUS_N = 2000


def gen_focus(out: dict) -> None:
    for j, name in enumerate(st.FOCUS_SCENES):
        RT, rec, _ = gg.trace_recorded(lambda ot_, **kw: st.focus_scene(ot_, name, **kw), FOCUS_N, 1300 + j, no_pol=True)
        F2 = RT.tma().focal_points[1]
        with ot.global_options.no_warnings():
            res, d = RT.focus_search("RMS Spot Size", z_start=F2)
        k = f"focus/{name}"
        out[f"{k}/p0"], out[f"{k}/s0"] = np.vstack([r[0] for r in rec]), np.vstack([r[1] for r in rec])
        out[f"{k}/w0"] = np.concatenate([r[3] for r in rec])
        out[f"{k}/wl"] = np.concatenate([r[4] for r in rec]).astype(np.float32)
        out[f"{k}/N_list"] = np.array(RT.rays.N_list)
        out[f"{k}/beam_radius"] = float(RT.ray_sources[0].surface.r)
        out[f"{k}/F2"], out[f"{k}/x"], out[f"{k}/fun"] = F2, float(res.x), float(res.fun)
        out[f"{k}/bounds"], out[f"{k}/N"] = np.array(d["bounds"]), d["N"]
        assert d["bounds"][0] < F2 < d["bounds"][1]
        print(f"focus {name}: beam radius {out[f'{k}/beam_radius']:.4g} mm, focal_points[1]={F2:.9g}, RMS focus "
              f"{float(res.x):.9g}, paraxial residual {float(res.x) - F2:+.3g} mm (search span "
              f"{d['bounds'][1] - d['bounds'][0]:.4g} mm, {d['N']} rays)")


if __name__ == "__main__":
    out = {}
    gen_systems(out)
    gen_raises(out)
    gen_ideal(out)
    gen_focus(out)
    np.savez_compressed(HERE / "tma.npz", **out)
    print("tma.npz", len(out))
