#!/usr/bin/env python3
"""Generate tests/golden/detectors.npz: detector hits of the reference for every detector kind at every placement.

Runs ONLY in the build container (needs the reference checkout, imported through oracle/refload.py); run by hand with
    python tests/golden/generate_golden_detectors.py
and never imported by a test.  Seeded and single-threaded: two runs write identical arrays.

Two scenes of tests/scenes.py (DETECTOR_SCENES) are traced once each; per scene the injected rays and every section are
stored like in trace_<scene>.npz.  Then one record per (kind, placement, projection) of `scenes.detector_records`, named
<scene>/<kind>/<placement>/<projection>: where the detector stood, what Raytracer._hit_detector returned (ph, w, wl, extent,
ill), the sparse detector_image with its extent and power, and under <scene>/<kind>/<placement>/user an image with a user
extent and the last source alone.  The records are stored concatenated (class Store; read by tests/detector_fixture.py).
Image values are stored as float32 (the tests compare images in image norm to 1e-4; powers are kept in float64).

Margins.  A record is only written when no ray sits on a decision threshold of the hit search, so that the tests need no
exclusions; otherwise the detector is displaced by a fraction of a millimetre and tried again (the position is part of the
record).  With `margins` below, for every living ray at every section the search tests it on:
  * the hit's z is not within 1e-9 of the section's end + C_EPS (the retry decision);
  * the hit is not within 1e-9 of the outline of the detector's mask (no mask_func surface can be a detector,
    detector.py:39-41, so there is no bitmap margin to keep);
  * no section start lies within 1e-9 of the detector's z_min / z_max.  Exact equality is admitted for section 0 alone: the
    injected start positions are the same doubles on both sides (a flat detector in the source plane), whereas any later
    position is computed and may differ in the last bit.
"""
from __future__ import annotations

import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))

from generate_golden import ot, sparse, trace_recorded  # noqa: E402  (loads the reference through oracle/refload.py)
import scenes  # noqa: E402

TOL = 1e-9
SEEDS = {"objective": 700, "numeric": 701}


class Marginal(Exception):
    pass


def margins(RT, surf, kind: str) -> int:
    """Walk the hit search of Raytracer._hit_detector section by section with the surface's own find_hit and raise Marginal
    where a living ray sits on a threshold.  -> number of living rays that were sent on to a later section."""
    p, w = np.asarray(RT.rays.p_list), np.asarray(RT.rays.w_list)
    N, nt = w.shape
    z = p[:, :, 2]
    z_min, z_max = surf.extent[4:6]
    for zb in (z_min, z_max):
        d = np.abs(z - zb)
        near = d < TOL
        near[:, 0] &= d[:, 0] != 0
        if near.any():
            raise Marginal(f"section start within {TOL} of z = {zb}")
    ge, gx = z >= z_min, z >= z_max
    todo = ~(np.all(ge & gx, axis=1) | np.all(~ge & ~gx, axis=1))
    k = (np.argmax(ge, axis=1) - 1).clip(0)
    retried = np.zeros(N, dtype=bool)
    cx, cy = surf.pos[:2]
    while todo.any():
        k[todo] += 1
        todo &= k < nt
        r = np.nonzero(todo)[0]
        if not r.size:
            break
        a, b = p[r, k[r] - 1], p[r, k[r]]
        with np.errstate(invalid="ignore", divide="ignore"):
            s = (b - a) / np.linalg.norm(b - a, axis=1)[:, None]
            ph, ish, _ = surf.find_hit(np.asfortranarray(a), np.asfortranarray(s))
        live = (w[r, k[r] - 1] > 0) & np.isfinite(ph[:, 2])
        if np.any(np.abs(ph[live, 2] - (b[live, 2] + surf.C_EPS)) < TOL):
            raise Marginal("hit within 1e-9 of the section's end + C_EPS")
        x, y = ph[live, 0] - cx, ph[live, 1] - cy
        rad = np.hypot(x, y)
        edges = [rad - surf.r] if hasattr(surf, "r") else []
        if kind == "ring":
            edges.append(rad - surf.ri)
        if kind in ("rect", "slit"):
            edges = [np.abs(x) - surf.dim[0] / 2, np.abs(y) - surf.dim[1] / 2]
        if kind == "slit":
            edges += [np.abs(x) - surf.dimi[0] / 2, np.abs(y) - surf.dimi[1] / 2]
        for e in edges:
            if np.any(np.abs(e) < TOL):
                raise Marginal("hit within 1e-9 of the outline")
        again = ph[:, 2] > b[:, 2] + surf.C_EPS
        retried[r[again & live]] = True
        todo[r] = again
    return int(np.count_nonzero(retried))


def user_extent(det):
    e0 = np.array(det.extent[:4])
    cx, cy = (e0[0] + e0[1]) / 2, (e0[2] + e0[3]) / 2
    return [cx - (e0[1] - e0[0]) / 5, cx + (e0[1] - e0[0]) / 4, cy - (e0[3] - e0[2]) / 4, cy + (e0[3] - e0[2]) / 6]


class Store:
    """The records, concatenated: a few long arrays instead of a dozen short ones per record (an .npz spends some 200 bytes on
    every array it holds).  tests/detector_fixture.py reads this layout."""

    def __init__(self):
        self.rec = dict(keys=[], pos=[], extent=[], ill=[], n=[], ph=[], w=[], wl=[])
        self.img = dict(keys=[], uext=[], extent=[], power=[], shape=[], n=[], iy=[], ix=[], val=[])

    def put_hits(self, key, pos, ph, w, wl, ext, ill):
        r = self.rec
        r["keys"].append(key), r["pos"].append(pos), r["extent"].append(ext), r["ill"].append(ill), r["n"].append(w.shape[0])
        r["ph"].append(ph.reshape(-1, 3)), r["w"].append(w), r["wl"].append(wl)

    def put_image(self, key, img, uext=None):
        sp, m = sparse(img._data), self.img
        m["keys"].append(key), m["uext"].append([np.nan] * 4 if uext is None else uext), m["extent"].append(img.extent)
        m["power"].append(img.power()), m["shape"].append(sp["shape"]), m["n"].append(sp["iy"].shape[0])
        m["iy"].append(sp["iy"]), m["ix"].append(sp["ix"]), m["val"].append(sp["val"])

    def arrays(self) -> dict:
        r, m = self.rec, self.img
        return {
            "rec/keys": np.array(r["keys"]), "rec/pos": np.array(r["pos"], dtype=np.float64),
            "rec/extent": np.array(r["extent"], dtype=np.float64), "rec/ill": np.array(r["ill"], dtype=np.int64),
            "rec/n": np.array(r["n"], dtype=np.int64), "rec/ph": np.vstack(r["ph"]).astype(np.float64),
            "rec/w": np.concatenate(r["w"]).astype(np.float32), "rec/wl": np.concatenate(r["wl"]).astype(np.float32),
            "img/keys": np.array(m["keys"]), "img/uext": np.array(m["uext"], dtype=np.float64),
            "img/extent": np.array(m["extent"], dtype=np.float64), "img/power": np.array(m["power"], dtype=np.float64),
            "img/shape": np.array(m["shape"], dtype=np.int64), "img/n": np.array(m["n"], dtype=np.int64),
            "img/iy": np.concatenate(m["iy"]).astype(np.int16), "img/ix": np.concatenate(m["ix"]).astype(np.int16),
            "img/val": np.vstack(m["val"]).astype(np.float32),
        }


def gen_scene(name: str, out: dict, store: Store, summary: dict):
    builder, N, rt_args = scenes.DETECTOR_SCENES[name]

    def build(ot_, **kw):
        RT = builder(ot_, **kw)
        build.idx = scenes.add_detectors(ot_, RT)
        return RT

    with ot.global_options.no_warnings():
        RT, rec, _ = trace_recorded(build, N, SEEDS[name], **rt_args)
    idx = build.idx
    out[f"{name}/N"] = N
    out[f"{name}/p0"] = np.vstack([r[0] for r in rec])
    out[f"{name}/s0"] = np.vstack([r[1] for r in rec])
    out[f"{name}/w0"] = np.concatenate([r[3] for r in rec])
    out[f"{name}/wl"] = np.concatenate([r[4] for r in rec]).astype(np.float32)
    if not RT.no_pol:
        out[f"{name}/pol0"] = np.vstack([r[2] for r in rec])
    out[f"{name}/N_list"] = RT.rays.N_list
    out[f"{name}/p_list"], out[f"{name}/w_list"] = np.array(RT.rays.p_list), np.array(RT.rays.w_list)
    assert np.array_equal(out[f"{name}/wl"], RT.rays.wl_list)
    died = np.count_nonzero((RT.rays.w_list[:, 1] > 0) & (RT.rays.w_list[:, -2] == 0))
    print(f"{name}: N={N} nt={RT.rays.Nt} msgs={RT._msgs.sum(axis=1)} rays lost on the way: {died}")

    done = set()
    with ot.global_options.no_warnings():
        for kind, place, proj in scenes.detector_records(name):
            det = RT.detectors[idx[kind]]
            base = f"{name}/{kind}/{place}"
            if (kind, place) not in done:  # position: the first displacement without a marginal ray
                for attempt in range(40):
                    pos = np.array(scenes.detector_position(RT, det.surface, place), dtype=np.float64)
                    pos[:2] += attempt * np.array([0.0137, 0.0071])
                    det.move_to(pos)
                    try:
                        retried = margins(RT, det.surface, kind)
                        break
                    except Marginal as why:
                        print(f"  {base}: {why}; displaced")
                else:
                    raise RuntimeError(f"{base}: no position without a marginal ray")
                done.add((kind, place))
                where = {**getattr(gen_scene, "where", {}), base: pos}
                gen_scene.where = where
                summary["retried"] += retried
            det.move_to(gen_scene.where[base])
            key = f"{base}/{proj}"
            ph, w, wl, ext, _, _, ill = RT._hit_detector("x", idx[kind], None, None, proj)
            if place in ("front", "beyond"):
                assert w.shape[0] == 0, f"{key}: no ray may reach / start before this placement"
            elif place not in ("source", "end") and kind != "tilted_ill":  # (the sources lie in a ring's hole and in the very plane of a flat detector,
                # a detector that bulges towards +z stands behind the outline's far face: any count there)
                assert w.shape[0] >= 50, f"{key}: only {w.shape[0]} hits"
            assert w.dtype == np.float32 and wl.dtype == np.float32
            store.put_hits(key, gen_scene.where[base], ph, w, wl, ext, ill)
            store.put_image(key, RT.detector_image(detector_index=idx[kind], projection_method=proj))
            summary["records"] += 1
            summary["ill"] += ill > 0
            summary["hits"].append((key, w.shape[0], int(ill)))
            if proj in (None, scenes.SPHERE_PROJECTIONS[0]):
                key = f"{base}/user"
                uext = user_extent(det)
                store.put_image(key, RT.detector_image(detector_index=idx[kind], extent=uext, projection_method=proj,
                                                       source_index=len(RT.ray_sources) - 1), uext)


def refused() -> np.ndarray:
    """names of `scenes.detector_refused` whose surface the reference's Detector does not take"""
    names = []
    for name, surf in scenes.detector_refused(ot).items():
        try:
            ot.Detector(surf, pos=[0, 0, 0])
        except RuntimeError:
            names.append(name)
    return np.array(names)


def main():
    out, summary = {}, dict(records=0, retried=0, ill=0, hits=[])
    out["refused"] = refused()
    print("not accepted as detector surfaces:", list(out["refused"]))
    store = Store()
    for name in scenes.DETECTOR_SCENES:
        gen_scene(name, out, store, summary)
    out.update(store.arrays())
    np.savez_compressed(HERE / "detectors.npz", **out)
    for key, n, ill in summary["hits"]:
        print(f"{key}: {n} hits" + (f", ill {ill}" if ill else ""))
    print(f"records: {summary['records']}; rays sent on to a later section: {summary['retried']}; "
          f"records with ill > 0: {summary['ill']}; file: {(HERE / 'detectors.npz').stat().st_size} bytes")
    assert summary["ill"] >= 1 and summary["retried"] >= 1


if __name__ == "__main__":
    main()
