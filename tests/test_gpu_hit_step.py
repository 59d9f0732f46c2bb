"""The surface hit step (find_hit, find_hit_conic, find_hit_asphere, illinois_search, handle_abnormal_f of
csrc/ot_device.hpp; detector_hit of csrc/ot_detector.hpp) against exact intersections at its edges
(tests/hit_cases.py, tests/golden/hit_step.npz): through the leaf operator, through the trace kernel in its hit levels, and
through the detector hit search; with it the conic normals at the exact hit coordinates.

What it is pinned to, per ray and coordinate (u = 2^-53, K = 32, see hit_cases for the count):
  closed forms   K u (|p|_inf + |o|_2 + |t|) around the exact point, hits and no-hit points alike; `tangent` times the
                 exact |B| / D; a start behind the surface comes back bitwise
  numeric hits   1e-7 |s_j| on top: C_EPS / 10 is the bracket width at which illinois_search leaves
  verdicts       the exact one for every ray whose exact radius is decided (everywhere but in the innermost rungs of `rim`);
                 the undecided ones may go either way, consistently with their own point
The reference is no yardstick here: tests/test_hit_host.py prints how far it is from these values (up to 0.75 mm and lost
rays for a beam 2^-20 off the axis of a paraboloid), and the oracle follows it bit for bit.

Measured on an MI355X, before this pin's change of find_hit_conic and after: DESIGN.md, "The hit step at its edges".
"""
import functools

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd.scene import CompiledScene

import hit_cases as hc
from helpers import load

pytestmark = pytest.mark.gpu

MISSING = 0   # Raytracer.INFOS
ALL_VARIANTS = ("par6", "sph8", "con_m75", "asph_a", "asph_n13", "tilted", "circle")   # the others run `plain` alone


@pytest.fixture(scope="module")
def g():
    return load("hit_step.npz")


def bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def surface(sn: str):
    with ot.global_options.no_warnings():
        return hc.placed(ot, sn)


def eps2(sn: str):
    d = hc.SURFACES[sn]
    return (d["r"] + hc.N_EPS) ** 2, ((d["ri"] - hc.N_EPS) ** 2 if d["kind"] == "ring" else None)


def report(title, k, res) -> str:
    ok = res["ratio"] <= 1 and res["wrong"] == 0 and res["consistent"]
    return (f"{title:22s} {k:18s} {res['err']:.1e} mm = {res['ratio']:9.2e} of the bar, {res['wrong']:2d} wrong verdicts, "
            f"{res['undecided']:2d} undecided" + ("" if ok else "   <-- FAILS"))


@pytest.mark.parametrize("sn", list(hc.PLAN))
def test_leaf_operator_against_exact_hits(g, sn, capsys):
    sf = surface(sn)
    assert np.array_equal([*sf.pos, sf.z_min, sf.z_max], g[f"{sn}/geom"][:5])
    lines, bad = [], []
    for fam in hc.PLAN[sn]:
        k = hc.key(sn, fam)
        inp = hc.inputs(sn, fam)
        assert hc.checksum(inp) == str(g[f"{k}/checksum"])
        ph, hit, ill = sf.find_hit(inp["p0"], inp["s0"])
        assert np.all(np.isfinite(ph)), k
        res = hc.check(g, sn, fam, inp, ph, hit, *eps2(sn))
        lines.append(report("leaf", k, res))
        if "FAILS" in lines[-1]:
            bad.append(k)
        if len(ill) and fam != "behind":   # every bracket of these classes has a sign change
            assert not np.any(ill), k
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, bad


class Run:
    """One launch: every class of a surface, one after the other."""


@functools.lru_cache(maxsize=None)
def run(sn: str, variant: str) -> Run:
    inps = [hc.inputs(sn, fam) for fam in hc.PLAN[sn]]
    cat = {key: np.concatenate([i[key] for i in inps]) for key in ("p0", "s0", "pol0", "w0", "wl")}
    n = cat["s0"].shape[0]
    r = Run()
    with ot.global_options.no_warnings():
        RT = hc.raytracer(ot, sn, variant)
        RT.trace(n, _initial_rays=(cat["p0"], cat["s0"], None if RT.no_pol else cat["pol0"], cat["w0"], cat["wl"]),
                 _N_list=np.array([n]))
        assert not RT.geometry_error
        r.p, r.w = RT.rays.p_list.copy(), RT.rays.w_list.copy()
        r.msgs = np.array(RT._msgs)
        front = CompiledScene(RT).surfaces[0]
    r.front = np.array([*front.pos, front.z_min, front.z_max])
    r.inps, r.cat, r.n = inps, cat, n
    return r


def trace_cases():
    return [(sn, v) for sn in hc.TRACED for v in (hc.VARIANTS if sn in ALL_VARIANTS else ("plain",))]


@pytest.mark.parametrize("sn,variant", trace_cases())
def test_trace_kernel_against_exact_hits(g, sn, variant, capsys):
    """Section 1 of every ray: the point find_hit<LEVEL> returned inside the trace kernel.  Alive behind the surface if and
    only if the exact verdict is a hit (n = 1 -> 1.5: no total reflection); the MISSING counter counts the live rays that
    do not hit; rays without power stay where they are.  The variants put a numeric-hit lens, a spline-surface lens, no
    polarisation or a continuous spectrum (the kernel without line tables; `plain` is monochromatic and has them) around
    the same surface: sections 0 .. 1 are bit-equal to `plain` in all of them."""
    r = run(sn, variant)
    assert np.array_equal(r.front, g[f"{sn}/geom"][:5]), "the lens front stands where the leaf surface stands"
    lines, bad, missing, seen, a = [], [], 0, 0, 0
    for fam, inp in zip(hc.PLAN[sn], r.inps):
        k = hc.key(sn, fam)
        sl = slice(a, a + inp["s0"].shape[0])
        a = sl.stop
        live = inp["w0"] > 0
        pts, alive = r.p[sl, 1], r.w[sl, 1] > 0
        assert np.all(np.isfinite(pts)), k
        back = hc.from_behind(g, sn, fam, inp)   # hits like any other; their power is the refraction step's business
        assert not np.any(back) or (sn == "hemi" and np.count_nonzero(back) <= 4), f"{k}: {np.count_nonzero(back)} hits from behind"
        seen += int(np.count_nonzero(live & ~back))
        res = hc.check(g, sn, fam, inp, pts, alive | back, *eps2(sn), sel=live)
        lines.append(report(f"trace {variant}", k, res))
        if "FAILS" in lines[-1]:
            bad.append(k)
        und = hc.undecided(g, k, inp)
        missing += int(np.count_nonzero(live & ~und & ~g[f"{k}/hit"])) + int(np.count_nonzero(live & und & ~alive))
        assert np.all(r.p[sl][~live] == inp["p0"][~live, None, :]) and np.all(r.w[sl][~live] == 0), f"{k}: dead rays moved"
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, bad
    assert r.msgs[MISSING, 1] == missing, (r.msgs[MISSING], missing)
    assert seen >= 0.8 * r.n
    if variant != "plain":
        base = run(sn, "plain")
        assert bits(r.p[:, :2], base.p[:, :2]), f"{sn} {variant}: sections 0 .. 1 differ from plain"
        if variant != "no_pol":
            assert bits(r.w[:, :2], base.w[:, :2]), f"{sn} {variant}: weights of sections 0 .. 1 differ from plain"


@pytest.mark.parametrize("sn", ["sph8", "par6"])
def test_conic_detectors_against_exact_hits(g, sn, capsys):
    """detector_hit<CONIC> reaches find_hit_conic: a collimated beam 2^-16 off the axis in free space, the tested conic as
    the detector; the hit list of Raytracer._hit_detector against the exact intersections of the stored sections."""
    fam = "tilt-16"
    k = hc.key(sn, fam)
    inp = hc.inputs(sn, fam)
    n = inp["s0"].shape[0]
    with ot.global_options.no_warnings():
        RT = ot.Raytracer(outline=[-12, 12, -12, 12, -12, 40])
        RT.add(ot.RaySource(ot.Point(), divergence="Isotropic", div_angle=5, pos=[0, 0, -10],
                            spectrum=ot.LightSpectrum("Monochromatic", wl=hc.WL)))
        RT.add(ot.Detector(hc.make_surface(ot, sn), pos=list(hc.POS)))
        RT.trace(n, _initial_rays=(inp["p0"], inp["s0"], inp["pol0"], inp["w0"], inp["wl"]), _N_list=np.array([n]))
        ph, hw, wl, ext, proj, ill = RT._hit_detector("x", 0, None, None, None)
    ph, hw = ph.cpu().numpy().reshape(3, n).T, hw.cpu().numpy()
    live = inp["w0"] > 0
    assert np.array_equal(hw > 0, live & g[f"{k}/hit"]) and np.all(g[f"{k}/hit"])
    res = hc.check(g, sn, fam, inp, ph, hw > 0, *eps2(sn), sel=live)
    with capsys.disabled():
        print("\n" + report("detector", k, res))
    assert res["ratio"] <= 1 and res["wrong"] == 0, res


def test_conic_normals_at_exact_hit_coordinates(g, capsys):
    """surface.normals at (hi_x, hi_y) against the exact unit normal there: 8 u per component, and 8 u / n_z for n_z on the
    near-hemisphere (the square root of a difference near zero: its argument carries ~4 u absolute)."""
    lines, bad = [], []
    for sn, fam in hc.CLASSES:
        k = hc.key(sn, fam)
        if f"{k}/n_hi" not in g:
            continue
        sel = g[f"{k}/hit"] & np.isfinite(g[f"{k}/n_hi"][:, 0])
        xy = g[f"{k}/hi"][sel]
        nd = surface(sn).normals(np.ascontiguousarray(xy[:, 0]), np.ascontiguousarray(xy[:, 1]))
        exact = hc.join(g[f"{k}/n_hi"][sel], g[f"{k}/n_lo"][sel])
        bar = np.full(exact.shape, 8 * hc.U, dtype=hc.LD)
        if sn == "hemi":
            bar[:, 2] = 8 * hc.U / exact[:, 2]
        ratio = float((np.abs(nd.astype(hc.LD) - exact) / bar).max())
        lines.append(f"normals {k:18s} n={int(sel.sum()):3d}  worst error / bar {ratio:.3f}" + ("" if ratio <= 1 else "   <-- FAILS"))
        if ratio > 1:
            bad.append(k)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert len(lines) >= 13 and not bad, bad
