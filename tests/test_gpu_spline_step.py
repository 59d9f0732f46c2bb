"""The spline path of the trace kernel (OT_HIT_SPLINE: find_hit, surf_values, surf_normal, data_gradient of
csrc/ot_device.hpp on csrc/ot_spline.hpp with its PatchCache) against the exact spline the surface carries, ray by ray
(tests/spline_cases.py): through the leaf operators (no cache: FITPACK's order with arithmetic knot cells) and through the
trace kernel (the LDS patch, fused row sums, analytic gradients from the patch of the hit search).

What it is pinned to (u = 2^-53, K = 32; see spline_cases for the bars and the count of roundings):
  values      K u A0 + (|S_x| + |S_y|) delta, and u |z| for the absolute height that Surface.values returns
  normals     the gradient bars of both components + 4 u
  hit points  1e-7 |s_j| + K u (|p|_inf + |o|_2 + |t|), exact verdicts where they are decided; `parallel` rays, whose x and y
              are the start's bitwise, also in z by the value bar + K u (|p| + |o| + |t|)
  direction   behind the surface, from the two stored points (the final direction for a ray that misses the lens's back),
              against the exact refraction at the exact normal of the carried spline at the kernel's own hit point: 16 u +
              twice the normal bar + 4 u (|p1| + |p2|) / |p2 - p1|.  A gradient from the neighbouring patch of a 50-grid is
              off by 1e-3, ten orders above this
Measured on an MI355X: DESIGN.md, "Spline surfaces at their edges".
"""
import functools

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd.scene import CompiledScene

import spline_cases as sc

pytestmark = pytest.mark.gpu

MISSING = 0   # Raytracer.INFOS
LD = sc.LD


def bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@functools.lru_cache(maxsize=None)
def surface(sn: str):
    with ot.global_options.no_warnings():
        return sc.placed(ot, sn)


@pytest.mark.parametrize("sn", list(sc.PLAN))
def test_leaf_operators_against_the_exact_spline(sn, capsys):
    """values, normals and find_hit of the leaf surface at the exact hit points of every class (for `parallel` and the
    on-knot targets of `knot` these are the aimed coordinates bit for bit) and on the rays themselves."""
    sf, sp = surface(sn), sc.spline(ot, sn)
    assert np.array_equal(np.asarray(sf._tab), sp.tab), "the placed surface carries the tables of the truth"
    lines, bad = [f"{sn}: delta = {sp.delta:.2e} mm = {sp.delta / sp.h:.1e} h, {sp.n} knots"], []
    for fam in sc.PLAN[sn]:
        k = sc.key(sn, fam)
        inp, ex, _ = sc.case(ot, sn, fam)
        x = np.ascontiguousarray(ex["point"][:, 0].astype(np.float64))
        y = np.ascontiguousarray(ex["point"][:, 1].astype(np.float64))
        if fam == "parallel":
            x, y = np.ascontiguousarray(inp["p0"][:, 0]), np.ascontiguousarray(inp["p0"][:, 1])
        pt = sp.point(x.astype(LD), y.astype(LD))
        # a point within 1e-9 of the edge of the mask may be on either side of it in float64: values are continuous there to
        # a slope times N_EPS, normals are not
        clear = np.abs(np.sqrt((x - sp.pos[0]).astype(LD) ** 2 + (y - sp.pos[1]).astype(LD) ** 2) - (LD(sp.r) + LD(sc.N_EPS))) > 1e-9
        v = sf.values(x, y)
        assert np.all(np.isfinite(v)), k
        vr = float(np.max((np.abs(v.astype(LD) - pt["z"]) / pt["Vz"])[clear], initial=0.0))
        sel = pt["inside"] & clear
        nr = sc.normal_ratio(sp, x[sel], y[sel], sf.normals(np.ascontiguousarray(x[sel]), np.ascontiguousarray(y[sel]))) if sel.any() else 0.0
        ph, hit, ill = sf.find_hit(inp["p0"], inp["s0"])
        assert np.all(np.isfinite(ph)), k
        assert not np.any(ill), f"{k}: every bracket of these classes has a sign change"
        res = sc.check(sp, fam, inp, ex, ph, hit)
        ok = sc.passes(res) and vr <= 1 and nr <= 1
        lines.append(sc.report("leaf", k, res).replace("   <-- FAILS", "") + f", values {vr:.3f}, normals {nr:.3f} of their bars"
                     + ("" if ok else "   <-- FAILS"))
        if not ok:
            bad.append(k)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, bad


class Run:
    """One launch: every class of a surface, one after the other."""


@functools.lru_cache(maxsize=None)
def run(sn: str, variant: str) -> Run:
    two = variant == "two_splines"
    cases = [sc.case(ot, sn, fam, two) for fam in sc.PLAN[sn]]
    inps = [c[0] for c in cases]
    cat = {key: np.concatenate([i[key] for i in inps]) for key in ("p0", "s0", "pol0", "w0", "wl")}
    n = cat["s0"].shape[0]
    r = Run()
    with ot.global_options.no_warnings():
        RT = sc.raytracer(ot, sn, variant)
        RT.trace(n, _initial_rays=(cat["p0"], cat["s0"], None if RT.no_pol else cat["pol0"], cat["w0"], cat["wl"]),
                 _N_list=np.array([n]))
        assert not RT.geometry_error
        r.p, r.w, r.s = RT.rays.p_list.copy(), RT.rays.w_list.copy(), RT.rays.s0_list.copy()
        r.msgs = np.array(RT._msgs)
        front = CompiledScene(RT).surfaces[1 if two else 0]
    r.front = np.array([*front.pos, front.z_min, front.z_max])
    r.cases, r.n, r.sec = cases, n, (2 if two else 1)
    assert n % 64 != 0 and n > 4 * 256
    return r


@pytest.mark.parametrize("sn,variant", [(sn, v) for sn in sc.PLAN for v in sc.VARIANTS])
def test_trace_kernel_against_the_exact_spline(sn, variant, capsys):
    """The section behind the tested surface: the point find_hit<OT_HIT_SPLINE> returned inside the trace kernel (alive if
    and only if the exact verdict is a hit; the MISSING counter; dead rays unmoved; everything finite), and the direction
    the ray leaves with, which carries the normal the kernel took from its patch cache.  `no_pol` and `continuous` are
    bit-equal to `plain` up to that section, `hurb` as well; `two_splines`, whose rays start further back and arrive through
    another spline surface (a filter of transmission 1), agrees within the two numeric bars."""
    r = run(sn, variant)
    sp = sc.spline(ot, sn)
    k1 = r.sec
    assert np.array_equal(r.front, [*sp.pos, sp.z_min, sp.z_max]), "the lens front stands where the leaf surface stands"
    lines, bad, thin, missing, seen, a = [], [], [], 0, 0, 0
    for fam, (inp, ex, _) in zip(sc.PLAN[sn], r.cases):
        k = sc.key(sn, fam)
        sl = slice(a, a + inp["s0"].shape[0])
        a = sl.stop
        live = inp["w0"] > 0
        pts, alive = r.p[sl, k1], r.w[sl, k1] > 0
        assert np.all(np.isfinite(r.p[sl])) and np.all(np.isfinite(r.w[sl])), k
        seen += int(np.count_nonzero(live))
        res = sc.check(sp, fam, inp, ex, pts, alive, sel=live)
        und = sc.undecided(sp, fam, inp, ex)
        missing += int(np.count_nonzero(live & ~und & ~ex["hit"])) + int(np.count_nonzero(live & und & ~alive))
        assert np.all(r.p[sl][~live] == inp["p0"][~live, None, :]) and np.all(r.w[sl][~live] == 0), f"{k}: dead rays moved"
        # the direction behind the surface, of the rays that are hits: from the next stored point for those that reach the
        # lens's back, the final direction for those that miss it (absorbed there, where they stand)
        nxt = r.p[sl, k1 + 1]
        go = live & alive & ex["hit"] & ((r.w[sl, k1 + 1] > 0) | np.all(nxt == pts, axis=1))
        dr = sc.direction_check(sp, inp["s0"][go], pts[go], nxt[go], r.s[sl][go]) if go.any() else 0.0
        ok = sc.passes(res) and dr <= 1
        lines.append(sc.report(f"trace {variant}", k, res).replace("   <-- FAILS", "") + f", direction {dr:.3f} of its bar ({int(go.sum())} rays)"
                     + ("" if ok else "   <-- FAILS"))
        if not ok:
            bad.append(k)
        if fam not in ("miss", "rim", "end") and np.count_nonzero(go) < 0.8 * np.count_nonzero(live):
            thin.append(f"{k}: {np.count_nonzero(go)} rays carry a direction")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, bad
    assert not thin, thin
    assert r.msgs[MISSING, k1] == missing, (r.msgs[MISSING], missing)
    assert np.all(r.msgs[MISSING, 1:k1] == 0), "no ray is lost in front of the tested surface"
    assert seen >= 0.8 * r.n
    if variant == "plain":
        return
    base = run(sn, "plain")
    if variant == "two_splines":
        a = 0
        for fam, (inp, ex, _), (inp0, ex0, _) in zip(sc.PLAN[sn], r.cases, base.cases):
            sl = slice(a, a + inp["s0"].shape[0])
            a = sl.stop
            live = inp["w0"] > 0
            bar = sc.hit_bars(sp, inp, ex) + sc.hit_bars(sp, inp0, ex0)
            und = sc.undecided(sp, fam, inp, ex)
            assert np.all((np.abs(r.p[sl, 2] - base.p[sl, 1]) <= bar)[live]), f"{sn}/{fam}: differs from plain by more than both bars"
            assert np.array_equal((r.w[sl, 2] > 0)[live & ~und], (base.w[sl, 1] > 0)[live & ~und]), f"{sn}/{fam}: verdicts differ from plain"
        return
    assert bits(r.p[:, :2], base.p[:, :2]), f"{sn} {variant}: sections 0 .. 1 differ from plain"
    if variant != "no_pol":
        assert bits(r.w[:, :2], base.w[:, :2]), f"{sn} {variant}: weights of sections 0 .. 1 differ from plain"
