"""Host side of the spline pin (tests/spline_cases.py; no GPU): the host build of csrc/ot_spline.hpp path against path
(tests/cpp/spline_paths_test.cpp), the float64 restatement of the trace kernel's spline path (`fast_form`) inside every bar of
every class, the longdouble truth against SciPy and against mpmath, the preconditions of the classes, and three planted
mistakes that named classes catch."""
import functools
import pathlib
import subprocess

import numpy as np
import pytest

import optrace_amd as ot

import spline_cases as sc

ROOT = pathlib.Path(__file__).resolve().parent.parent
LD, SK = sc.LD, sc.SK


def _points(sp: sc.Spline, rng) -> np.ndarray:
    """(m, 2) arguments in the spline's own frame: every distinct knot with its two neighbouring doubles, the seam and end
    cells, points beyond the range, and random ones; the second coordinate is the same list in another order, and the
    knots also pair with themselves."""
    t, n = sp.t, sp.n
    ks = t[SK:n - SK]
    trip = np.concatenate((ks, np.nextafter(ks, -np.inf), np.nextafter(ks, np.inf)))
    seam = list(range(sp.ulo + SK - 2, sp.ulo + SK + 2)) + list(range(sp.uhi - SK - 1, sp.uhi - SK + 3))
    one = np.concatenate((trip, sc._cell_points(sp, rng, seam, 240)[0], sc._cell_points(sp, rng, [SK, n - SK - 2], 80)[0],
                          [sp.lo - 1e-10, sp.hi + 1e-10, sp.lo - 3e-10, sp.hi + 5e-11], rng.uniform(sp.lo, sp.hi, 300)))
    if sp.one_d:
        one = np.concatenate((one, [0.0, 1e-300, 1e-12, 1e-9]))
        return np.column_stack((one, np.zeros_like(one)))
    return np.concatenate((np.column_stack((one, rng.permutation(one))), np.column_stack((trip, trip))))


def test_host_build_of_the_header_path_against_path(tmp_path, capsys):
    """g++ build of ot_spline.hpp: cached / table / leaf values and gradients inside V and G, the A-B-A cache protocol, when
    the cached gradients apply, clamping, and every index checked against its array."""
    words = [3.0]
    for q, sn in enumerate(("d2_50", "d2_200", "d1_50")):
        sp = sc.spline(ot, sn)
        pts = _points(sp, np.random.default_rng([20263, q]))
        words += [1.0 if sp.one_d else 2.0, float(sp.n), float(sp.tab.size), sp.delta, sp.h2, float(pts.shape[0])]
        words += list(sp.tab) + list(pts.ravel())
    data = tmp_path / "tables.bin"
    np.asarray(words, dtype=np.float64).tofile(data)
    exe = tmp_path / "spline_paths_test"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", "-ffp-contract=off", "-I", str(ROOT / "optrace_amd" / "csrc"),
           str(ROOT / "tests" / "cpp" / "spline_paths_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=120)
    with capsys.disabled():
        print("\n" + r.stdout[-4000:])
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.rstrip().endswith("ok 3 tables")


@functools.lru_cache(maxsize=None)
def restated(sn: str, fam: str, mistake: str = None) -> dict:
    """fast_form on a class -> the class's check and the worst normal error over its bar."""
    sp = sc.spline(ot, sn)
    inp, ex, _ = sc.case(ot, sn, fam)
    ff = sc.fast_form(sp, inp["p0"], inp["s0"], mistake)
    res = sc.check(sp, fam, inp, ex, ff["point"], ff["hit"])
    h = ff["hit"]
    res["normal"] = sc.normal_ratio(sp, ff["point"][h, 0], ff["point"][h, 1], ff["normal"][h])
    res["ill"], res["cached"], res["hits"] = int(ff["ill"].sum()), int(ff["cached"].sum()), int(h.sum())
    return res


def holds(res: dict) -> bool:
    return sc.passes(res) and res["normal"] <= 1


@pytest.mark.parametrize("sn", list(sc.PLAN))
def test_fast_form_meets_every_bar(sn, capsys):
    """The float64 restatement of the trace kernel's path: hit points, verdicts, the tight z bar of `parallel` (the last
    Illinois iterate of a linear f lands on the root to rounding: the bar holds in float64, so the device is held to it),
    and the normals from the patch cache with their fallbacks."""
    sp = sc.spline(ot, sn)
    lines, bad = [f"{sn}: delta = {sp.delta:.2e} mm = {sp.delta / sp.h:.1e} h"], []
    for fam in sc.PLAN[sn]:
        res = restated(sn, fam)
        lines.append(sc.report("fast_form", sc.key(sn, fam), res).replace("   <-- FAILS", "")
                     + f", normals {res['normal']:.3f} of their bar ({res['cached']} of {res['hits']} from the patch)" + ("" if holds(res) else "   <-- FAILS"))
        assert res["ill"] == 0
        if not holds(res):
            bad.append(fam)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, bad


@pytest.mark.parametrize("sn", list(sc.PLAN))
def test_truth_agrees_with_scipy(sn):
    """The longdouble de Boor sums against SciPy's own evaluation of the same tck, values and first derivatives, to 1e-13."""
    sp, sf = sc.spline(ot, sn), sc.placed(ot, sn)
    rng = np.random.default_rng(5)
    x, y = rng.uniform(sp.lo, sp.hi, 400), rng.uniform(sp.lo, sp.hi, 400)
    if sp.one_d:
        S, dS, _, _ = sp.eval1(np.abs(x).astype(LD))
        assert np.max(np.abs(S - sf._interp(np.abs(x)))) <= 1e-13 and np.max(np.abs(dS - sf._interp(np.abs(x), nu=1))) <= 1e-13
        return
    S, Sx, Sy, _, _, _ = sp.eval2(x.astype(LD), y.astype(LD))
    assert np.max(np.abs(S - sf._interp(x, y, grid=False))) <= 1e-13
    assert np.max(np.abs(Sx - sf._interp(x, y, dx=1, grid=False))) <= 1e-13
    assert np.max(np.abs(Sy - sf._interp(x, y, dy=1, grid=False))) <= 1e-13


def _de_boor(mp, t, c, k, x, i):
    """de Boor's triangular scheme on cell i (mpf): the spline sum_j c[j] B_{j,k}(x), c[j] for j = i - k .. i given as a list."""
    d = list(c)
    for r in range(1, k + 1):
        for j in range(k, r - 1, -1):
            a = (x - t[j + i - k]) / (t[j + 1 + i - r] - t[j + i - k])
            d[j] = (1 - a) * d[j - 1] + a * d[j]
    return d[k]


def _mp_spline(mp, t, c, k, x, i, nu):
    """Value (nu = 0) or first derivative (nu = 1: the spline of degree k - 1 on the differenced coefficients) on cell i."""
    cs = [c[j] for j in range(i - k, i + 1)]
    if nu == 0:
        return _de_boor(mp, t, cs, k, x, i)
    dc = [k * (cs[j + 1] - cs[j]) / (t[i - k + j + 1 + k] - t[i - k + j + 1]) for j in range(k)]
    return _de_boor(mp, t, dc, k - 1, x, i)


@pytest.mark.parametrize("sn", list(sc.PLAN))
def test_truth_agrees_with_mpmath(sn):
    """64 points per surface (knots, seam and end cells among them) at 400 bits, by de Boor's triangular scheme on the
    coefficients -- another algorithm than the truth's basis functions: values and derivatives to 2^-60 of their condition
    sums A0, Ax, Ay (the spline itself passes through zero)."""
    mp = sc._mp()
    f = mp.mpf
    sp = sc.spline(ot, sn)
    pts = _points(sp, np.random.default_rng(7))
    pts = pts[np.random.default_rng(8).permutation(pts.shape[0])[:64]]
    t = [f(float(v)) for v in sp.t]
    tol = f(2) ** -60
    for x, y in pts:
        if sp.one_d:
            S, dS, A0, A1 = (v[0] for v in sp.eval1(np.array([x], dtype=LD)))
            i = int(sp.cell(np.array([x]))[0])
            c = [f(float(v)) for v in sp.c]
            for nu, got, cond in ((0, S, A0), (1, dS, A1)):
                want = _mp_spline(mp, t, c, SK, f(float(x)), i, nu)
                hi = np.float64(got)
                assert abs(f(float(hi)) + f(float(got - hi)) - want) <= tol * f(float(cond)), (sn, x, nu)
            continue
        S, Sx, Sy, A0, Ax, Ay = (v[0] for v in sp.eval2(np.array([x], dtype=LD), np.array([y], dtype=LD)))
        xc, yc = min(max(x, sp.lo), sp.hi), min(max(y, sp.lo), sp.hi)
        ix, iy = int(sp.cell(np.array([xc]))[0]), int(sp.cell(np.array([yc]))[0])
        for nux, nuy, got, cond in ((0, 0, S, A0), (1, 0, Sx, Ax), (0, 1, Sy, Ay)):
            rows = {a: _mp_spline(mp, t, {b: f(float(sp.c[a, b])) for b in range(iy - SK, iy + 1)}, SK, f(float(yc)), iy, nuy)
                    for a in range(ix - SK, ix + 1)}
            want = _mp_spline(mp, t, rows, SK, f(float(xc)), ix, nux)
            hi = np.float64(got)
            assert abs(f(float(hi)) + f(float(got - hi)) - want) <= tol * f(float(cond)), (sn, x, y, nux, nuy)


@pytest.mark.parametrize("sn", list(sc.PLAN))
def test_classes_meet_their_preconditions(sn):
    sp = sc.spline(ot, sn)
    d = sc.SURFACES[sn]
    assert sp.delta <= 1e-9 * sp.h and sp.cells[1] - sp.cells[0] >= 4
    # both parts of the knot array lie inside the aperture
    assert sp.t[sp.cells[0]] > -sp.r and sp.t[sp.cells[1] + 1] < sp.r
    for fam in sc.PLAN[sn]:
        inp, ex, info = sc.case(ot, sn, fam)
        k = sc.key(sn, fam)
        live = inp["w0"] > 0
        assert np.count_nonzero(~live) == len(range(3, sc.N_RAYS, 8)) and not np.any(ex["behind"])
        if fam not in ("rim", "end", "parallel"):
            assert np.all(np.abs(ex["delta"]) >= 1e-6), f"{k}: a verdict within 1e-6 of the edge of the mask"
        if fam not in ("miss", "rim"):
            assert np.count_nonzero(ex["hit"] & live) >= 0.8 * np.count_nonzero(live), k
        if fam == "miss":
            assert not np.any(ex["hit"])
        if fam == "hop":
            assert np.all(info.patches >= 3), k
        if fam == "stay":
            assert np.all(info.patches == 1), k
            assert restated(sn, fam)["cached"] == restated(sn, fam)["hits"] or sp.deriv_unrot, f"{k}: the gradient comes from the one patch"
        if fam == "seam":
            assert info.table_side >= 20 and info.arith_side >= 20, (k, info.table_side, info.arith_side)
        if fam in ("knot", "parallel"):
            assert info.on_knot >= 8, (k, info.on_knot)
        if fam == "knot":
            assert sc.checksum(sc.inputs(sp, sn, fam)) == sc.checksum(inp), f"{k}: the generator gives other bits the second time"
        if fam == "parallel":
            assert np.all(inp["s0"] == [0.0, 0.0, 1.0])
    if d["kind"] == "func2d":
        assert sp.deriv_unrot and sp.rot
    if d.get("flip"):
        assert sp.sgn == -1.0


def test_planted_mistakes_are_caught():
    """Three altered copies of fast_form, each failing a named class: the cell index from round (the neighbouring polynomial,
    continued: off by the jump of the fourth derivative, far below the 1e-7 of a hit point but not below the value bar of
    `parallel` or the normal bar), the gradient from the patch of the cell before a hop, the derivatives' arguments rotated
    although deriv_unrot is set."""
    assert holds(restated("d2_50", "parallel")) and holds(restated("d2_50", "wide")) and holds(restated("d2_50", "hop"))
    assert holds(restated("f2_rot", "wide"))
    wrong = restated("d2_50", "parallel", "round")
    assert wrong["zratio"] > 1, wrong
    assert restated("d2_50", "wide", "round")["normal"] > 1
    assert restated("d2_50", "hop", "stale_grad")["normal"] > 1e6
    assert restated("d1_50", "hop", "stale_grad")["normal"] > 1e6
    assert restated("f2_rot", "wide", "rotate_unrot")["normal"] > 1e6
    # the mistakes are specific: a surface without the flag is untouched by the third
    assert holds(restated("d2_rot_flip", "wide", "rotate_unrot"))
