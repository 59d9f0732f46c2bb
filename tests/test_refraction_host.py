"""The refraction step on the host: the fixture tests/golden/refraction_step.npz (the reference's own results and the
exact values of its formulas, tests/golden/generate_golden_refraction.py) against the inputs that refraction_cases
regenerates, the C oracle against the reference's bits, and the bars of tests/test_gpu_refraction_step.py against two
float64 restatements, so that they are known to bite.  CPU only."""
import numpy as np
import pytest

import optrace_amd as ot

import refraction_cases as rc
from helpers import load

SCENES = rc.scenes()
NAMES = [sc.name for sc in SCENES]
TIR, MISSING = 1, 0   # Raytracer.INFOS


@pytest.fixture(scope="module")
def g():
    return load("refraction_step.npz")


def bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_fixture_belongs_to_the_regenerated_inputs(g, name):
    sc = rc.scene(name)
    inp = rc.inputs(sc)
    n = inp["s0"].shape[0]
    assert str(g[f"{name}/checksum"]) == rc.checksum(inp)
    assert n % 64 != 0 and np.count_nonzero(inp["w0"] == 0) == len(range(3, n, 8))
    for key, shape in (("w1", (n,)), ("pol1", (n, 3)), ("s1", (n, 3)), ("s_out", (n, 3)), ("tir", (n,)), ("T_hi", (n,)),
                       ("T_lo", (n,)), ("pol_hi", (n, 3)), ("pol_lo", (n, 3))):
        assert g[f"{name}/{key}"].shape == shape, key
    assert bits(g[f"{name}/normal"], rc.unit_normal(sc.normal)), "np.linalg.norm rounds the tilted normal differently here"
    # pol0 is float32 and perpendicular to s0 to float32 rounding, not better
    dot = np.abs(np.sum(inp["s0"] * inp["pol0"].astype(np.float64), axis=1))
    assert dot.max() < 2.0 ** -23 and (sc.classes == ("parallel", "critical") or dot.max() > 2.0 ** -30)
    if "critical" in sc.classes:
        sel = (inp["cls"] == sc.classes.index("critical")) & (inp["w0"] > 0)
        assert np.count_nonzero(g[f"{name}/tir"][sel]) >= 50 and np.count_nonzero(g[f"{name}/w1"][sel] > 0) >= 50
    if name == "flat/1.5_1":   # the one ray with W == 0 exactly: no power, not a total reflection
        sel = (inp["w0"] > 0) & ~g[f"{name}/tir"] & (g[f"{name}/w1"] == 0)
        assert np.count_nonzero(sel) == 1 and np.all(np.isfinite(g[f"{name}/s1"][sel]))


@pytest.mark.parametrize("name", NAMES)
def test_oracle_has_the_references_bits(g, name):
    """The float64 yardstick of the GPU test: s' (through the direction behind the element), w', pol', the
    total-reflection verdicts and the counters of the C oracle are the reference's, bit for bit."""
    sc = rc.scene(name)
    inp = rc.inputs(sc)
    with ot.global_options.no_warnings():
        RT = rc.raytracer(ot, sc)
        RT._geometry_checks()
        assert not RT.geometry_error
        rays, msgs, csc = rc.oracle_trace(RT, inp)
    live = inp["w0"] > 0
    assert msgs[MISSING, 1] == 0, "every live ray meets the tested surface"
    assert msgs[TIR, 0] == int(g[f"{name}/tir_count"])
    assert bits(rays.w_list[:, 1], g[f"{name}/w1"])
    assert bits(rays.pol_list[:, 1], g[f"{name}/pol1"])
    assert np.all(g[f"{name}/w1"][g[f"{name}/tir"]] == 0)
    through = rays.w_list[:, -2] > 0   # met every face with power left
    assert np.count_nonzero(through) >= 19
    assert bits(rays.s_final[through], g[f"{name}/s_out"][through])
    if sc.D is not None:
        assert bits(g[f"{name}/s1"], g[f"{name}/s_out"]) and np.array_equal(through, live)
        centre = live & (inp["cls"] == 0) & (np.arange(live.shape[0]) < rc.IDEAL_CENTRE)
        assert bits(rays.s_final[centre], inp["s0"][centre]) and bits(rays.pol_list[centre, 1], inp["pol0"][centre])
    # dead rays stay where and what they are
    assert np.all(rays.p_list[~live] == inp["p0"][~live, None, :]) and np.all(rays.w_list[~live] == 0)
    assert all(bits(rays.pol_list[~live, i], inp["pol0"][~live]) for i in range(csc.nt))
    # the restatement that the error table below uses is the reference's arithmetic too
    if sc.D is None:
        re = rc.reference_step(g[f"{name}/normal"], inp["s0"], inp["pol0"], sc.n1, sc.n2)
        assert bits(re["s_"][live], g[f"{name}/s1"][live])
        assert bits((inp["w0"] * re["T"]).astype(np.float32)[live], g[f"{name}/w1"][live])
        assert bits(re["pol_"].astype(np.float32)[live], g[f"{name}/pol1"][live])


def test_exact_values_are_reproduced_by_mpmath(g):
    pytest.importorskip("mpmath")
    checked = 0
    for sc in SCENES:
        inp = rc.inputs(sc)
        k = sc.name
        if sc.D is not None:
            with ot.global_options.no_warnings():
                rays, _, _ = rc.oracle_trace(rc.raytracer(ot, sc), inp)
        for r in range(0, inp["s0"].shape[0], 8):
            if inp["w0"][r] == 0 or g[f"{k}/tir"][r]:
                assert np.isnan(g[f"{k}/pol_hi"][r, 0])
                continue
            if sc.D is None:
                ex = rc.exact_step(g[f"{k}/normal"], inp["s0"][r], inp["pol0"][r], sc.n1, sc.n2)
                if ex is None:
                    assert np.isnan(g[f"{k}/T_hi"][r]) and np.isnan(g[f"{k}/pol_hi"][r, 0])
                    continue
                assert rc.split(ex[0]) == (g[f"{k}/T_hi"][r], g[f"{k}/T_lo"][r])
                assert all(rc.split(ex[1][c]) == (g[f"{k}/pol_hi"][r, c], g[f"{k}/pol_lo"][r, c]) for c in range(3))
            else:   # the hit point is the oracle's here (the reference's to a rounding): 2^-52 / |s' x s| <= 2^-36
                ex = rc.exact_ideal(sc.D, (0.0, 0.0, 0.0), rays.p_list[r, 1], inp["s0"][r], inp["pol0"][r])
                if ex is None:
                    assert np.isnan(g[f"{k}/pol_hi"][r, 0])
                    continue
                assert all(abs(float(ex[c]) - g[f"{k}/pol_hi"][r, c]) <= 2.0 ** -36 for c in range(3))
            checked += 1
    assert checked > 800


def reference_rows(g, sc, inp, form):
    """Rows of rc.against_exact for a float64 restatement of the step, rounded to float32 the way the store does."""
    res = form(g[f"{sc.name}/normal"], inp["s0"], inp["pol0"], sc.n1, sc.n2)
    with np.errstate(all="ignore"):
        w1 = (inp["w0"] * res["T"]).astype(np.float32)
    return rc.against_exact(sc, inp, g, w1, res["pol_"].astype(np.float32)), res


def test_bars_bite_and_the_references_own_error(g, capsys):
    """Prints the reference's own error per class (DESIGN.md section 4 takes its table from here; no bar contains it) and
    shows that the bars are not vacuous: the plane-of-incidence form without a near-normal branch breaks them at
    sin(alpha) ~ 2^-40 on a tilted normal, the same form with the branch keeps them in every class."""
    lines = ["scene          class      | reference, f64: T rel, pol abs | stored: w, pol in bars | n x s form | with the branch"]
    fails = {"ref": {}, "plain": {}, "guarded": {}}
    forms = {"ref": rc.reference_step, "plain": rc.incidence_plane_form,
             "guarded": lambda *a: rc.incidence_plane_form(*a, guard=2.0 ** -54)}
    for sc in SCENES:
        if sc.D is not None or sc.n1 == sc.n2:
            continue
        inp = rc.inputs(sc)
        rows = {}
        for key, form in forms.items():
            rows[key], res = reference_rows(g, sc, inp, form)
            fails[key][sc.name] = [r["cls"] for r in rows[key] if not rc.row_passes(r)]
            if key == "ref":
                ref64 = res
        for j, row in enumerate(rows["ref"]):   # the reference before its float32 store
            sel = (inp["cls"] == sc.classes.index(row["cls"])) & (inp["w0"] > 0) & np.isfinite(g[f"{sc.name}/T_hi"])
            T = rc.join(g[f"{sc.name}/T_hi"][sel], g[f"{sc.name}/T_lo"][sel])
            pol = rc.join(g[f"{sc.name}/pol_hi"][sel], g[f"{sc.name}/pol_lo"][sel])
            cell = lambda r: f"{r['w_over']:9.2e} {r['pol_over']:9.2e}"
            lines.append(f"{sc.name:14s} {row['cls']:10s} | {float(np.max(np.abs(ref64['T'][sel] - T) / T)):.2e} "
                         f"{float(np.max(np.abs(ref64['pol_'][sel] - pol))):.2e} | {cell(row)} | {cell(rows['plain'][j])} | "
                         f"{cell(rows['guarded'][j])}")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert all(v == [] for v in fails["guarded"].values()), fails["guarded"]
    plain = fails["plain"]
    assert {"small-40", "small-48"} <= set(plain["tilt_a/1_1.5"]) and "small-40" in plain["tilt_b/up"]
    assert "small-40" in plain["tilt_a/down"] and "small-40" in plain["tilt_b/1.7_1"] and "small-40" in plain["tilt_a/1_2.5"]
    assert plain["flat/1_1.5"] == [], "the flat normal's cross product is exact"
    assert not any(c in ("wide", "small-10", "small-20", "small-24") for v in plain.values() for c in v)
    # the reference: sound at ordinary angles everywhere and on the flat normal, lost at small angles on a tilted one
    assert fails["ref"]["flat/1_1.5"] == [] and not any("wide" in v for v in fails["ref"].values())
    assert "small-48" in fails["ref"]["tilt_a/1_1.5"] and "small-30" in fails["ref"]["tilt_b/up"]


def test_where_the_reference_divides_zero_by_zero(g):
    """s' differs from s by a rounding while s' x s is exactly zero: normalize gives 0 / 0 and the reference's weight is
    NaN (the ray is dead from there on).  It happens for a beam along a tilted normal and at nearly matched indices below
    sin(alpha) ~ 2^-36; the GPU test holds the product to the exact value (or, for m == 0, to the unchanged-direction
    contract) in exactly these places and to the oracle everywhere else."""
    found = {}
    for sc in SCENES:
        inp = rc.inputs(sc)
        nan = np.isnan(g[f"{sc.name}/w1"])
        assert not np.any(nan & (inp["w0"] == 0))
        for ci, cls in enumerate(sc.classes):
            if np.any(nan & (inp["cls"] == ci)):
                found[f"{sc.name} {cls}"] = int(np.count_nonzero(nan & (inp["cls"] == ci)))
    assert set(found) == {"tilt_a/1_1.5 parallel", "tilt_a/down small-36", "tilt_a/down small-40", "tilt_a/down small-48"}, found
    assert found["tilt_a/1_1.5 parallel"] == len([i for i in range(rc.N_PARALLEL) if (128 + i) % 8 != 3])
