"""The refraction step of the trace kernel (refract, refraction_polarization, same_medium_polarization, fresnel_T2,
refract_ideal / compute_polarization of csrc/ot_trace.hpp) at its edges, one plate or ideal lens per launch
(tests/refraction_cases.py, tests/golden/refraction_step.npz).

What it is pinned to:
  * the C oracle's bits (which tests/test_refraction_host.py pins to the reference's) for everything discrete -- counters,
    alive masks, total-reflection verdicts -- for the direction behind the plate, for pol' at N == 1, and to one float32
    unit in the last place for the weights at N == 1, of a beam along the normal and around the critical angle;
  * the EXACT value of the reference's formulas (mpmath, stored as hi + lo) for every other weight and polarisation, per
    ray, with u = 2^-53 and a = sin(alpha) = |n x s| (ideal lens: |s' x s|) taken from the inputs in longdouble:
        |w_dev - w0 T|      <= w0 T (2^-24 + 2^-30 + min(2^-24, 2^-49 / a))
        |pol_dev - pol|     <= 2^-25 + 2^-30 + min(2^-25, 2^-49 / a)         per component
    2^-24, 2^-25: the float32 store.  2^-30: ~30 double operations at the worst conditioning of the classes (W >= 2^-8,
    |s' x s| >= 2^-16).  2^-49 / a: 16 times the rounding bound u / a of a basis built from n x s.  The cap: below
    a ~ 2^-25 an answer exact to a^2 exists without any basis, so a kernel must not use the noisy one.
    The reference's own error is in no bar (test_refraction_host.py prints it): at nearly matched indices and small
    angles the reference is wrong by up to 0.9 in T and returns NaN below sin(alpha) ~ 2^-36; the product is held to the
    exact value there, and its rays stay alive where the reference's weight is NaN.
  * A beam along the normal (m == 0) is held to the reference's contract for an unchanged direction, A_ts^2 = A_tp^2 =
    1/2 and pol' = pol: the weight within one float32 unit of w0 T(1/2, 1/2), T in longdouble.  On the flat normal the
    reference's s' equals s bitwise, it takes that branch itself, and the oracle's weight is the yardstick as well.  On a
    tilted normal s' differs from s by a rounding and the reference builds its basis from s' x s, which is noise there:
    it loses up to 2e-3 of the weight or divides 0 by 0 (printed below; MI355X: 2.1e-3 for n1 = 1.7 -> 1 on the normal
    (0.3, -0.2, 0.9), NaN for 1 -> 1.5).  The oracle cannot be the yardstick in that place --
    test_gpu_edges::test_beam_along_a_face_normal_keeps_its_power fixes the normal-incidence value as the product's.

Variants run the same rays through other template instances of the kernel (tabulated medium, a numeric-hit or a
spline-surface lens behind the plate, no_pol); the elements behind must leave sections 0 .. 2 alone.
"""
import functools

import numpy as np
import pytest

import optrace_amd as ot

import refraction_cases as rc
from helpers import load

pytestmark = pytest.mark.gpu

SCENES = rc.scenes()
TIR, MISSING = 1, 0   # Raytracer.INFOS
STRAIGHT = ("plain", "data_medium", "no_pol")   # nothing behind the plate: s0_list is the direction behind its back face


@pytest.fixture(scope="module")
def g():
    return load("refraction_step.npz")


def bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Run:
    """One launch: the device's storage (host copies) and the oracle's for the same compiled scene and rays."""


@functools.lru_cache(maxsize=None)
def run(name: str, variant: str) -> Run:
    sc = rc.scene(name)
    inp = rc.inputs(sc)
    n = inp["s0"].shape[0]
    r = Run()
    with ot.global_options.no_warnings():
        RT = rc.raytracer(ot, sc, variant)
        pol0 = None if RT.no_pol else inp["pol0"]
        RT.trace(n, _initial_rays=(inp["p0"], inp["s0"], pol0, inp["w0"], inp["wl"]), _N_list=np.array([n]))
        assert not RT.geometry_error
        r.p, r.w, r.s = RT.rays.p_list.copy(), RT.rays.w_list.copy(), RT.rays.s0_list.copy()
        r.pol = None if RT.no_pol else RT.rays.pol_list.copy()
        if RT.no_pol:
            assert np.all(np.isnan(RT.rays.pol_list))
        r.msgs = np.array(RT._msgs)
        r.orc, r.orc_msgs, _ = rc.oracle_trace(RT, inp)
    r.sc, r.inp, r.live, r.n = sc, inp, inp["w0"] > 0, n
    r.lost = r.live & np.isnan(r.orc.w_list[:, 1])   # the reference's 0 / 0: s' x s == 0 although s' != s
    return r


def runs(variant):
    """Every scene of the variant (the ideal lens has no medium to tabulate)."""
    return [run(sc.name, variant) for sc in SCENES if not (sc.D is not None and variant == "data_medium")]


def cls_mask(r, *prefixes):
    idx = [ci for ci, c in enumerate(r.sc.classes) if c.startswith(prefixes)]
    return np.isin(r.inp["cls"], idx)


def within_one_ulp(a, b) -> bool:
    both_nan = np.isnan(a) & np.isnan(b)
    ok = both_nan | (~np.isnan(a) & ~np.isnan(b))
    d = rc.ulp32_distance(np.where(both_nan, 0, a), np.where(both_nan, 0, b))
    return bool(np.all(ok) and np.all(d[ok] <= 1))


@pytest.mark.parametrize("variant", rc.VARIANTS)
def test_discrete_results_are_the_oracles(g, variant):
    for r in runs(variant):
        k = r.sc.name
        assert r.n % 64 != 0
        assert r.msgs[MISSING, 1] == 0, f"{k}: a live ray missed the tested surface"
        assert r.msgs[TIR, 0] == int(g[f"{k}/tir_count"]) == r.orc_msgs[TIR, 0], k
        assert np.array_equal(r.msgs[TIR], r.orc_msgs[TIR]), f"{k}\n{r.msgs}\n{r.orc_msgs}"
        # the reference's NaN weights: a beam along a tilted normal, and nearly matched indices below sin(alpha) = 2^-30
        near = cls_mask(r, "small-3", "small-4") if k.endswith(("/up", "/down")) else np.zeros(r.n, dtype=bool)
        assert np.all((near | cls_mask(r, "parallel"))[r.lost]) and not (np.any(r.lost) and r.sc.normal == "flat"), k
        if not np.any(r.lost) or variant == "no_pol":   # (rays that live on where the reference's died may be counted later)
            assert not np.any(r.lost) and np.array_equal(r.msgs, r.orc_msgs), f"{k}\n{r.msgs}\n{r.orc_msgs}"
        keep = ~r.lost
        assert np.array_equal(r.w[keep] > 0, r.orc.w_list[keep] > 0), f"{k}: alive masks"
        assert np.all(r.w[r.lost, 1] > 0), "where the reference divides 0 by 0 the product has the exact weight"
        assert np.array_equal(r.w[:, 1] == 0, r.orc.w_list[:, 1] == 0) and np.all(r.w[g[f"{k}/tir"], 1] == 0), k
        assert np.all(np.isfinite(r.w)) and np.all(np.isfinite(r.p))
        dead = ~r.live
        assert np.all(r.p[dead] == r.inp["p0"][dead, None, :]) and np.all(r.w[dead] == 0), f"{k}: dead rays moved"
        if r.pol is not None:
            assert all(bits(r.pol[dead, i], r.inp["pol0"][dead]) for i in range(r.pol.shape[1])), f"{k}: dead rays' pol"
        if variant != "plain":   # what stands behind the element, or how its index is stored, leaves its sections alone
            base, ns = run(k, "plain"), 3 if r.sc.D is None else 2
            assert bits(r.p[:, :ns], base.p[:, :ns]), k
            if variant != "no_pol":
                assert bits(r.w[:, :ns], base.w[:, :ns]) and bits(r.pol[:, :ns], base.pol[:, :ns]), k


@pytest.mark.parametrize("variant", STRAIGHT)
def test_direction_behind_the_plate_has_the_oracles_bits(g, variant):
    """Both normals are constant, so the final direction of a ray that passed both faces does not depend on hit points:
    s' in the reference's operation order gives the reference's bits (the hit masks downstream rest on that)."""
    for r in runs(variant):
        through = r.orc.w_list[:, -2] > 0
        if r.sc.D is None:
            assert np.count_nonzero(through) >= 19
            for cls in r.sc.classes:
                sel = through & cls_mask(r, cls)
                assert bits(r.s[sel], r.orc.s_final[sel]), f"{r.sc.name} {cls}"
                if variant != "no_pol":   # (the archive's second refraction ran on the rays its first left with power)
                    assert bits(r.s[sel], g[f"{r.sc.name}/s_out"][sel]), f"{r.sc.name} {cls}: the reference's own"
        else:
            # The hit point enters: the rays through the centre keep their direction and with it their pol (the
            # unchanged-direction branch compares values), the others agree to rounding.  Not bitwise: for f < 0 the
            # reference gets -0 / |f| = -0, times sign(f) = +0, while the device's division core returns +0 for a zero
            # numerator of either sign and ends at -0.  No comparison or division downstream tells the two apart.
            centre = r.live & (np.arange(r.n) < rc.IDEAL_CENTRE)
            assert np.array_equal(r.s[centre], r.inp["s0"][centre])
            if r.pol is not None:
                assert bits(r.pol[centre, 1], r.inp["pol0"][centre])
            assert np.max(np.abs(r.s[r.live] - r.orc.s_final[r.live])) <= 2.0 ** -50


@pytest.mark.parametrize("variant", rc.VARIANTS)
def test_same_medium_has_the_oracles_bits(variant):
    """N == 1: pol' comes from the reference's basis of rounding noise in the reference's operation order."""
    seen = 0
    for r in runs(variant):
        if r.sc.D is not None or r.sc.n1 != r.sc.n2:
            continue
        seen += 1
        if r.pol is not None:
            assert bits(r.pol[:, 1], r.orc.pol_list[:, 1]), r.sc.name
            assert np.any(r.pol[r.live, 1] != r.inp["pol0"][r.live]), "some s' differ from s by a rounding"
        assert within_one_ulp(r.w[:, 1], r.orc.w_list[:, 1]), r.sc.name
    assert seen == 3


@pytest.mark.parametrize("variant", rc.VARIANTS)
def test_parallel_and_critical_weights_within_one_ulp(g, variant, capsys):
    zero_W, lines = 0, []
    for r in runs(variant):
        k = r.sc.name
        crit, par = cls_mask(r, "critical"), cls_mask(r, "parallel")
        assert within_one_ulp(r.w[crit, 1], r.orc.w_list[crit, 1]), k
        if np.any(par):
            # the unchanged-direction contract everywhere; the oracle too wherever the reference took that branch itself
            want = (r.inp["w0"][par] * rc.nopol_T(g[f"{k}/normal"], r.inp["s0"][par], r.sc.n1, r.sc.n2)).astype(np.float32)
            assert within_one_ulp(r.w[par, 1], want), k
            unchanged = par & np.all(g[f"{k}/s1"] == r.inp["s0"], axis=1)
            assert within_one_ulp(r.w[unchanged, 1], r.orc.w_list[unchanged, 1]), k
            assert r.sc.normal != "flat" or np.array_equal(unchanged, par)
            noisy = par & r.live & ~unchanged
            if np.any(noisy) and variant == "plain":
                with np.errstate(all="ignore"):
                    off = np.abs(r.orc.w_list[noisy, 1].astype(np.float64) / r.w[noisy, 1] - 1)
                lines.append(f"{k:14s} beam along the normal: the reference's weight is off by up to {np.max(off[~np.isnan(off)], initial=0.0):.1e}, "
                             f"NaN for {np.count_nonzero(np.isnan(off))} of {off.size} rays")
            if r.pol is not None and r.sc.n1 != r.sc.n2:   # m == 0: the direction may change by a rounding, pol does not
                assert bits(r.pol[par, 1], r.inp["pol0"][par]), k
        # W == 0 exactly: no power is left, but it is no total reflection and the direction stays finite
        z = crit & r.live & ~g[f"{k}/tir"] & (g[f"{k}/w1"] == 0)
        zero_W += np.count_nonzero(z)
        assert np.all(r.w[z, 1] == 0) and np.all(np.isfinite(r.s[z])) and np.all(np.isfinite(g[f"{k}/s1"][z]))
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert zero_W == 1


@pytest.mark.parametrize("variant", rc.VARIANTS)
def test_weights_and_polarisation_against_exact_values(g, variant, capsys):
    lines, bad = [], []
    for r in runs(variant):
        rows = rc.against_exact(r.sc, r.inp, g, r.w[:, 1], None if r.pol is None else r.pol[:, 1], s_out=r.orc.s_final,
                                no_pol=(variant == "no_pol"))
        lines.append(rc.format_rows(f"{variant} {r.sc.name}", rows))
        bad += [f"{r.sc.name} {row['cls']}" for row in rows if not rc.row_passes(row)]
    with capsys.disabled():
        print("\n" + "\n".join(l for l in lines if l))
    assert not bad, bad
