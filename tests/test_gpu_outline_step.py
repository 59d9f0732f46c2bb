"""Rays that miss an element in the trace kernel (the miss rules of trace_ray, outline_clip and the rare-event counters of
csrc/ot_trace.hpp), one element per launch in a tight box (tests/outline_cases.py, tests/golden/wavelength_step.npz).

Pinned to the C oracle's bits, which tests/test_outline_host.py pins to the reference's: every section's point and weight,
the direction left in s0_list, the polarisation and the whole counter table, row by row.  All surfaces of the plain scenes
are flat and the clip is plain IEEE arithmetic, so nothing here has a tolerance.  The rules a missed ray obeys are asserted
in words as well (outline_cases.rule_violations), so that a failure names the rule.

The variants run the same rays through other instances of the kernel: without polarisation, with a surface of the general
record (OT_HOT_OTHER), a numeric-hit asphere or a spline surface behind the tested element, and with a tabulated filter
behind it (the table kernel).  What stands behind must leave the tested element's sections and counter columns alone;
where it is flat the whole trace is the oracle's.  One launch per scene generates its rays and runs render-only: its
counters and the records of its living rays are the stored form's.
"""
import functools

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd.ray_storage import TailStorage

import outline_cases as oc

pytestmark = pytest.mark.gpu

bits = oc.bits
FLAT_BEHIND = ("plain", "no_pol", "data_behind")   # every surface flat: the whole trace is bitwise the oracle's


class Run:
    """One launch: the device's storage (host copies) and the oracle's for the same compiled scene and rays."""


@functools.lru_cache(maxsize=None)
def run(name: str, variant: str) -> Run:
    inp = oc.inputs(name)
    n = inp["s0"].shape[0]
    r = Run()
    with ot.global_options.no_warnings():
        RT = oc.raytracer(ot, name, variant)
        pol0 = None if RT.no_pol else inp["pol0"]
        RT.trace(n, _initial_rays=(inp["p0"], inp["s0"], pol0, inp["w0"], inp["wl"]), _N_list=np.array([n]))
        assert not RT.geometry_error
        r.p, r.w, r.s = RT.rays.p_list.copy(), RT.rays.w_list.copy(), RT.rays.s0_list.copy()
        r.pol = None if RT.no_pol else RT.rays.pol_list.copy()
        r.msgs = np.array(RT._msgs)
        r.orc, r.orc_msgs, _ = oc.oracle_trace(RT, inp)
    r.inp, r.n, r.nt = inp, n, r.w.shape[1]
    return r


@pytest.mark.parametrize("variant", oc.VARIANTS)
@pytest.mark.parametrize("name", oc.SCENES)
def test_points_weights_and_counters_are_the_oracles(name, variant):
    r = run(name, variant)
    assert r.n % 64 != 0
    ns = 1 + oc.n_tested(name)            # sections 0 .. ns - 1 belong to the tested element
    upto = r.nt if variant in FLAT_BEHIND else ns
    for i in range(upto):
        assert bits(r.p[:, i], r.orc.p_list[:, i]), f"p of section {i}"
        assert bits(r.w[:, i], np.ascontiguousarray(r.orc.w_list[:, i])), f"w of section {i}"
        if r.pol is not None:
            assert bits(r.pol[:, i], r.orc.pol_list[:, i]), f"pol of section {i}"
    # the counter table, row by row: a step's events are complete in the columns up to its own; ABSORB_MISSING of the
    # tested element's last step stands one column further
    for row, cols in ((oc.OUTLINE_INTERSECTION, upto if upto == r.nt else ns - 1), (oc.ABSORB_MISSING, upto), (oc.TIR, upto if upto == r.nt else ns - 1),
                      (oc.ILL_COND, upto), (oc.HURB_NEG_DIR, upto)):
        assert np.array_equal(r.msgs[row, :cols], r.orc_msgs[row, :cols]), f"counter row {row}\n{r.msgs}\n{r.orc_msgs}"
    clipped = int(np.count_nonzero(oc.expected(name, r.inp)["clip"]))
    assert int(r.msgs[oc.OUTLINE_INTERSECTION, 0]) == clipped >= 500, "the clipped rays of the classes"
    if variant in FLAT_BEHIND:
        assert np.array_equal(r.msgs, r.orc_msgs), f"\n{r.msgs}\n{r.orc_msgs}"
        assert bits(r.s, r.orc.s_final), "s0_list"
    else:   # a ray that was dead behind the tested element has its direction from there
        gone = r.w[:, ns - 1] == 0
        assert bits(r.s[gone], r.orc.s_final[gone])
    if variant != "plain":   # what stands behind the element leaves its sections alone
        base = run(name, "plain")
        assert bits(r.p[:, :ns], base.p[:, :ns])
        if variant != "no_pol" or name != "lens":   # (without polarisation the plate transmits T(1/2, 1/2))
            assert bits(r.w[:, :ns], base.w[:, :ns])
        if r.pol is not None:
            assert bits(r.pol[:, :ns], base.pol[:, :ns])


@pytest.mark.parametrize("variant", oc.VARIANTS)
@pytest.mark.parametrize("name", oc.SCENES)
def test_rules_of_a_missed_ray_in_words(name, variant):
    r = run(name, variant)
    bad = oc.rule_violations(name, r.inp, r.p, r.w, r.msgs, r.pol)
    assert not bad, "\n".join(bad)


def test_mixed_block_counts_like_blocks_of_its_own():
    """The device counts a step's rare events behind one wave-wide test.  The block in which hits, kept misses, killed misses,
    clipped and dead rays alternate lane by lane, traced alone, gives the counters the oracle gives for those 64 rays, and the
    blocks of pure hits around it add nothing to the columns of the tested element."""
    for name in oc.SCENES:
        inp = oc.inputs(name)
        with ot.global_options.no_warnings():
            RT = oc.raytracer(ot, name)
            for lo, hi in ((64, 128), (0, 64), (0, 192)):
                sub = {k: np.ascontiguousarray(v[lo:hi]) for k, v in inp.items()}
                RT.trace(hi - lo, _initial_rays=(sub["p0"], sub["s0"], sub["pol0"], sub["w0"], sub["wl"]), _N_list=np.array([hi - lo]))
                msgs = np.array(RT._msgs)
                _, orc_msgs, _ = oc.oracle_trace(RT, sub)
                assert np.array_equal(msgs, orc_msgs), f"{name} rays {lo}:{hi}\n{msgs}\n{orc_msgs}"
                if (lo, hi) == (0, 64):
                    assert not msgs[:, :oc.n_tested(name)].any() and not msgs[oc.ABSORB_MISSING, :1 + oc.n_tested(name)].any(), name
                else:
                    assert msgs[oc.OUTLINE_INTERSECTION, 0] == 16, name


def tail_records(tail):
    """(n, 7) records of the living rays of a render-only trace: p[nt - 2], p[nt - 1], w."""
    cap, n = tail._cap, tail.N
    p = tail._dev["p"].view(3, 2, cap)[:, :, :n].cpu().numpy()
    tw = tail._dev["w"].view(2, cap)[:, :n].cpu().numpy()
    live = tw[0] > 0
    assert not tw[1].any() and int(live.sum()) == tail.alive
    return np.concatenate([p[:, 0, live].T, p[:, 1, live].T, tw[0, live, None].astype(np.float64)], axis=1)


@pytest.mark.parametrize("name", oc.SCENES)
def test_render_only_launch_counts_and_ends_like_the_stored_one(name):
    """Rays generated on the device (a wide cone inside the box: hits, misses inside, every x and y wall): the stored form
    against the oracle on the rays it stored in section 0, the render-only form against the stored one."""
    N, seed = 3001, 11
    with ot.global_options.no_warnings():
        RT = oc.raytracer(ot, name, seed=seed)
        RT.trace(N)
        p, w, pol, s, wl, msgs = (RT.rays.p_list.copy(), RT.rays.w_list.copy(), RT.rays.pol_list.copy(), RT.rays.s0_list.copy(),
                                  RT.rays.wl_list.copy(), np.array(RT._msgs))
        nt = w.shape[1]
        tail = TailStorage()
        RT.trace(N, _tail=tail)
        tail_msgs = np.array(RT._msgs)
        recs = tail_records(tail)
        # the oracle on the stored start: the directions of the rays are not stored (s0_list holds the final ones), so the
        # rays enter it one section late wherever the first step leaves the direction alone
        RI = oc.raytracer(ot, name)
    assert msgs[oc.OUTLINE_INTERSECTION, 0] >= 500 and msgs[oc.OUTLINE_INTERSECTION, nt - 2] + (w[:, nt - 2] > 0).sum() >= 20
    assert np.array_equal(tail_msgs, msgs), f"\n{tail_msgs}\n{msgs}"
    sel = w[:, nt - 2] > 0
    ref = np.concatenate([p[sel, nt - 2], p[sel, nt - 1], w[sel, nt - 2, None].astype(np.float64)], axis=1)
    order = lambda a: a[np.lexsort(a.T[::-1])]
    assert tail.traced == N and bits(order(recs), order(ref)), "render-only records differ from the stored sections"
    # every ray the first step clipped or left beside the element still has its direction: replay those through the oracle
    live = w[:, 0] > 0
    straight = live & np.all(np.abs(np.cross(p[:, 1] - p[:, 0], s)) <= 1e-12, axis=1) & (np.linalg.norm(p[:, 1] - p[:, 0], axis=1) > 0)
    straight &= (w[:, 1] == 0) | (w[:, 1] == w[:, 0])
    assert np.count_nonzero(straight) >= 500
    sub = dict(p0=np.ascontiguousarray(p[straight, 0]), s0=np.ascontiguousarray(s[straight]), pol0=np.ascontiguousarray(pol[straight, 0]),
               w0=np.ascontiguousarray(w[straight, 0]), wl=np.ascontiguousarray(wl[straight]))
    with ot.global_options.no_warnings():
        orc, _, _ = oc.oracle_trace(RI, sub)
    for i in range(nt):
        assert bits(np.ascontiguousarray(p[straight, i]), np.ascontiguousarray(orc.p_list[:, i])), f"section {i}"
        assert bits(np.ascontiguousarray(w[straight, i]), np.ascontiguousarray(orc.w_list[:, i])), f"section {i}"
