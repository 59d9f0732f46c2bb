"""The HURB step of the trace kernel (hurb_bend of csrc/ot_trace.hpp, hurb_props and philox_normal2 of csrc/ot_device.hpp)
ray by ray: one or two HURB apertures per launch, rays at the edges of the step (tests/hurb_cases.py: scenes, classes, the
longdouble restatement and the derivation of every bar; tests/test_hurb_host.py: the C oracle's own distance from the exact
value, which is what the margins rest on).

3a  injected normals (`_hurb_normals` = float64 of the replayed pairs), with and without polarisation.  Discrete results
    are the C oracle's: alive masks, who is bent, counters (HURB_NEG_DIR per section), untouched dead / blocked / on-edge
    rays.  The hit point against p0 + t s in longdouble; s' per component against `bend` evaluated from the stored hit
    point, inside u [8 + G_a (20 q_b + 4) + G_b (20 q_b + 7) + g_a E_a + g_b E_b]; pol' inside the refraction pin's
    2^-25 + 2^-30 + min(2^-25, 2^-49 / |s' x s|) plus L times the s' bar (hurb_cases.py) -- the EXACT value also where the bend is tiny and the reference's own
    projection form is noise (up to 2.7e-3 in the `tiny` class, test_hurb_host.py): below |s' x s| ~ 2^-25 pol' = pol - s (s'.pol)
    to |s' x s|^2 without any basis, so a kernel has no reason to be noisy there.  w' is w or 0, bit for bit.
3b  the device's own draws: the same launches without injected normals against `bend` at the longdouble pairs; the bar grows
    by 6 u r (|tan_sig_a| + |tan_sig_b|) / |v| alone.  Slots, the high word of the seed, the global ray index and the order
    (za, zb) each have a test that fails if the kernel gets them wrong.
3c  the production kernels (rays generated in the kernel, line and rectangle spectrum): against a second trace of the
    bitwise same rays with the replayed normals injected, and the render-only form against the stored one bit for bit.
3d  the verdict s'_z < 0 is open only within the direction bar of zero; the number of open rays per class is capped
    (hurb_cases.open_cap) and asserted in 3a and 3b.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd._device import stream_ptr
from optrace_amd.ray_storage import TailStorage

import hurb_cases as hc
import scenes
from hurb_cases import LD

pytestmark = pytest.mark.gpu

NAMES = [sc.name for sc in hc.SCENES]
HURB_NEG_DIR = 4   # Raytracer.INFOS


def bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


class Run:
    """One launch: host copies of the device's storage, the normals it was given (or the replay of those it drew), the
    oracle's storage for the injected ones, and `bend` evaluated from the device's own sections."""


def launch(sc, inp, no_pol, seed, nrm) -> Run:
    r = Run()
    n = inp["s0"].shape[0]
    with ot.global_options.no_warnings():
        RT = hc.raytracer(ot, sc, no_pol, seed)
        RT.trace(n, _initial_rays=(inp["p0"], inp["s0"], None if no_pol else inp["pol0"], inp["w0"], inp["wl"]),
                 _hurb_normals=nrm, _N_list=np.array([n]))
        assert not RT.geometry_error
        r.p, r.w, r.s = RT.rays.p_list.copy(), RT.rays.w_list.copy(), RT.rays.s0_list.copy()
        r.pol = None if no_pol else RT.rays.pol_list.copy()
        r.n_index = RT.rays.n_list[:, 0].copy()
        r.msgs = np.array(RT._msgs)
    r.RT, r.sc, r.inp, r.n, r.live = RT, sc, inp, n, inp["w0"] > 0
    return r


@functools.lru_cache(maxsize=None)
def run(name: str, no_pol: bool, drawn: bool, seed: int = hc.SEED) -> Run:
    sc = hc.scene(name)
    inp = hc.inputs(sc)
    with ot.global_options.no_warnings():
        plain, _ = hc.oracle_trace(hc.raytracer(ot, sc, no_pol, seed), inp, None)
    n_orc = plain.n_list[:, 0].copy()
    if drawn:
        r = launch(sc, inp, no_pol, seed, None)
        r.nrm, rr = hc.pairs(sc, r.n, seed)
    else:
        nrm, rr = hc.injected(sc, inp, seed, n_orc), None
        r = launch(sc, inp, no_pol, seed, nrm)
        r.nrm = nrm
        with ot.global_options.no_warnings():
            r.orc, r.orc_msgs = hc.oracle_trace(r.RT, inp, nrm)
    # the index in front of the aperture is an input of the step: the device's own, held to the oracle's (8 units in the last
    # place: the Abbe model's powers are repeated products on the device, within 3 of pow each)
    assert np.all(np.abs(r.n_index - n_orc) <= 8 * np.spacing(n_orc)), name
    r.res = hc.evaluate(sc, inp, r.p, r.pol, r.w, r.n_index, r.nrm, rr)
    return r


def check_against_exact(r: Run, title: str, lines: list) -> list:
    """Hit point, weights, s' and pol' of one launch against `bend`; -> the classes that leave a bar or a cap."""
    sc, inp, res = r.sc, r.inp, r.res
    hit, hbar = hc.hit_point(inp, sc.apertures[0].z)
    assert np.all(np.abs(r.p[r.live, 1].astype(LD) - hit[r.live]) <= hbar[r.live] + hc.U * np.abs(hit[r.live])), f"{title}: hit points"
    assert np.all(np.isfinite(r.p)) and np.all(np.isfinite(r.w)) and np.all(np.isfinite(r.s))
    moved = np.any(r.s != inp["s0"], axis=1)
    assert np.array_equal(moved, functools.reduce(np.logical_or, [rs["bent"] for rs in res])), f"{title}: who is bent"
    opened = 0
    for slot, rs in enumerate(res):
        decided, gone = ~rs["open"], rs["hit"] & (r.w[:, slot] > 0)
        opened += int(np.count_nonzero(rs["open"]))
        assert np.all(r.w[gone, slot + 1] == 0), f"{title}: rays on the aperture are absorbed"
        keep = decided & ~gone & ~rs["neg"]
        assert bits(r.w[keep, slot + 1], r.w[keep, slot]), f"{title}: HURB changes no weight"
        assert np.all(r.w[decided & rs["neg"], slot + 1] == 0), f"{title}: rays bent backwards are absorbed"
        assert abs(int(r.msgs[HURB_NEG_DIR, slot + 1]) - int(np.count_nonzero(rs["neg"] & decided))) <= np.count_nonzero(rs["open"]), title
        assert not np.any(rs["neg"] & ~r.live), "a dead ray is counted only for its own s_z < 0"
        if r.pol is not None:
            still = ~rs["bent"]
            assert bits(r.pol[still, slot + 1], r.pol[still, slot]), f"{title}: pol of rays that are not bent"
    dead = ~r.live
    assert np.all(r.p[dead] == inp["p0"][dead, None, :]) and np.all(r.w[dead] == 0) and bits(r.s[dead], inp["s0"][dead]), f"{title}: dead rays"
    rows = hc.ratios(sc, inp, res[-1], r.s, None if r.pol is None else r.pol[:, len(res)])
    lines.append(hc.format_rows(title, rows))
    return [f"{title} {row['cls']}" for row in rows
            if not row["finite"] or row["s_over"] > 1 or row["pol_over"] > 1 or row["open"] > hc.open_cap(row["cls"])]


# ---- 3a, 3d --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", hc.VARIANTS)
def test_injected_normals_discrete_results_are_the_oracles(variant):
    for name in NAMES:
        r = run(name, variant == "no_pol", False)
        sc, inp, o = r.sc, r.inp, r.orc
        assert r.n % 2 == 1
        if not any(np.any(rs["open"]) for rs in r.res):
            assert np.array_equal(r.msgs, r.orc_msgs), f"{name}\n{r.msgs}\n{r.orc_msgs}"
            assert np.array_equal(r.w > 0, o.w_list > 0), f"{name}: alive masks"
        assert np.array_equal(np.any(r.s != inp["s0"], axis=1), np.any(o.s_final != inp["s0"], axis=1)), f"{name}: inside"
        quiet = hc.cls_mask(sc, inp, "edge-40", "on_edge", "blocked", "outside") | ~r.live
        if len(sc.apertures) == 1:   # not bent by anything: direction and pol come back bit for bit
            assert bits(r.s[quiet], inp["s0"][quiet]) and bits(r.s[quiet], o.s_final[quiet]), name
            if r.pol is not None:
                assert all(bits(r.pol[quiet, i], inp["pol0"][quiet]) for i in range(r.pol.shape[1])), name
        absorbed = hc.cls_mask(sc, inp, "edge-40", "on_edge", "blocked")
        assert np.all(r.w[absorbed, 1] == 0) and bits(r.w[hc.cls_mask(sc, inp, "outside"), 1], inp["w0"][hc.cls_mask(sc, inp, "outside")])
        if r.pol is None:
            assert np.all(np.isnan(r.RT.rays.pol_list))


@pytest.mark.parametrize("variant", hc.VARIANTS)
def test_injected_normals_against_the_exact_bend(variant, capsys):
    lines, bad = [], []
    for name in NAMES:
        bad += check_against_exact(run(name, variant == "no_pol", False), f"{variant} {name}", lines)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, bad


def test_tiny_bends_cover_their_range():
    r = run("big", False, False)
    a = r.res[0]["a"][hc.cls_mask(r.sc, r.inp, "tiny") & r.res[0]["bent"]].astype(np.float64)
    assert a.min() < 2.0 ** -47 and a.max() > 2.0 ** -21 and np.count_nonzero(a < 2.0 ** -25) > 60


# ---- 3b ------------------------------------------------------------------------------------------------------------------
def test_device_draws_against_the_replay(capsys):
    lines, bad = [], []
    for name in NAMES:
        bad += check_against_exact(run(name, False, True), f"drawn {name}", lines)
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert not bad, bad


def worst_over(r: Run, res) -> float:
    rows = hc.ratios(r.sc, r.inp, res[-1], r.s, None)
    return max(row["s_over"] for row in rows)


def test_two_apertures_draw_two_pairs():
    r = run("double", False, True)
    assert not np.any(r.nrm[0] == r.nrm[2]) and not np.any(r.nrm[1] == r.nrm[3])
    both = np.all([rs["bent"] for rs in r.res], axis=0)
    assert np.count_nonzero(both) > 150, "rays bent twice"
    assert worst_over(r, r.res) <= 1
    same = np.concatenate((r.nrm[:2], r.nrm[:2]))   # the first aperture's pair at the second one as well
    assert worst_over(r, hc.evaluate(r.sc, r.inp, r.p, r.pol, r.w, r.n_index, same, np.ones((2, r.n)))) > 1e6


def test_normal_za_bends_about_a_and_zb_about_b():
    """The slit's sides are unequal (0.5 x 1.5): a swapped pair is another bend."""
    r = run("slit_rot", False, True)
    assert worst_over(r, r.res) <= 1
    assert worst_over(r, hc.evaluate(r.sc, r.inp, r.p, r.pol, r.w, r.n_index, r.nrm[::-1], np.ones((1, r.n)))) > 1e6


def test_high_word_of_the_seed_reaches_the_draws():
    lo, hi = run("ring", False, True), run("ring", False, True, hc.SEED + (1 << 32))
    bent = lo.res[0]["bent"]
    assert np.array_equal(bent, hi.res[0]["bent"]) and np.all(np.any(lo.s[bent] != hi.s[bent], axis=1))
    lines = []
    assert check_against_exact(hi, "seed + 2^32", lines) == [], "\n".join(lines)


def test_draws_use_the_global_ray_index():
    """70 001 rays (more than one workgroup's share, a last wave that is not full) against the replay at their global
    indices, and the first 4097 of them bit for bit those of a launch of 4097."""
    sc = hc.scene("slit_rot")
    base = hc.inputs(sc)
    out = []
    for n in (70_001, 4097):
        inp = hc.tile_inputs(base, n)
        r = launch(sc, inp, False, hc.SEED, None)
        r.nrm, rr = hc.pairs(sc, n, hc.SEED)
        r.res = hc.evaluate(sc, inp, r.p, r.pol, r.w, r.n_index, r.nrm, rr)
        lines = []
        assert check_against_exact(r, f"{n} rays", lines) == [], "\n".join(lines)
        out.append(r)
    big, small = out
    k = small.n
    assert bits(big.p[:k], small.p) and bits(big.w[:k], small.w) and bits(big.pol[:k], small.pol) and bits(big.s[:k], small.s)
    period = base["s0"].shape[0]   # the same ray again, 'period' indices later: another pair, another bend
    bent = big.res[0]["bent"][:period] & big.res[0]["bent"][period:2 * period]
    assert np.all(np.any(big.s[:period][bent] != big.s[period:2 * period][bent], axis=1))


# ---- 3c ------------------------------------------------------------------------------------------------------------------
C5_SLIT = hc.Surf("slit", (0.0, 0.0), 0.0, None, None, (2.5, 2.5), (0.05, 2.0), None)   # the aperture of scenes.hurb_slit_lens
C5 = hc.Scene("hurb_slit_lens", (C5_SLIT,), "1.33", None, None, ("all",))
SPECTRA = {"lines": lambda: ot.LightSpectrum("Lines", lines=[450.0, 550.123, 650.0], line_vals=[1.0, 2.0, 0.5]),
           "rectangle": lambda: ot.LightSpectrum("Rectangle", wl0=450., wl1=650.)}


def generated_rays(RT, N, seed):
    """The rays the trace kernel generated, from ot_rays_generate with the same table, ranges and seed (bit-equal:
    test_gpu_generate_replay.py::test_trace_kernels_generate_the_same_rays)."""
    lib, st = _capi.load_library(), RT.rays
    tab, rng = st._source_table(seed), st._source_ranges()
    buf = {k: torch.empty(m * N, dtype=dt, device="cuda") for k, m, dt in
           (("p", 3, torch.float64), ("s", 3, torch.float64), ("w", 1, torch.float32), ("n", 1, torch.float64),
            ("wl", 1, torch.float32), ("pol", 3, torch.float32))}
    rays = _capi.Rays()
    rays.N, rays.nt = N, 1
    rays.p, rays.s, rays.w, rays.n, rays.wl = (buf[k].data_ptr() for k in ("p", "s", "w", "n", "wl"))
    rays.pol = buf["pol"].data_ptr()
    _capi.check(lib.ot_rays_generate(tab.handle, rng, len(rng), seed, 0, C.byref(rays), stream_ptr()))
    torch.cuda.synchronize()
    vec = lambda k: np.ascontiguousarray(buf[k].cpu().numpy().reshape(3, N).T)
    return vec("p"), vec("s"), vec("pol"), buf["w"].cpu().numpy(), buf["wl"].cpu().numpy()


def tail_records(tail):
    """(n, 8) records of the living rays of a render-only trace: p[nt - 2], p[nt - 1], w, wl."""
    cap, n = tail._cap, tail.N
    p = tail._dev["p"].view(3, 2, cap)[:, :, :n].cpu().numpy()
    tw = tail._dev["w"].view(2, cap)[:, :n].cpu().numpy()
    twl = tail._dev["wl"][:n].cpu().numpy()
    live = tw[0] > 0
    assert not tw[1].any() and int(live.sum()) == tail.alive
    return np.concatenate([p[:, 0, live].T, p[:, 1, live].T, tw[0, live, None].astype(np.float64), twl[live, None].astype(np.float64)], axis=1)


@pytest.mark.parametrize("spectrum", list(SPECTRA))
def test_production_kernels_bend_like_the_injected_trace(spectrum):
    N, seed = 10_037, 77
    with ot.global_options.no_warnings():
        RT = scenes.hurb_slit_lens(ot, seed=seed)
        RT.ray_sources[0].spectrum = SPECTRA[spectrum]()
        RT.trace(N)
        A = dict(p=RT.rays.p_list.copy(), w=RT.rays.w_list.copy(), pol=RT.rays.pol_list.copy(), s=RT.rays.s0_list.copy(),
                 wl=RT.rays.wl_list.copy(), msgs=np.array(RT._msgs))
        nt = RT.rays.Nt
        p0, s0, pol0, w0, wl = generated_rays(RT, N, seed)
        assert bits(p0, A["p"][:, 0]) and bits(w0, A["w"][:, 0]) and bits(wl, A["wl"]) and bits(pol0, A["pol"][:, 0])
        if spectrum == "lines":
            assert set(np.unique(wl)) == {np.float32(450.0), np.float32(550.123), np.float32(650.0)}
        tail = TailStorage()
        RT.trace(N, _tail=tail)
        assert np.array_equal(RT._msgs, A["msgs"])
        recs = tail_records(tail)
        nrm, rr = hc.pairs(C5, N, seed)
        RB = scenes.hurb_slit_lens(ot, seed=seed)
        RB.ray_sources[0].spectrum = SPECTRA[spectrum]()
        RB.trace(N, _initial_rays=(p0, s0, pol0, w0, wl), _hurb_normals=nrm.astype(np.float64), _N_list=np.array([N]))
        B = dict(p=RB.rays.p_list.copy(), w=RB.rays.w_list.copy(), pol=RB.rays.pol_list.copy(), s=RB.rays.s0_list.copy(),
                 n=RB.rays.n_list[:, 0].copy(), msgs=np.array(RB._msgs))
    # the render-only form of the same call: the records of the living rays are the stored run's last section, bit for bit
    sel = A["w"][:, nt - 2] > 0
    ref = np.concatenate([A["p"][sel, nt - 2], A["p"][sel, nt - 1], A["w"][sel, nt - 2, None].astype(np.float64),
                          A["wl"][sel, None].astype(np.float64)], axis=1)
    order = lambda a: a[np.lexsort(a.T[::-1])]
    assert tail.traced == N and bits(order(recs), order(ref)), "render-only records differ from the stored sections"
    # section 1 and the direction: each run is within the 3a bar of its exact value, and the two exact values differ by the
    # draw's rounding alone (3b).  Decided from the injected run's sections.
    inp = dict(p0=p0, s0=s0, pol0=pol0, w0=w0, wl=wl, cls=np.zeros(N, dtype=int))
    res = hc.evaluate(C5, inp, B["p"], B["pol"], B["w"], B["n"], nrm, rr)[0]
    sure = ~res["open"]
    assert np.count_nonzero(res["bent"]) > 0.9 * N and np.count_nonzero(res["open"]) <= 2
    assert bits(A["p"][:, 1], B["p"][:, 1]) and bits(A["w"][sure, 1], B["w"][sure, 1])
    assert np.array_equal(A["msgs"][:, :2], B["msgs"][:, :2]) or not np.all(sure)
    # two float32 roundings of values 1e-15 apart: at most one unit in the last place of a component below 1
    assert np.max(np.abs(A["pol"][sure, 1] - B["pol"][sure, 1])) <= 2.0 ** -24, "pol' differs by more than the store's rounding"
    # behind the lens: both refractions and the 12 mm in between multiply a difference of direction by less than 16
    # (d n = d p / R with d p <= 12 d s / s_z and R = 18; a refraction passes d s and d n with factors below 2)
    through = sure & (A["w"][:, nt - 2] > 0) & (B["w"][:, nt - 2] > 0)
    assert np.count_nonzero(through) > 0.5 * N and np.array_equal(A["w"][sure] > 0, B["w"][sure] > 0)
    bar = (2 * res["bar_s"][through] + 2 * hc.U).astype(np.float64)
    assert np.all(np.abs(A["s"][through] - B["s"][through]) <= 16 * bar[:, None]), "final directions"
    assert np.all(np.abs(A["p"][through, 2] - B["p"][through, 2]) <= 16 * 16 * bar[:, None] + 2.0 ** -48), "hit points on the lens"
