"""The HURB step on the host (tests/hurb_cases.py): the integer layer of the draw replay against Philox's known answers,
the longdouble restatement `bend` against mpmath at 50 digits, and the C oracle with injected normals inside the bars that
tests/test_gpu_hurb_step.py holds the device to.  CPU only.

The oracle evaluates the reference's lines in float64 in the reference's order; its distance from the exact value is the
measurement the margins of the bars rest on (no number below comes from the device).  Worst error / bar per class over all
scenes and both variants, as `test_oracle_stays_inside_the_bars` prints it:

    class      s' / bar   pol' / bar            class      s' / bar   pol' / bar
    middle      0.233      0.969                corner      0.268      0.969
    edge-3      0.259      0.964                steep       0.208      0.961
    edge-10     0.247      0.969                centre      0.179      0.969
    edge-20     0.190      0.962                tiny        0.194      (exempt: 4.5e+04, 2.7e-3 absolute)
    edge-30     0.216      0.965
    (edge-40, on_edge, blocked, outside: no ray is bent.)  Open verdicts: none in any class.

pol' / bar is the float32 store of the oracle's own pol': half a unit in the last place of a component above 1/2 is 2^-25,
the bar's first term, so 0.97 is the store and nothing else.  In `tiny` the reference's projection form builds its basis
from s' x s, two vectors down to 2^-48 apart: the result is noise, so the oracle's pol' is exempt there and printed; the
device is held to the exact value in that class as well (tests/test_gpu_hurb_step.py).
"""
import numpy as np
import pytest

import optrace_amd as ot

import hurb_cases as hc
from hurb_cases import LD

NAMES = [sc.name for sc in hc.SCENES]
HURB_NEG_DIR = 4   # Raytracer.INFOS


def _words(s):
    return [int(v, 16) for v in s.split()]


@pytest.mark.parametrize("counter, key, want", [
    ("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_draw_bits_against_known_answers(counter, key, want):
    """kat_vectors of Random123 (as tests/test_generate_replay_host.py) through the argument order of the draw: the counter
    is (ray lo, ray hi, stream, slot), the key (seed lo, seed hi)."""
    c, k = _words(counter), _words(key)
    got = hc.draw_bits(k[0] | (k[1] << 32), np.array([c[0] | (c[1] << 32)], dtype=np.uint64), c[3], stream=c[2])
    assert got.dtype == np.uint32 and got[0].tolist() == _words(want)


def test_normal_pair_layers():
    ray = np.array([0, 1, 63, 64, 4096, (1 << 32) + 5], dtype=np.uint64)
    bits = hc.draw_bits(77, ray, 1).astype(np.uint64)
    z0, z1, r = hc.normal_pair(77, ray, 1)
    u0 = ((bits[:, 1] << np.uint64(32) | bits[:, 0]) >> np.uint64(11)).astype(LD) / LD(2.0 ** 53)
    assert np.all((u0 >= 0) & (u0 < 1)) and np.all(np.abs(r * r + 2 * np.log(1 - u0)) <= 2.0 ** -58 * (1 + r * r))
    assert np.all(np.abs(z0 * z0 + z1 * z1 - r * r) <= 2.0 ** -58 * (1 + r * r))
    # slot, the high word of the seed and the high word of the ray index all reach the block
    assert not np.array_equal(bits, hc.draw_bits(77, ray, 0)) and not np.array_equal(bits, hc.draw_bits(77 + (1 << 32), ray, 1))
    assert not np.array_equal(hc.draw_bits(77, ray[-1:], 1), hc.draw_bits(77, ray[-1:] & np.uint64(0xffffffff), 1))
    # the mean and the variance of 2 x 20000 draws
    za, zb, _ = hc.normal_pair(5, np.arange(20000), 0)
    z = np.concatenate((za, zb)).astype(np.float64)
    assert abs(z.mean()) < 0.02 and abs(z.var() - 1) < 0.03 and abs(np.mean(za * zb)) < 0.02


def test_inputs_are_what_the_classes_say():
    for sc in hc.SCENES:
        inp, surf = hc.inputs(sc), sc.apertures[0]
        n = inp["s0"].shape[0]
        assert n % 2 == 1 and np.all(inp["s0"][:, 2] > 0) and np.count_nonzero(inp["w0"] == 0) == len(range(3, n, 8))
        assert np.max(np.abs(np.sum(inp["s0"] ** 2, axis=1) - 1)) < 2.0 ** -50
        hit, _ = hc.hit_point(inp, surf.z)
        pr = hc.props(surf, hit[:, 0], hit[:, 1])
        m = lambda *c: hc.cls_mask(sc, inp, *c)
        nearest = np.minimum(pr["a_"], pr["b_"]) if surf.kind == "slit" else pr["b_"]
        for e in hc.EDGE_E:
            sel = m(f"edge{e}")
            if np.any(sel):
                assert np.all((nearest[sel] >= 2.0 ** e * (1 - 2.0 ** -8)) & (nearest[sel] < 2.0 ** (e + 1) * (1 + 2.0 ** -8))), (sc.name, e)
                assert np.all(pr["inside"][sel]) and np.all(pr["hit"][sel] == (e == -40))
        assert np.all(pr["inside"][m("middle", "steep", "tiny", "centre", "corner")])
        assert not np.any(pr["hit"][m("middle", "steep", "tiny", "centre", "corner", "outside")])
        # (on_edge is a float64 fact: in longdouble such a point lies 2^-54 to either side, and the mask absorbs it anyway)
        assert np.all(pr["hit"][m("blocked", "on_edge")]) and not np.any(pr["inside"][m("blocked", "outside")])
        if np.any(m("steep")):
            b = pr["b"][m("steep")]
            s = inp["s0"][m("steep")].astype(LD)
            big = np.maximum(np.abs(s[:, 0] * b[:, 0] + s[:, 1] * b[:, 1]), np.abs(s[:, 1] * b[:, 0] - s[:, 0] * b[:, 1]))
            assert big.min() > 0.87 and 1 - big.max() < 2.0 ** -11 and s[:, 2].min() >= 0.0199
        if np.any(m("centre")):
            assert np.all(inp["p0"][m("centre"), :2] == np.asarray(surf.pos))
        if np.any(m("on_edge")) and surf.kind == "ring":   # bitwise in float64, in every rounding order (hc._on_ring_edge)
            dx, dy = inp["p0"][m("on_edge"), 0] - surf.pos[0], inp["p0"][m("on_edge"), 1] - surf.pos[1]
            assert np.all(np.sqrt(dx * dx + dy * dy) == surf.ri) and len(np.unique(dx)) >= 30


def _mp_bend(surf, x, y, s, pol, wl32, n, za, zb, factor):
    """The reference's lines for one bent ray, literally (ps from s' x s), in mpmath."""
    import mpmath as mp
    f = lambda v: mp.mpf(float(v))
    cr = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    unit = lambda a: [v / mp.sqrt(dot(a, a)) for v in a]
    dx, dy = f(x) - f(surf.pos[0]), f(y) - f(surf.pos[1])
    if surf.kind == "ring":
        r = mp.sqrt(dx * dx + dy * dy)
        b_ = f(surf.ri) - r
        a_ = mp.sqrt(b_ * f(surf.ri))
        th = mp.atan2(dy, dx)
        b = [mp.cos(th), mp.sin(th), mp.mpf(0)]
    else:
        ang = f(hc.angle_of(surf))
        xr, yr = dx * mp.cos(-ang) - dy * mp.sin(-ang), dx * mp.sin(-ang) + dy * mp.cos(-ang)
        a_, b_ = f(surf.dimi[1]) / 2 - abs(yr), f(surf.dimi[0]) / 2 - abs(xr)
        b = [mp.cos(ang), mp.sin(ang), mp.mpf(0)]
    a = [-b[1], b[0], b[2]]
    s, pol = [f(v) for v in s], [f(v) for v in pol]
    cpa, cpb = mp.sqrt(1 - dot(s, a) ** 2), mp.sqrt(1 - dot(s, b) ** 2)
    k = 2 * mp.pi * f(n) / f(np.float32(wl32) * np.float32(1e-9))
    tb = abs(f(factor) / (2 * b_ * cpb * f(1e-3) * k)) * f(zb)
    ta = abs(f(factor) / (2 * a_ * cpa * f(1e-3) * k)) * f(za)
    sa = unit(cr(b, s))
    sb = cr(s, sa)
    s_ = unit([s[c] + sa[c] * ta + sb[c] * tb for c in range(3)])
    ps = unit(cr(s_, s))
    pp, pp_ = cr(ps, s), cr(ps, s_)
    A_ts, A_tp = dot(ps, pol), dot(pp, pol)
    return s_, [ps[c] * A_ts + pp_[c] * A_tp for c in range(3)]


def _oracle(sc, no_pol):
    inp = hc.inputs(sc)
    with ot.global_options.no_warnings():
        RT = hc.raytracer(ot, sc, no_pol)
        RT._geometry_checks()
        assert not RT.geometry_error
        plain, _ = hc.oracle_trace(RT, inp, None)                      # (for the index in front of the aperture)
        n_index = plain.n_list[:, 0].copy()
        nrm = hc.injected(sc, inp, hc.SEED, n_index)
        rays, msgs = hc.oracle_trace(RT, inp, nrm)
    return inp, rays, msgs, nrm, n_index


def test_bend_against_mpmath():
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 50
    checked = 0
    for sc in hc.SCENES[:5]:
        inp, rays, _, nrm, n_index = _oracle(sc, False)
        res = hc.evaluate(sc, inp, rays.p_list, rays.pol_list, rays.w_list, n_index, nrm)[0]
        for r in range(0, inp["s0"].shape[0], 16):
            if not res["bent"][r]:
                continue
            s_, pol_ = _mp_bend(sc.apertures[0], rays.p_list[r, 1, 0], rays.p_list[r, 1, 1], inp["s0"][r], inp["pol0"][r], inp["wl"][r],
                                n_index[r], nrm[0][r], nrm[1][r], hc.factor_of(sc))
            # longdouble carries 2^-64 where the bars count roundings of 2^-53: it follows the exact value 2^11 times closer than
            # the bar, whatever the conditioning (2^-8 of the bar is asked); pol' follows s' with a factor below 4
            thr = float(res["bar_s"][r]) * 2.0 ** -8 + 2.0 ** -56
            ld = lambda v: mp.mpf(float(v)) + mp.mpf(float(v - LD(float(v))))   # a longdouble, exactly
            assert all(abs(float(s_[c] - ld(res["s_"][r, c]))) < thr for c in range(3)), (sc.name, r)
            assert all(abs(float(pol_[c] - ld(res["pol_"][r, c]))) < 4 * thr for c in range(3)), (sc.name, r)
            checked += 1
    assert checked > 150


@pytest.mark.parametrize("no_pol", [False, True], ids=list(hc.VARIANTS))
def test_oracle_stays_inside_the_bars(no_pol, capsys):
    lines, bad, worst = [], [], {}
    for sc in hc.SCENES:
        inp, rays, msgs, nrm, n_index = _oracle(sc, no_pol)
        n, live = inp["s0"].shape[0], inp["w0"] > 0
        hit, hbar = hc.hit_point(inp, sc.apertures[0].z)
        assert np.all(np.abs(rays.p_list[live, 1].astype(LD) - hit[live]) <= hbar[live] + hc.U * np.abs(hit[live])), sc.name
        res = hc.evaluate(sc, inp, rays.p_list, None if no_pol else rays.pol_list, rays.w_list, n_index, nrm)
        last = res[-1]
        # discrete: who is bent, who is absorbed, the verdicts and their counter, what stays untouched
        moved = np.any(rays.s_final != inp["s0"], axis=1)
        assert np.array_equal(moved, res[0]["bent"] | last["bent"]), sc.name
        for slot, rs in enumerate(res):
            decided = ~rs["open"]
            gone = rs["hit"] & (rays.w_list[:, slot] > 0)
            assert np.all((rays.w_list[:, slot + 1] == 0)[gone]) and not np.any(rs["neg"] & ~rs["bent"]), sc.name
            keep = decided & ~gone & ~rs["neg"]
            assert np.array_equal(rays.w_list[keep, slot + 1], rays.w_list[keep, slot]), sc.name
            assert abs(int(msgs[HURB_NEG_DIR, slot + 1]) - int(np.count_nonzero(rs["neg"] & decided))) <= np.count_nonzero(rs["open"])
            if not no_pol:
                still = ~rs["bent"]
                assert np.array_equal(rays.pol_list[still, slot + 1], rays.pol_list[still, slot]), sc.name
        assert np.all(rays.p_list[~live] == inp["p0"][~live, None, :]) and np.all(rays.w_list[~live] == 0)
        assert np.array_equal(rays.s_final[~live], inp["s0"][~live])
        rows = hc.ratios(sc, inp, last, rays.s_final, None if no_pol else rays.pol_list[:, len(res)])
        lines.append(hc.format_rows(f"{'no_pol' if no_pol else 'pol'} {sc.name}", rows))
        for row in rows:
            w = worst.setdefault(row["cls"], [0.0, 0.0, 0.0, 0])
            exempt = row["cls"] == "tiny"
            w[0], w[3] = max(w[0], row["s_over"]), w[3] + row["open"]
            w[1 if not exempt else 2] = max(w[1 if not exempt else 2], row["pol_over"])
            if not row["finite"] or row["s_over"] > 1 or (row["pol_over"] > 1 and not exempt) or row["open"] > hc.open_cap(row["cls"]):
                bad.append(f"{sc.name} {row['cls']}")
        if "tiny" in sc.classes:   # the bends of the class are what it promises
            a = last["a"][hc.cls_mask(sc, inp, "tiny") & last["bent"]].astype(np.float64)
            assert a.min() < 2.0 ** -47 and a.max() > 2.0 ** -21 and np.count_nonzero(a < 2.0 ** -25) > 60
    with capsys.disabled():
        print("\n" + "\n".join(lines))
        print("worst per class (s' / bar, pol' / bar, exempt pol' / bar, open verdicts):")
        print("\n".join(f"    {c:9s} {w[0]:.3f}  {w[1]:.3f}  {w[2]:.3g}  {w[3]}" for c, w in worst.items()))
    assert not bad, bad


def test_bars_bite():
    """The bars are not vacuous: the restatement with one planted mistake of the kind a kernel can make leaves them."""
    sc = hc.scene("slit_abbe")
    inp, rays, _, nrm, n_index = _oracle(sc, False)
    good = hc.evaluate(sc, inp, rays.p_list, rays.pol_list, rays.w_list, n_index, nrm)[0]
    sel = good["bent"] & ~good["open"]

    def over(res):
        return float(np.max(np.abs(res["s_"][sel] - good["s_"][sel]) / good["bar_s"][sel][:, None]))

    swapped = hc.evaluate(sc, inp, rays.p_list, rays.pol_list, rays.w_list, n_index, nrm[::-1])[0]
    assert over(swapped) > 1e6
    wl64 = hc.bend(rays.p_list[:, 1, 0], rays.p_list[:, 1, 1], inp["s0"], inp["pol0"], inp["w0"], inp["wl"],
                   n_index * (1 + 2.0 ** -26), nrm[0], nrm[1], sc.apertures[0])   # k off by a float32 rounding of the wavelength
    assert over(wl64) > 100
