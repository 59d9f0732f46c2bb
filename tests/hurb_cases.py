"""Inputs, host restatement and error bars for the HURB step of the trace kernel (hurb_bend of csrc/ot_trace.hpp with
hurb_props and philox_normal2 of csrc/ot_device.hpp), shared by tests/test_hurb_host.py and tests/test_gpu_hurb_step.py.
NumPy only; nothing here reads the reference project or a fixture -- everything is computed when the tests run.

Restatement
  normal_pair(seed, ray, slot)   the device's two normal draws: Philox-4x32-10 on the counter (ray lo, ray hi, 0x48555242, slot)
        with the key (seed lo, seed hi) bit for bit, the two 53-bit uniforms u = (64 bits >> 11) 2^-53 exactly, then in
        longdouble r = sqrt(-2 log(1 - u0)), z0 = r cos(2 pi u1), z1 = r sin(2 pi u1).
  bend(...)   Raytracer.__hurb (raytracer.py:417-490) with RingSurface.hurb_props / SlitSurface.hurb_props and the surfaces'
        masks, from their definitions in longdouble: cos / sin(atan2(dy, dx)) = (dx, dy) / r, a = (-b_y, b_x, 0), the float32
        product wl * float32(1e-9), the bend mask hwnh & inside, s'_z < 0 over all rays, pol' by the projection form
        ps A_ts + (ps x s') A_tp.  One thing is written differently from the reference's lines, for the conditioning of the
        restatement itself: ps = normalize(s' x s) is formed as normalize(tb (s.s) sa - ta sb), which is s' x s |v| exactly
        (s' |v| = s + ta sa + tb sb, sa x s = -sb, sb x s = (s.s) sa) without the cancellation of two nearly equal vectors.
        tests/test_hurb_host.py holds it against the literal form in mpmath at 50 digits.

Scenes and classes (see SCENES): one point source given through `_initial_rays`, one HURB aperture, nothing else -- the
end aperture that every tracer appends stands behind it, so the aperture is not the last element (which never bends,
raytracer.py:385).  Classes of 128 rays (33 where every ray is the same point):
  middle      hit points in the inner half of the opening, s_z >= 0.5, wl from {380, 550.123, 780} as float32
  edge<e>     distance to the nearest edge 2^e [1, 2).  The ladder is -3, -10, -20, -30, -40: an opening of half width 0.5
              (ring) or 0.25 (slit) has no point 2^-1 [1, 2) from its edge; -3 is the outer half that `middle` leaves out.
              At -40 the ray is within N_EPS = 1e-10 of the edge: the surface's mask counts it as a hit, so it is absorbed
              and NOT bent although hurb_props calls it inside; the bars then have nothing to say and the discrete
              comparison with the oracle has.
  corner      slit: both distances small, 2^-10 .. 2^-30 each
  centre      the ring's centre, bitwise (the r == 0 branch); s = (0, 0, 1) so that the hit point is the start point's x, y
  on_edge     r == ri bitwise (ring), |x'| == hdx or |y'| == hdy bitwise (unrotated slit): not inside, absorbed, unchanged
  blocked     in the opaque part;  outside: beyond the outer rim (passes unbent)
  steep       |s.b| or |s.a| = 1 - 2^-k [1, 2), k = 4 .. 12.  s_z >= 0.05 of the issue cannot hold beyond |s.b| = 0.99875
              (s_z^2 <= 1 - (s.b)^2): s_z = q sqrt(1 - (s.b)^2) with q in 0.9 .. 1, i.e. s_z >= 0.0199.
  tiny        the large ring with the injected normals scaled so that |s' x s| runs over 2^-20 .. 2^-48
Every eighth ray has w0 = 0; no input has s_z <= 0; every launch has an odd number of rays.  Apart from cos / sin of the
one slit angle the inputs come from the bit generator through + - * / sqrt.

Bars (u = 2^-53; hurb_bend and hurb_props evaluate without contraction, ot_div / ot_sqrt / normalize3 return IEEE bits).
Counting roundings from the stored hit point (x, y), in units of u:
  b         ring: dx 1, dx^2 + dy^2 4, r 3, dx / r 5 per component; as cos(atan2) (the oracle's form) 8.   delta_b = 8
  s.a, s.b  8 (|s_x| + |s_y|) + 2 <= 14 absolute
  cos_psi   1 - (s.b)^2: 28 |s.b| + 2 absolute, relative to 1 - (s.b)^2 = 1 / (1 + kappa_b) with kappa_b =
            (s.b)^2 / (1 - (s.b)^2); after the square root 15 (1 + kappa_b) + 1 = 16 + 15 kappa_b
  b_        ring: r carries 3, so ri - r carries 3 ri / b_ + 1; slit: the rotation 4 (|dx| + |dy|) / b_, the difference 1.
            With c_b = ri / b_ (ring) or (|dx| + |dy|) / b_ (slit):  4 c_b + 1;  a_ = sqrt(b_ ri): 2 c_b + 2 <= 4 c_a + 1
            with c_a = c_b (ring);  slit: 4 c_a + 1 with c_a = (|dx| + |dy|) / a_
  k         pi 1.1, two products / quotients 2 (n and the float32 wl are inputs):  4
  tan_th    three products of the denominator, the quotient, the product with z:  5
            E_b = 4 c_b + 15 kappa_b + 26,  E_a = 4 c_a + 15 kappa_a + 26     (relative error of tan_thb, tan_tha)
  sa        b x s: 9, 9, 14.3 absolute, norm 20; divided by |b x s| = cos_psi_b: 20 q_b + 3 with q_b = sqrt(1 + kappa_b)
  sb        s x sa: 20 q_b + 6
  s'        v = s + sa ta + sb tb, s' = v / |v|.  An error of direction delta in sa reaches s' as delta |ta| / |v| =
            delta G_a; a relative error E in ta only through the part of ta sa perpendicular to v:
            E |ta| sqrt(1 + tb^2) / |v|^2 = E g_a (at a bend of 10^4 the ray points along sb whatever tb is exactly).
            The sums and the normalisation: K = 8.
      |s'_dev - s'| <= u [8 + G_a (20 q_b + 4) + G_b (20 q_b + 7) + g_a E_a + g_b E_b]          per component
  pol', w   the bars of tests/test_gpu_refraction_step.py with a = |s' x s|:  2^-25 + 2^-30 + min(2^-25, 2^-49 / a) per
            component of pol', plus what the error of s' above does to pol': the projection form is R (pol - s (s.pol)) with
            R the rotation about s x s' that takes s to s', R = I + [k]x + [k]x^2 / (1 + c), k = s x s', c = s.s', so an
            error d in s' moves pol' by at most L d, L = 1 + 2 a / (1 + c) + a^2 / (1 + c)^2 (<= 4 up to a right angle).
            L times the s' bar is below 2^-38 in every class but `corner`, where both tangents are ~10^4 and s' itself is
            only good to 10^-8.  HURB does not change a weight: w' is w or 0, compared bit for bit.
  draws     (3b) 1 - u0 is exact, log within 1 ulp = 2 u, the square root halves it and adds 1: r carries 2 u; sincospi
            below 1 ulp of a value <= 1: 2 u; the product 1:  |z_dev - z| <= 6 u r (5 counted, 1 spare).  It reaches s' as
            6 u r (|tan_sig_a| + |tan_sig_b|) / |v|, on top of the bar above.
  verdict   s'_z < 0 is left open where |s'_z| is within the direction bar of zero (3d caps the number of such rays).
  second aperture (double scene): its s is the first one's s' and carries that bar, amplified by
            A = 1 + G_a (2 + q_b + kappa_a) + G_b (3 + q_b + kappa_b)   (d sa / ds <= q_b, d ta / ta <= (1 + kappa_a) ds).
"""
from __future__ import annotations

from collections import namedtuple
from fractions import Fraction

import numpy as np

import refraction_cases as rc
from generate_replay import LD, LD_PI, philox4x32

U = LD(2.0 ** -53)
N_EPS = 1e-10             # Surface.N_EPS
HURB_STREAM = 0x48555242
FACTOR = 2 ** 0.5         # Raytracer.HURB_FACTOR
DEPTH = 0.03              # mm between a ray's start and the aperture plane, along the ray
WLS = np.array([380.0, 550.123, 780.0], dtype=np.float32)
N_CLASS, N_POINT = 128, 33
EDGE_E = (-3, -10, -20, -30, -40)
SEED = 20250

Surf = namedtuple("Surf", "kind pos z r ri dim dimi rot")   # rot: degrees given to Surface.rotate, then to Aperture.rotate
Scene = namedtuple("Scene", "name apertures medium factor outline classes")

RING = Surf("ring", (0.25, -0.125), 0.0, 3.0, 0.5, None, None, None)
BIG = Surf("ring", (0.0, 0.0), 0.0, 250.0, 200.0, None, None, None)
SLIT = Surf("slit", (-0.125, 0.25), 0.0, None, None, (4.0, 4.0), (0.5, 1.5), None)
SLIT_ROT = Surf("slit", (0.25, 0.125), 0.0, None, None, (4.0, 3.0), (0.5, 1.5), (33.0, -12.5))
SLIT_2ND = Surf("slit", (0.0, 0.0), 1.0, None, None, (9.0, 9.0), (3.0, 2.5), (33.0, -12.5))
BOX, BIG_BOX = (-12, 12, -12, 12, -12, 40), (-300, 300, -300, 300, -12, 40)
_EDGES = tuple(f"edge{e}" for e in EDGE_E)

SCENES = (
    Scene("ring", (RING,), "1", None, BOX, ("middle",) + _EDGES + ("centre", "on_edge", "blocked", "outside", "steep")),
    Scene("ring_water_f1", (RING,), "1.33", 1.0, BOX, ("middle", "edge-10", "steep", "centre")),
    Scene("big", (BIG,), "1", None, BIG_BOX, ("middle", "tiny", "centre")),
    Scene("slit_abbe", (SLIT,), "abbe", None, BOX, ("middle",) + _EDGES + ("corner", "on_edge", "blocked", "outside", "steep")),
    Scene("slit_rot", (SLIT_ROT,), "1.33", None, BOX, ("middle", "edge-10", "edge-30", "corner", "blocked", "steep")),
    Scene("double", (RING, SLIT_2ND), "1", None, BOX, ("middle", "edge-10", "blocked")),
    # a negative factor: tan_sig is negative, and |tan_sig| is what scales the draw (np.random.normal(scale=np.abs(...)))
    Scene("slit_f_minus1", (SLIT,), "1", -1.0, BOX, ("middle", "edge-10")),
)
VARIANTS = ("pol", "no_pol")


def factor_of(sc: Scene) -> float:
    return FACTOR if sc.factor is None else sc.factor


def scene(name: str) -> Scene:
    return next(sc for sc in SCENES if sc.name == name)


def angle_of(surf: Surf) -> float:
    """Surface._angle after the two rotations: 0.0 + deg2rad(first) + deg2rad(second)."""
    a = 0.0
    for deg in surf.rot or ():
        a = a + np.deg2rad(deg)
    return float(a)


# ---- the draws ---------------------------------------------------------------------------------------------------------
def draw_bits(seed: int, ray, slot: int, stream: int = HURB_STREAM):
    """-> (n, 4) uint32: the Philox block behind the normal pair of global ray index `ray` at HURB aperture `slot`."""
    ray = np.atleast_1d(np.asarray(ray)).astype(np.uint64)
    ctr = np.stack([ray & np.uint64(0xffffffff), ray >> np.uint64(32), np.full_like(ray, stream), np.full_like(ray, slot)], axis=-1)
    return philox4x32(ctr, np.array([seed & 0xffffffff, (seed >> 32) & 0xffffffff], dtype=np.uint64))


def normal_pair(seed: int, ray, slot: int):
    """-> z0, z1, r (longdouble arrays): z0 belongs to the a axis, z1 to the b axis."""
    c = draw_bits(seed, ray, slot).astype(np.uint64)
    u0 = ((c[:, 1] << np.uint64(32) | c[:, 0]) >> np.uint64(11)).astype(LD) * LD(2.0 ** -53)
    u1 = ((c[:, 3] << np.uint64(32) | c[:, 2]) >> np.uint64(11)).astype(LD) * LD(2.0 ** -53)
    r = np.sqrt(-2 * np.log(1 - u0))
    return r * np.cos(2 * LD_PI * u1), r * np.sin(2 * LD_PI * u1), r


# ---- the step ----------------------------------------------------------------------------------------------------------
def _rot(dx, dy, angle):
    c, s = np.cos(LD(angle)), np.sin(LD(angle))
    return dx * c - dy * s, dx * s + dy * c


def props(surf: Surf, x, y) -> dict:
    """hurb_props and mask of the aperture's surface in longdouble -> a_, b_, b (n, 3), inside, hit, c_a, c_b."""
    dx, dy = np.asarray(x, dtype=LD) - LD(surf.pos[0]), np.asarray(y, dtype=LD) - LD(surf.pos[1])
    b = np.zeros(dx.shape + (3,), dtype=LD)
    with np.errstate(all="ignore"):
        if surf.kind == "ring":
            r2 = dx * dx + dy * dy
            r, R = np.sqrt(r2), LD(surf.ri)
            inside, b_ = r < R, R - r
            a_ = np.sqrt(b_ * R)
            pos = r > 0
            b[:, 0], b[:, 1] = np.where(pos, dx / np.where(pos, r, 1), 1), np.where(pos, dy / np.where(pos, r, 1), 0)
            hit = ((R - LD(N_EPS)) ** 2 <= r2) & (r2 <= (LD(surf.r) + LD(N_EPS)) ** 2)
            c_b = R / np.abs(b_)
            c_a = c_b
        else:
            ang = angle_of(surf)
            xr, yr = _rot(dx, dy, -ang)
            hx, hy = LD(surf.dimi[0]) / 2, LD(surf.dimi[1]) / 2
            a_, b_ = hy - np.abs(yr), hx - np.abs(xr)
            inside = (a_ > 0) & (b_ > 0)
            b[:, 0], b[:, 1] = np.cos(LD(ang)), np.sin(LD(ang))
            e = LD(N_EPS)
            outer = (np.abs(xr) <= LD(surf.dim[0]) / 2 + e) & (np.abs(yr) <= LD(surf.dim[1]) / 2 + e)
            opening = (-hx + e <= xr) & (xr <= hx - e) & (-hy + e <= yr) & (yr <= hy - e)
            hit = outer & ~opening
            c_b, c_a = (np.abs(dx) + np.abs(dy)) / np.abs(b_), (np.abs(dx) + np.abs(dy)) / np.abs(a_)
    return dict(a_=a_, b_=b_, b=b, inside=inside, hit=hit, c_a=c_a, c_b=c_b)


def _norm(v):
    return np.sqrt(rc._rdot(v, v))


def bend(x, y, s, pol, w, wl32, n, za, zb, surface: Surf, hurb_factor=FACTOR) -> dict:
    """One HURB step in longdouble.  x, y: the hit point on the aperture's plane; s (k, 3); pol (k, 3) float32 or None
    (no_pol); w the weight before the aperture; wl32 float32; n the index in front; za, zb the normal draws.
    -> dict(s_, pol_, bent, neg, absorbed, a (|s' x s|), bar_s, draw_gain, amplify, open, conds...)."""
    s = np.asarray(s, dtype=LD)
    pr = props(surface, x, y)
    hw = np.asarray(w) > 0
    bent = hw & ~pr["hit"] & pr["inside"]
    b = pr["b"]
    a = np.stack((-b[:, 1], b[:, 0], b[:, 2]), axis=1)
    with np.errstate(all="ignore"):
        sa_, sb_ = rc._rdot(s, a), rc._rdot(s, b)
        cpa, cpb = np.sqrt(1 - sa_ ** 2), np.sqrt(1 - sb_ ** 2)
        wlm = (np.asarray(wl32, dtype=np.float32) * np.float32(1e-9)).astype(LD)   # a float32 product
        k = 2 * LD_PI * np.asarray(n, dtype=LD) / wlm
        sig_b = LD(hurb_factor) / (2 * pr["b_"] * cpb * LD(1e-3) * k)
        sig_a = LD(hurb_factor) / (2 * pr["a_"] * cpa * LD(1e-3) * k)
        ta, tb = np.abs(sig_a) * np.asarray(za, dtype=LD), np.abs(sig_b) * np.asarray(zb, dtype=LD)
        sa = rc._cross(b, s)
        sa = sa / _norm(sa)[:, None]
        sb = rc._cross(s, sa)
        sab = s + sa * ta[:, None] + sb * tb[:, None]
        v = _norm(sab)
        s_ = np.where(bent[:, None], sab / v[:, None], s)
        m = sa * (tb * rc._rdot(s, s))[:, None] - sb * ta[:, None]     # (s' x s) |v|
        bendmag = np.where(bent, _norm(m) / v, 0)
        c1 = 1 + rc._rdot(s, s_)
        pol_gain = 1 + 2 * bendmag / c1 + (bendmag / c1) ** 2
        pol_ = None
        if pol is not None:
            polL = np.asarray(pol, dtype=np.float32).astype(LD)
            ps = m / _norm(m)[:, None]
            pp, pp_ = rc._cross(ps, s), rc._cross(ps, s_)
            pol_ = np.where(bent[:, None], ps * rc._rdot(ps, polL)[:, None] + pp_ * rc._rdot(pp, polL)[:, None], polL)
        ka, kb = sa_ ** 2 / (1 - sa_ ** 2), sb_ ** 2 / (1 - sb_ ** 2)
        qb = np.sqrt(1 + kb)
        Ga, Gb = np.abs(ta) / v, np.abs(tb) / v
        ga, gb = Ga * np.sqrt(1 + tb ** 2) / v, Gb * np.sqrt(1 + ta ** 2) / v
        Ea, Eb = 4 * pr["c_a"] + 15 * ka + 26, 4 * pr["c_b"] + 15 * kb + 26
        bar = U * (8 + Ga * (20 * qb + 4) + Gb * (20 * qb + 7) + ga * Ea + gb * Eb)
        amplify = 1 + Ga * (2 + qb + ka) + Gb * (3 + qb + kb)
        draw_gain = 6 * U * (np.abs(sig_a) + np.abs(sig_b)) / v          # times the pair's r
    neg = s_[:, 2] < 0
    bar = np.where(bent, bar, 0)
    return dict(s_=s_, pol_=pol_, bent=bent, neg=neg, hit=pr["hit"], inside=pr["inside"], a=bendmag, bar_s=bar,
                amplify=np.where(bent, amplify, 1), pol_gain=pol_gain, draw_gain=np.where(bent, draw_gain, 0),
                open=bent & (np.abs(s_[:, 2]) <= bar), c_a=pr["c_a"], c_b=pr["c_b"], kappa_a=ka, kappa_b=kb,
                inv_a=1 / np.where(bendmag > 0, bendmag, 1), tan_sig_a=sig_a, tan_sig_b=sig_b, ta=ta, tb=tb)


def pol_bar(a):
    """The refraction pin's bar (refraction_cases.pol_bar) for the bend a = |s' x s|; unbent rays: 0 (bitwise)."""
    return np.where(a > 0, rc.pol_bar(np.where(a > 0, a, 1)), 0)


# ---- inputs ------------------------------------------------------------------------------------------------------------
def _dirs(rng, k, st_max=0.85):
    """k unit vectors with sin(theta) <= st_max at a random azimuth (s_z >= 0.5 for 0.85)."""
    st, cs = rng.uniform(0, st_max, k), rc._unit2(rng, k)
    return np.stack((st * cs[0], st * cs[1], np.sqrt(1 - st * st)), axis=1)


def _to_world(surf, xr, yr):
    ang = angle_of(surf)
    if ang == 0.0:
        return xr, yr
    c, s = np.cos(ang), np.sin(ang)
    return xr * c - yr * s, xr * s + yr * c


def _sign(rng, k):
    return np.where(rng.random(k) < 0.5, -1.0, 1.0)


def _b_axis(surf, d):
    if surf.kind == "ring":
        r = np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2)
        return np.stack((d[:, 0] / r, d[:, 1] / r, np.zeros_like(r)), axis=1)
    ang = angle_of(surf)
    return np.tile([np.cos(ang), np.sin(ang), 0.0], (d.shape[0], 1))


def _on_ring_edge(surf, rng, k):
    """Start points whose r, as any rounding order of sqrt(dx dx + dy dy) gives it, equals ri bitwise."""
    px, py, ri = surf.pos[0], surf.pos[1], surf.ri
    out = [(px + ri, py), (px - ri, py), (px, py + ri), (px, py - ri)]

    def exact(dx, dy):
        fx, fy = Fraction(dx) ** 2, Fraction(dy) ** 2
        sums = {float(dx * dx + dy * dy), float(fx + Fraction(dy * dy)), float(Fraction(dx * dx) + fy)}   # plain, two fused orders
        return all(np.sqrt(v) == ri for v in sums)

    while len(out) < k:
        c, sn = rc._unit2(rng, 1)
        x = px + ri * float(c[0])
        y = up = dn = py + float(np.sign(sn[0])) * float(np.sqrt(ri * ri - (x - px) ** 2))
        cands = [y]
        for _ in range(32):
            up, dn = float(np.nextafter(up, np.inf)), float(np.nextafter(dn, -np.inf))
            cands += [up, dn]
        hit = [v for v in cands if exact(x - px, v - py)]
        if hit:
            out.append((x, hit[0]))
    return np.array(out[:k])


def _class_rays(sc: Scene, cls: str, rng):
    """-> (xy (k, 2) world coordinates of the hit point on the first aperture, s (k, 3), wl (k,) f32)"""
    surf = sc.apertures[0]
    k = N_POINT if cls in ("centre", "on_edge") else N_CLASS
    ring = surf.kind == "ring"
    wl = np.full(k, 550.0, dtype=np.float32)
    s = _dirs(rng, k, 0.43 if sc.name == "double" else 0.85)
    hx, hy = (surf.dimi[0] / 2, surf.dimi[1] / 2) if not ring else (None, None)
    zaxis = np.tile([0.0, 0.0, 1.0], (k, 1))

    def polar(r):
        c, sn = rc._unit2(rng, k)
        return np.stack((r * c, r * sn), axis=1)

    def rect(xr, yr):
        return np.stack(_to_world(surf, xr, yr), axis=1)

    if cls in ("middle", "tiny", "steep"):
        if cls == "middle":
            wl = WLS[rng.integers(0, 3, k)]
        d = polar(surf.ri / 2 * np.sqrt(rng.uniform(0.0004, 1, k))) if ring else rect(rng.uniform(-hx / 2, hx / 2, k), rng.uniform(-hy / 2, hy / 2, k))
        if cls == "steep":
            e = _b_axis(surf, d)
            along_a = np.arange(k) % 2 == 1
            e = np.where(along_a[:, None], np.stack((-e[:, 1], e[:, 0], e[:, 2]), axis=1), e)
            eo = np.stack((-e[:, 1], e[:, 0], e[:, 2]), axis=1)
            c = (1 - np.ldexp(1 + rng.random(k), -rng.integers(4, 13, k))) * _sign(rng, k)   # 1 - 2^-k [1, 2)
            q = np.sqrt(1 - c * c)
            sphi = rng.uniform(-0.43, 0.43, k)
            s = rc._normalized(c[:, None] * e + (q * np.sqrt(1 - sphi * sphi))[:, None] * zaxis + (q * sphi)[:, None] * eo)
    elif cls.startswith("edge") or cls == "corner":
        dist = lambda e: np.ldexp(1 + rng.random(k), e)
        if cls == "corner":
            da, db = dist(-rng.integers(10, 31, k)), dist(-rng.integers(10, 31, k))
            d = rect(_sign(rng, k) * (hx - db), _sign(rng, k) * (hy - da))
        elif ring:
            d = polar(surf.ri - dist(int(cls[4:])))
        else:
            dd, inner = dist(int(cls[4:])), rng.uniform(-0.5, 0.5, k)
            x_edge = np.arange(k) % 2 == 0
            d = rect(np.where(x_edge, _sign(rng, k) * (hx - dd), inner * hx), np.where(x_edge, inner * hy, _sign(rng, k) * (hy - dd)))
    elif cls == "centre":
        d, s = np.zeros((k, 2)), zaxis
    elif cls == "on_edge":
        s = zaxis
        if ring:
            return _on_ring_edge(surf, rng, k), s, wl
        x_edge, inner = np.arange(k) % 2 == 0, rng.uniform(-0.9, 0.9, k)
        d = np.stack((np.where(x_edge, _sign(rng, k) * hx, inner * hx), np.where(x_edge, inner * hy, _sign(rng, k) * hy)), axis=1)
    elif cls == "blocked":
        d = polar(rng.uniform(surf.ri + 0.1, surf.r - 0.1, k)) if ring else rect(_sign(rng, k) * rng.uniform(hx + 0.1, surf.dim[0] / 2 - 0.1, k),
                                                                                   rng.uniform(-1, 1, k) * (surf.dim[1] / 2 - 0.1))
    elif cls == "outside":
        d = polar(rng.uniform(3.5, 6.0, k))
    else:
        raise ValueError(cls)
    return d + np.asarray(surf.pos), s, wl


def inputs(sc: Scene) -> dict:
    """-> dict(p0, s0 (n, 3) f64, pol0 (n, 3) f32, w0, wl (n,) f32, cls (n,) index into sc.classes), n odd."""
    index = [q.name for q in SCENES].index(sc.name)
    XY, S, WL, C = [], [], [], []
    for ci, cls in enumerate(sc.classes):
        xy, s, wl = _class_rays(sc, cls, np.random.default_rng([SEED, index, ci]))
        XY.append(xy), S.append(s), WL.append(wl), C.append(np.full(s.shape[0], ci))
    xy, s0, wl, cls = np.concatenate(XY), np.concatenate(S), np.concatenate(WL), np.concatenate(C)
    if s0.shape[0] % 2 == 0:
        xy, s0, wl, cls = xy[:-1], s0[:-1], wl[:-1], cls[:-1]
    n = s0.shape[0]
    rng = np.random.default_rng([SEED + 1, index])
    pol0 = rc._pol_for(s0, rng)
    w0 = rng.uniform(0.25, 1.0, n).astype(np.float32)
    w0[3::8] = 0.0
    hit = np.column_stack((xy, np.full(n, sc.apertures[0].z)))
    straight = np.all(s0 == [0.0, 0.0, 1.0], axis=1)
    p0 = np.where(straight[:, None], hit - [0.0, 0.0, DEPTH], hit - DEPTH * s0)
    assert np.all(s0[:, 2] > 0) and n % 2 == 1
    return dict(p0=p0, s0=s0, pol0=pol0, w0=w0, wl=wl.astype(np.float32), cls=cls)


def cls_mask(sc: Scene, inp: dict, *prefixes) -> np.ndarray:
    """Rays of the named classes; "edge*" names a whole family."""
    fits = lambda c: any(c == p or (p.endswith("*") and c.startswith(p[:-1])) for p in prefixes)
    return np.isin(inp["cls"], [ci for ci, c in enumerate(sc.classes) if fits(c)])


def tile_inputs(inp: dict, n: int) -> dict:
    """The rays of `inp` repeated cyclically to n rays."""
    idx = np.arange(n) % inp["s0"].shape[0]
    return {k: np.ascontiguousarray(v[idx]) for k, v in inp.items()}


def hit_point(inp: dict, z: float):
    """p0 + t s on the plane z in longdouble, and its bar: 4 roundings on the scale |p0| + |t s| per component."""
    p0, s0 = inp["p0"].astype(LD), inp["s0"].astype(LD)
    t = (LD(z) - p0[:, 2]) / s0[:, 2]
    return p0 + t[:, None] * s0, 4 * U * (np.abs(p0) + np.abs(t[:, None] * s0))


def pairs(sc: Scene, n: int, seed: int, first: int = 0):
    """The replayed draws of a launch of n rays whose first ray has the global index `first` -> (2 per aperture, n) longdouble
    with the rows (za, zb) per slot, and the pairs' r (slots, n)."""
    rows, rr = [], []
    for slot in range(len(sc.apertures)):
        za, zb, r = normal_pair(seed, first + np.arange(n), slot)
        rows += [za, zb]
        rr.append(r)
    return np.array(rows), np.array(rr)


def injected(sc: Scene, inp: dict, seed: int, n_index) -> np.ndarray:
    """The normals a launch is given: float64(normal_pair), rows (za, zb) per slot.  `tiny` rays: scaled so that the bend
    |s' x s| ~ |(ta, tb)| is 2^-t, t spread evenly over 20 .. 48."""
    n = inp["s0"].shape[0]
    rows, _ = pairs(sc, n, seed)
    if "tiny" in sc.classes:
        surf = sc.apertures[0]
        hit, _ = hit_point(inp, surf.z)
        res = bend(hit[:, 0], hit[:, 1], inp["s0"], None, inp["w0"], inp["wl"], n_index, rows[0], rows[1], surf, factor_of(sc))
        t = 20 + 28 * (np.arange(n) % N_CLASS) / (N_CLASS - 1)
        scale = np.where(cls_mask(sc, inp, "tiny"), LD(2.0) ** -t / np.sqrt(res["ta"] ** 2 + res["tb"] ** 2), 1)
        rows[:2] = rows[:2] * scale
    return rows.astype(np.float64)


# ---- scenes in the package ----------------------------------------------------------------------------------------------
def medium(ot, key: str):
    if key == "abbe":
        return ot.RefractionIndex("Abbe", n=1.5, V=40)
    return ot.RefractionIndex("Constant", n=float(key))


def surface(ot, surf: Surf):
    if surf.kind == "ring":
        return ot.RingSurface(r=surf.r, ri=surf.ri)
    sf = ot.SlitSurface(dim=list(surf.dim), dimi=list(surf.dimi))
    if surf.rot:
        sf.rotate(surf.rot[0])
    return sf


def raytracer(ot, sc: Scene, no_pol: bool = False, seed: int = SEED):
    RT = ot.Raytracer(outline=list(sc.outline), n0=medium(ot, sc.medium), use_hurb=True, no_pol=no_pol, seed=seed)
    RT.add(ot.RaySource(ot.Point(), divergence="Isotropic", div_angle=5, pos=[0, 0, -10],
                        spectrum=ot.LightSpectrum("Monochromatic", wl=550.)))
    for surf in sc.apertures:
        ap = ot.Aperture(surface(ot, surf), pos=[surf.pos[0], surf.pos[1], surf.z])
        if surf.rot:
            ap.rotate(surf.rot[1])
            assert float(ap.front._angle) == angle_of(surf)
        RT.add(ap)
    if sc.factor is not None:
        RT.HURB_FACTOR = sc.factor
    return RT


def oracle_trace(RT, inp: dict, hurb_normals):
    """The rays of `inp` through the C oracle with injected normals -> (HostRays, counters)."""
    from optrace_amd.scene import CompiledScene
    import oracle_bridge as ob
    csc = CompiledScene(RT)
    rays = ob.HostRays(inp["s0"].shape[0], csc.nt, RT.no_pol)
    rays.set_initial(inp["p0"], inp["s0"], None if RT.no_pol else inp["pol0"], inp["w0"], inp["wl"])
    msgs, st = ob.trace(csc.desc, rays, hurb_normals)
    assert st == 0
    return rays, msgs


# ---- comparison ------------------------------------------------------------------------------------------------------
def evaluate(sc: Scene, inp: dict, p_list, pol_list, w_list, n_index, nrm, rr=None) -> list:
    """bend() per aperture from the stored sections of a run -- the hit points p_list[:, 1 + slot], pol_list[:, slot] (None:
    no_pol) and w_list[:, slot] in front of it -- and the normals nrm (rows za, zb per slot; float64 or longdouble) -> one
    result dict per aperture.  The direction between two apertures is stored nowhere: the second one's input is the first
    one's exact s', and its bar carries the first one's, amplified.  rr: the pairs' r where the device drew the normals itself:
    the bar is widened by the draw's own rounding."""
    out = []
    s, carried = inp["s0"].astype(LD), 0
    for slot, surf in enumerate(sc.apertures):
        res = bend(p_list[:, 1 + slot, 0], p_list[:, 1 + slot, 1], s, None if pol_list is None else pol_list[:, slot], w_list[:, slot],
                   inp["wl"], n_index, nrm[2 * slot], nrm[2 * slot + 1], surf, factor_of(sc))
        if rr is not None:
            res["bar_s"] = res["bar_s"] + res["draw_gain"] * rr[slot]
        res["bar_s"] = np.where(res["bent"], res["bar_s"] + res["amplify"] * carried, carried)
        res["open"] = res["open"] | (np.abs(res["s_"][:, 2]) <= res["bar_s"])
        out.append(res)
        s, carried = res["s_"], res["bar_s"]
    return out


def ratios(sc: Scene, inp: dict, res: dict, s_got, pol_got) -> list:
    """Errors of a result (s_got (n, 3) f64, pol_got (n, 3) f32 or None) against the exact values `res` of the aperture that
    bent last, per class, over the rays it bent and whose verdict is not open: rows dict(cls, n, s_abs, s_over, pol_abs,
    pol_over, pol_over_noisy, open).  pol_over leaves out nothing; for the host test `pol_over_noisy` is the same figure
    over the rays with a bend below 2^-25 alone, where the reference's own projection form is noise."""
    rows = []
    for ci, cls in enumerate(sc.classes):
        sel = (inp["cls"] == ci) & res["bent"] & ~res["open"]
        row = dict(cls=cls, n=int(np.count_nonzero(sel)), s_abs=0.0, s_over=0.0, pol_abs=0.0, pol_over=0.0, pol_over_noisy=0.0,
                   open=int(np.count_nonzero((inp["cls"] == ci) & res["open"])), finite=True)
        if row["n"]:
            err = np.abs(s_got[sel].astype(LD) - res["s_"][sel])
            bar = res["bar_s"][sel]
            row.update(s_abs=float(err.max()), s_over=float(np.max(err / bar[:, None])), finite=bool(np.all(np.isfinite(s_got[sel]))))
            if pol_got is not None:
                err = np.abs(pol_got[sel].astype(LD) - res["pol_"][sel]) / (pol_bar(res["a"][sel]) + res["pol_gain"][sel] * bar)[:, None]
                small = res["a"][sel] < 2.0 ** -25
                row.update(pol_abs=float(np.abs(pol_got[sel].astype(LD) - res["pol_"][sel]).max()), pol_over=float(err.max()),
                           pol_over_noisy=float(err[small].max(initial=0.0)),
                           finite=row["finite"] and bool(np.all(np.isfinite(pol_got[sel]))))
        rows.append(row)
    return rows


def format_rows(title: str, rows: list) -> str:
    return "\n".join(f"{title:24s} {r['cls']:9s} n={r['n']:4d} open={r['open']}  s' abs {r['s_abs']:.2e} ({r['s_over']:.3f} of bar)  "
                     f"pol' abs {r['pol_abs']:.2e} ({r['pol_over']:.3f} of bar)" for r in rows)


OPEN_CAP = {"middle": 0, "centre": 0, "steep": 0, "tiny": 0}   # every edge / corner class: 2


def open_cap(cls: str) -> int:
    return OPEN_CAP.get(cls, 2)
