"""Inputs for the part of the trace step that deals with rays which MISS a surface: where such a ray is left, whether it
keeps its weight, the outline clip (outline_clip of csrc/ot_trace.hpp, Raytracer.__outline_intersection of the reference)
and the counter rows all of that lands in.  Shared by the fixture generator tests/golden/generate_golden_wavelength.py
(run on the reference), tests/test_outline_host.py and tests/test_gpu_outline_step.py.

A *scene* is one tested element in a constant ambient inside the tight, asymmetric box OUTLINE (the six walls are
distinguishable), with a small constant filter far behind it, so that the next section of a ray that kept its weight is
observable, and the absorber the tracer puts on the box's +z wall:
  lens      a plate of two flat discs (front and back are separate steps)
  ideal     an ideal lens, off-centre
  filter    a disc, T = 0.5
  aperture  a ring, HURB off
All surfaces are flat, so every hit point is p + s ((z - p_z) / s_z) in the reference's operation order and everything
compared here is bitwise.

A *class* is a family of rays (N_CLASS each; `mixed` has three blocks of 64):
  mixed        block 0 and 2: hits.  Block 1: hits, misses inside the box, clipped rays and dead rays interleaved lane by lane
               -- the two sides of the wave-wide test the device counts its rare events behind.  The class comes first, so
               its blocks are the first three waves.
  hit          aimed at the element's material
  miss_inside  misses the element, the continued point strictly inside the box: lens front and ideal lens kill the ray there,
               filter and aperture keep weight and point; for the lens a part of the class meets the front near its rim
               on the way outwards and misses the back, where the ray is left at its front point; for the aperture a part
               passes the hole
  wall_xlo, wall_xhi, wall_ylo, wall_yhi    misses, continued point outside through the one wall
  wall_zhi     A ray travelling in +z cannot leave through the +z wall at an element: its continued point has the
               element's z, so an x or y wall comes first.  The wall is met at the absorber: rays that pass beside both
               elements nearly parallel to the axis and end on the absorber or (the more tilted half) miss it and are
               clipped in the last step.  Lens and ideal lens kill these rays at the tested element.
  axis0        s_x exactly +0 and exactly -0 (quotients -inf, +inf or the other way round), clipped at a y wall; the same
               for s_y, clipped at an x wall
  on_plane     s_x = +-0 with p_x exactly on an x wall (0 / 0 and +-inf: both dropped, by the NaN rule and by T > 0), the
               same for y; half of them clipped at the other pair of walls, half run on to the +z wall and are clipped there.
               Every fifth leaves its wall inwards with a small s_x instead (|s| = 1 to 2^-15): its quotient for that wall
               is 0 / s_x = +-0, which T > 0 drops and T >= 0 would take, leaving the ray where it started
  edge         aimed from a point whose distances to an x and a y wall are in a power-of-two ratio at the box's edge, so two
               quotients are bitwise equal; and at the +z corners (three equal quotients, met in the absorber's step)
  on_wall      the continued miss point lies exactly on a wall coordinate (the inside test is strict, so it is outside):
               found by a search over start points with the reference's hit-point formula restated below
Every start point lies inside the box (on_plane: on its wall); a start outside is out of contract.  Every eighth ray has
w0 = 0, wl = 550, pol0 a float32-rounded unit vector perpendicular to s0.  The inputs are built from the bit generator with
+, -, *, / and sqrt alone, so that every machine regenerates the same bits.
"""
from __future__ import annotations

import hashlib
from collections import namedtuple

import numpy as np

from focus_cases import write_npz  # noqa: F401  (archives with fixed time stamps)
from refraction_cases import _normalized, _pol_for

OUTLINE = (-3.0, 3.0, -2.0, 2.5, -12.0, 30.0)
WL = 550.0
R_EL = 1.0             # radius of the tested element
R_HOLE = 0.4           # the aperture's inner radius
PLATE_D = 0.5          # the lens: front at z = -PLATE_D, back at z = +PLATE_D
Z_BEHIND = 20.0        # the filter behind
R_BEHIND = 0.75
T_TESTED, T_BEHIND = 0.5, 0.25
IDEAL_POS = (0.25, -0.125, 0.0)
N_CLASS = 80
CLASSES = ("mixed", "hit", "miss_inside", "wall_xlo", "wall_xhi", "wall_ylo", "wall_yhi", "wall_zhi", "axis0", "on_plane",
           "edge", "on_wall")
SCENES = ("lens", "ideal", "filter", "aperture")
# Raytracer.INFOS
ABSORB_MISSING, TIR, ILL_COND, OUTLINE_INTERSECTION, HURB_NEG_DIR = 0, 1, 2, 3, 4

Scene = namedtuple("Scene", "name z centre kills")   # z of the first tested surface; kills: a miss takes the weight


def scene(name: str) -> Scene:
    return {"lens": Scene("lens", -PLATE_D, (0.0, 0.0), True), "ideal": Scene("ideal", 0.0, IDEAL_POS[:2], True),
            "filter": Scene("filter", 0.0, (0.0, 0.0), False), "aperture": Scene("aperture", 0.0, (0.0, 0.0), False)}[name]


def n_tested(name: str) -> int:
    """Steps of the tested element: its sections are 1 .. n_tested."""
    return 2 if name == "lens" else 1


# ---- inputs ----------------------------------------------------------------------------------------------------------
def flat_hit_point(p, s, z):
    """Surface.find_hit of a flat surface at z, in the reference's operation order (surface.py:321-322)."""
    t = (z - p[:, 2]) / s[:, 2]
    return p + s * t[:, None]


def _annulus(rng, k, r0, r1):
    """k points with r0 <= |xy| <= r1, by rejection from the square."""
    xy = rng.uniform(-r1, r1, (16 * k + 64, 2))
    r2 = xy[:, 0] * xy[:, 0] + xy[:, 1] * xy[:, 1]
    xy = xy[(r2 >= r0 * r0) & (r2 <= r1 * r1)][:k]
    assert xy.shape[0] == k
    return xy


def _start(rng, k, half=0.3, z=(-10.0, -6.0)):
    return np.column_stack((rng.uniform(-half, half, (k, 2)), rng.uniform(z[0], z[1], k)))


def _aimed(p0, target):
    return _normalized(target - p0)


def _at(xy, z):
    return np.column_stack((xy, np.full(xy.shape[0], z)))


def _hits(sc, rng, k):
    p0 = _start(rng, k)
    return p0, _aimed(p0, _at(_annulus(rng, k, 0.55, 0.85) + sc.centre, sc.z))


def _beside(sc, rng, k):
    """Targets in the element's plane, inside the box with a margin, more than 1.15 away from the element's centre."""
    xy = np.column_stack((rng.uniform(-2.8, 2.8, 16 * k), rng.uniform(-1.8, 2.3, 16 * k)))
    d = xy - sc.centre
    xy = xy[d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] > 1.15 * 1.15][:k]
    assert xy.shape[0] == k
    p0 = _start(rng, k)
    return p0, _aimed(p0, _at(xy, sc.z))


def _miss_inside(sc, rng, k):
    p0, s = _beside(sc, rng, k)
    if sc.name == "lens":      # from just in front of the plate through the rim zone of its front: misses the back
        j = k // 2
        q0 = np.column_stack((rng.uniform(-0.05, 0.05, (j, 2)), rng.uniform(-1.3, -1.1, j)))
        p0[:j], s[:j] = q0, _aimed(q0, _at(_annulus(rng, j, 0.9, 0.97), sc.z))
    if sc.name == "aperture":  # through the hole
        j = k // 2
        q0 = _start(rng, j)
        p0[:j], s[:j] = q0, _aimed(q0, _at(_annulus(rng, j, 0.0, 0.3), sc.z))
    return p0, s


def _wall(sc, rng, k, wall):
    """Targets in the element's plane beyond one wall, inside the other pair."""
    far, x_in, y_in = rng.uniform(0.2, 3.0, k), rng.uniform(-2.5, 2.5, k), rng.uniform(-1.5, 2.0, k)
    xy = {"xlo": (OUTLINE[0] - far, y_in), "xhi": (OUTLINE[1] + far, y_in), "ylo": (x_in, OUTLINE[2] - far),
          "yhi": (x_in, OUTLINE[3] + far)}[wall]
    p0 = _start(rng, k)
    return p0, _aimed(p0, _at(np.column_stack(xy), sc.z))


def _wall_zhi(sc, rng, k):
    p0 = np.column_stack((rng.uniform(1.5, 2.0, k), rng.uniform(1.0, 1.5, k), rng.uniform(-10.0, -8.0, k)))
    sign = np.where(rng.random((k, 2)) < 0.5, -1.0, 1.0)
    off = rng.uniform(0.0, 0.12, (k, 2))
    off[k // 2:] = rng.uniform(0.3, 0.5, (k - k // 2, 2))   # leaves the box between the filter behind and the absorber
    off[k // 2:, 0] = np.abs(off[k // 2:, 0])
    return p0, _aimed(p0, _at(p0[:, :2] + sign * off * [1.0, 1.0], sc.z))


def _axis0(sc, rng, k):
    p0, s = _start(rng, k), np.zeros((k, 3))
    q = k // 4
    for j, (comp, zero) in enumerate(((0, 0.0), (0, -0.0), (1, 0.0), (1, -0.0))):
        sl = slice(j * q, (j + 1) * q if j < 3 else k)
        m = p0[sl].shape[0]
        other = 1 - comp
        lo, hi = (OUTLINE[2], OUTLINE[3]) if other == 1 else (OUTLINE[0], OUTLINE[1])
        far = rng.uniform(0.2, 3.0, m)
        t = np.where(rng.random(m) < 0.5, lo - far, hi + far)   # beyond a wall of the other pair
        v = np.zeros((m, 3))
        v[:, other], v[:, 2] = t - p0[sl, other], sc.z - p0[sl, 2]
        s[sl] = _normalized(v)
        s[sl, comp] = zero
    return p0, s


def _on_plane(sc, rng, k):
    p0, s = _start(rng, k), np.zeros((k, 3))
    q = k // 4
    walls = ((0, OUTLINE[0]), (0, OUTLINE[1]), (1, OUTLINE[2]), (1, OUTLINE[3]))
    for j, (comp, wall) in enumerate(walls):
        sl = slice(j * q, (j + 1) * q if j < 3 else k)
        m = p0[sl].shape[0]
        other = 1 - comp
        lo, hi = (OUTLINE[2], OUTLINE[3]) if other == 1 else (OUTLINE[0], OUTLINE[1])
        far = rng.uniform(0.2, 3.0, m)
        t = np.where(rng.random(m) < 0.5, lo - far, hi + far)
        t[m // 2:] = p0[sl, other][m // 2:] + rng.uniform(-0.02, 0.02, m - m // 2)   # runs on to the +z wall
        v = np.zeros((m, 3))
        v[:, other], v[:, 2] = t - p0[sl, other], sc.z - p0[sl, 2]
        s[sl] = _normalized(v)
        s[sl, comp] = np.where(np.arange(m) % 2 == 0, 0.0, -0.0)
        inward = np.arange(m) % 5 == 4     # leaves its wall inwards: the quotient is 0 / s = +-0, no T > 0
        s[sl, comp] = np.where(inward, (-1.0 if wall > 0 else 1.0) * 2.0 ** -7, s[sl, comp])
        p0[sl, comp] = wall
    return p0, s


def _edge(sc, rng, k):
    """v = (dx, dy, dz) with |dx| / |dy| a power of two and dx, dy the exact distances to an x and a y wall: the two
    components of s = v / |v| differ by that factor exactly, so the two quotients are the same double."""
    starts = (((0.0, 1.0), (3.0, 1.5)), ((0.0, 1.0), (-3.0, 1.5)), ((0.0, 1.0), (3.0, -3.0)), ((0.0, 1.0), (-3.0, -3.0)),
              ((1.5, -0.5), (1.5, -1.5)), ((1.5, -0.5), (1.5, 3.0)), ((-1.5, 1.75), (-1.5, 0.75)), ((-1.5, 1.75), (4.5, -3.75)))
    corners = (((0.5, 0.0, -10.0), (2.5, 2.5, 40.0)), ((0.5, 1.25, -10.0), (2.5, 1.25, 40.0)), ((-0.5, 0.0, -10.0), (-2.5, 2.5, 40.0)),
               ((0.5, 0.5, -10.0), (2.5, -2.5, 40.0)), ((-2.0, 2.0, -2.0), (-1.0, 0.5, 32.0)), ((2.0, -1.0, -2.0), (1.0, -1.0, 32.0)))
    p0, v = np.zeros((k, 3)), np.zeros((k, 3))
    for i in range(k):
        if i % 10 == 9:
            a, b = corners[(i // 10) % len(corners)]
            p0[i], v[i] = a, b
        else:
            (x0, y0), (dx, dy) = starts[i % len(starts)]
            # (the last start is no power-of-two pair: an ordinary shot at an edge)
            z0 = -10.0 + 0.125 * (i // len(starts))
            p0[i], v[i] = (x0, y0, z0), (dx, dy, 0.5 + 0.375 * (i % 7))
    return p0, _normalized(v)


def _on_wall(sc, rng, k):
    """Start points and directions whose continued point in the element's plane has x or y exactly on a wall: s with
    |s_x| = s_z (or |s_y| = s_z) and start points on a 1/8 grid make the product nearly exact, the search keeps what is."""
    out_p, out_s = [], []
    inv = 1 / np.sqrt(2.0)
    for comp, wall in ((0, OUTLINE[1]), (0, OUTLINE[0]), (1, OUTLINE[3]), (1, OUTLINE[2])):
        sign = 1.0 if wall > 0 else -1.0
        z0 = sc.z - rng.integers(8, 44, 4000) * 0.125           # 1 .. 5.5 in front of the plane
        c0 = wall - sign * (sc.z - z0)                           # so that c0 + sign (z - z0) == wall exactly
        o0 = rng.integers(-8, 9, 4000) * 0.125
        p = np.zeros((4000, 3))
        p[:, comp], p[:, 1 - comp], p[:, 2] = c0, o0, z0
        s = np.zeros((4000, 3))
        s[:, comp], s[:, 2] = sign * inv, inv
        lo, hi = (OUTLINE[0], OUTLINE[1]) if comp == 0 else (OUTLINE[2], OUTLINE[3])
        ok = (flat_hit_point(p, s, sc.z)[:, comp] == wall) & (c0 > lo) & (c0 < hi)
        _, first = np.unique(np.round(z0[ok] * 8), return_index=True)
        sel = np.nonzero(ok)[0][np.sort(first)][:k // 4]
        out_p.append(p[sel])
        out_s.append(s[sel])
    return np.concatenate(out_p), np.concatenate(out_s)


def _mixed(sc, rng):
    p0, s = _hits(sc, rng, 192)
    mi_p, mi_s = _miss_inside(sc, rng, 64)
    cl = [_wall(sc, rng, 16, w) for w in ("xlo", "xhi", "ylo", "yhi")]
    cl_p, cl_s = np.concatenate([c[0] for c in cl]), np.concatenate([c[1] for c in cl])
    for lane in range(64):      # hit, miss inside, clipped, hit (dead every eighth), ...
        r = 64 + lane
        if lane % 4 == 1:
            p0[r], s[r] = mi_p[lane], mi_s[lane]
        elif lane % 4 == 2:
            p0[r], s[r] = cl_p[lane], cl_s[lane]
    return p0, s


def inputs(name: str) -> dict:
    """-> dict(p0 (n, 3) f64, s0 (n, 3) f64, pol0 (n, 3) f32, w0 (n,) f32, wl (n,) f32, cls (n,) index into CLASSES)."""
    sc = scene(name)
    index = SCENES.index(name)
    P, S, C = [], [], []
    for ci, cls in enumerate(CLASSES):
        rng = np.random.default_rng([20251, index, ci])
        if cls == "mixed":
            p0, s = _mixed(sc, rng)
        elif cls == "hit":
            p0, s = _hits(sc, rng, N_CLASS)
        elif cls == "miss_inside":
            p0, s = _miss_inside(sc, rng, N_CLASS)
        elif cls == "wall_zhi":
            p0, s = _wall_zhi(sc, rng, N_CLASS)
        elif cls.startswith("wall_"):
            p0, s = _wall(sc, rng, N_CLASS, cls[5:])
        elif cls == "axis0":
            p0, s = _axis0(sc, rng, N_CLASS)
        elif cls == "on_plane":
            p0, s = _on_plane(sc, rng, N_CLASS)
        elif cls == "edge":
            p0, s = _edge(sc, rng, N_CLASS)
        else:
            p0, s = _on_wall(sc, rng, N_CLASS)
        P.append(p0)
        S.append(s)
        C.append(np.full(p0.shape[0], ci))
    p0, s0, cls = np.concatenate(P), np.concatenate(S), np.concatenate(C)
    if p0.shape[0] % 64 == 0:
        p0, s0, cls = p0[:-1], s0[:-1], cls[:-1]
    rng = np.random.default_rng([20252, index])
    pol0 = _pol_for(s0, rng)
    w0 = rng.uniform(0.25, 1.0, s0.shape[0]).astype(np.float32)
    w0[3::8] = 0.0
    o = OUTLINE
    assert np.all((p0[:, 0] >= o[0]) & (p0[:, 0] <= o[1]) & (p0[:, 1] >= o[2]) & (p0[:, 1] <= o[3]) & (p0[:, 2] > o[4]) & (p0[:, 2] < o[5]))
    return dict(p0=p0, s0=s0, pol0=pol0, w0=w0, wl=np.full(s0.shape[0], WL, dtype=np.float32), cls=cls)


def checksum(inp: dict) -> str:
    h = hashlib.sha256()
    for k in ("p0", "s0", "pol0", "w0", "wl", "cls"):
        h.update(np.ascontiguousarray(inp[k]).tobytes())
    return h.hexdigest()[:16]


def cls_mask(inp: dict, *names) -> np.ndarray:
    return np.isin(inp["cls"], [CLASSES.index(c) for c in names])


# ---- scenes in either package ------------------------------------------------------------------------------------------
VARIANTS = ("plain", "no_pol", "other_form", "asphere_behind", "spline_behind", "data_behind")


def raytracer(ot, name: str, variant: str = "plain", seed=None):
    """The tested element, what stands behind it, and the absorber on the +z wall.  The variants select other template
    instances of the trace kernel; they change nothing about the tested element's sections:
      other_form      a tilted disc behind: its step takes the general surface record, not the compiled hot one
      asphere_behind  a numeric-hit asphere lens behind (ideal lens and filter always compiled in)
      spline_behind   a spline-surface lens behind
      data_behind     a tabulated filter behind (the table kernel)"""
    const = lambda n: ot.RefractionIndex("Constant", n=n)
    kw = {} if seed is None else dict(seed=seed)   # (the product's tracer alone takes a seed)
    RT = ot.Raytracer(outline=list(OUTLINE), n0=const(1.0), no_pol=(variant == "no_pol"), **kw)
    # the source matters to the launches that generate their rays (the render-only form): a cone wide enough that rays hit,
    # miss inside the box and leave through every x and y wall
    RT.add(ot.RaySource(ot.Point(), divergence="Isotropic", div_angle=50, pos=[0.1, 0.2, -4],
                        spectrum=ot.LightSpectrum("Monochromatic", wl=WL)))
    if name == "lens":
        RT.add(ot.Lens(ot.CircularSurface(r=R_EL), ot.CircularSurface(r=R_EL), n=const(1.5), pos=[0, 0, 0], d1=PLATE_D, d2=PLATE_D))
    elif name == "ideal":
        RT.add(ot.IdealLens(r=R_EL, D=25.0, pos=list(IDEAL_POS)))
    elif name == "filter":
        RT.add(ot.Filter(ot.CircularSurface(r=R_EL), pos=[0, 0, 0], spectrum=ot.TransmissionSpectrum("Constant", val=T_TESTED)))
    else:
        RT.add(ot.Aperture(ot.RingSurface(r=R_EL, ri=R_HOLE), pos=[0, 0, 0]))
    if variant == "other_form":
        RT.add(ot.Filter(ot.TiltedSurface(r=R_BEHIND, normal=[0.2, -0.1, 1.0]), pos=[0, 0, Z_BEHIND],
                         spectrum=ot.TransmissionSpectrum("Constant", val=T_BEHIND)))
    elif variant == "asphere_behind":
        RT.add(ot.Lens(ot.AsphericSurface(r=R_BEHIND, R=4, k=-0.8, coeff=[2e-3, -4e-5]), ot.CircularSurface(r=R_BEHIND), de=0.2,
                       n=const(1.6), pos=[0, 0, Z_BEHIND]))
    elif variant == "spline_behind":
        Y, X = np.mgrid[-R_BEHIND:R_BEHIND:60j, -R_BEHIND:R_BEHIND:60j]
        RT.add(ot.Lens(ot.DataSurface2D(r=R_BEHIND, data=X ** 2 / 9 + Y ** 2 / 7), ot.CircularSurface(r=R_BEHIND), de=0.2,
                       n=const(1.6), pos=[0, 0, Z_BEHIND]))
    elif variant == "data_behind":
        RT.add(ot.Filter(ot.CircularSurface(r=R_BEHIND), pos=[0, 0, Z_BEHIND],
                         spectrum=ot.TransmissionSpectrum("Data", wls=np.linspace(380.0, 780.0, 41), vals=np.full(41, T_BEHIND))))
    else:
        RT.add(ot.Filter(ot.CircularSurface(r=R_BEHIND), pos=[0, 0, Z_BEHIND], spectrum=ot.TransmissionSpectrum("Constant", val=T_BEHIND)))
    return RT


def oracle_trace(RT, inp: dict):
    from refraction_cases import oracle_trace as run
    return run(RT, inp)


def bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- the rules in words: what any trace of these scenes has to show ----------------------------------------------------
def strictly_inside(q) -> np.ndarray:
    o = OUTLINE
    return (o[0] < q[:, 0]) & (q[:, 0] < o[1]) & (o[2] < q[:, 1]) & (q[:, 1] < o[3]) & (o[4] < q[:, 2]) & (q[:, 2] < o[5])


RIM_MARGIN = 0.02   # no continued point of any class lies nearer than this to an edge of the tested element's mask


def expected(name: str, inp: dict) -> dict:
    """What the first step has to do with every ray, from the inputs alone: c the continued point in the tested surface's
    plane (the reference's formula, so its bits), hit the verdict of the mask (every class keeps RIM_MARGIN from the
    edges, so rounding does not enter), clip = live, missed and c not strictly inside the box."""
    sc = scene(name)
    c = flat_hit_point(inp["p0"], inp["s0"], sc.z)
    d = np.sqrt((c[:, 0] - sc.centre[0]) ** 2 + (c[:, 1] - sc.centre[1]) ** 2)
    edges = (R_HOLE, R_EL) if name == "aperture" else (R_EL,)
    assert all(np.all(np.abs(d - e) > RIM_MARGIN) for e in edges), name
    hit = (d < R_EL) & ((d > R_HOLE) if name == "aperture" else True)
    live = inp["w0"] > 0
    return dict(c=c, hit=hit, live=live, clip=live & ~hit & ~strictly_inside(c))


def rule_violations(name: str, inp: dict, p, w, msgs, pol=None) -> list:
    """p (n, nt, 3), w (n, nt), msgs (5, nt), pol (n, nt, 3) or None of a trace of scene `name` (any variant) -> the rules
    about missed rays that the result breaks, in words (empty: none)."""
    sc, e, bad = scene(name), expected(name, inp), []
    nt = w.shape[1]
    live, hit, clip = e["live"], e["hit"], e["clip"]
    miss = live & ~hit

    def rule(ok, text):
        if not ok:
            bad.append(text)

    rule(np.all(p[~live] == inp["p0"][~live, None, :]) and np.all(w[~live] == 0), "a ray that is dead on entry never moves")
    if pol is not None:
        rule(all(bits(pol[~live, i], inp["pol0"][~live]) for i in range(nt)), "a ray that is dead on entry keeps its polarisation")
        rule(all(bits(pol[miss, i], inp["pol0"][miss]) for i in range(1 + n_tested(name))),
             "a ray that missed or was clipped keeps its entry polarisation")
    for i in range(1, nt - 1):
        gone = w[:, i] == 0
        rule(bits(p[gone, i + 1], p[gone, i]), f"a ray without weight does not move afterwards (section {i + 1})")
    rule(np.all(w[clip, 1:] == 0), "a clipped ray has weight 0 from the clip on")
    rule(np.all(p[clip, 1:] == p[clip, 1:2]), "a clipped ray does not move afterwards")
    rule(np.all(np.any(p[clip, 1] != inp["p0"][clip], axis=1)), "a clipped ray is moved forward (t > 0), not left at its start")
    walls = np.array(OUTLINE)[[0, 1, 2, 3, 5]]
    q = p[clip, 1][:, [0, 0, 1, 1, 2]]
    rule(np.all(np.any(np.abs(q - walls) <= 4 * np.spacing(np.abs(walls)), axis=1)), "a clipped ray sits on a wall of the box")
    rule(bits(p[live & ~clip, 1], e["c"][live & ~clip]), "a ray that is not clipped sits at its continued point")
    rule(int(msgs[OUTLINE_INTERSECTION, 0]) == np.count_nonzero(clip) and int(msgs[OUTLINE_INTERSECTION, nt - 1]) == 0,
         "OUTLINE_INTERSECTION of step i is counted in row i")
    rule(int(msgs[ABSORB_MISSING, 0]) == 0 and int(msgs[ABSORB_MISSING, 1]) == (np.count_nonzero(miss) if sc.kills else 0),
         "ABSORB_MISSING of step i is counted in row i + 1 (lenses only)")
    if sc.kills:
        rule(np.all(w[miss, 1] == 0), "a lens or ideal-lens miss loses its weight")
    else:
        rule(bits(w[miss & ~clip, 1], inp["w0"][miss & ~clip]), "a filter or aperture miss keeps its weight")
        rule(np.all(msgs[ABSORB_MISSING, :2] == 0), "filters and apertures count no ABSORB_MISSING")
    if name == "lens":
        back_miss = (w[:, 1] > 0) & (w[:, 2] == 0)     # (no total reflection from air into glass, no T == 0)
        rule(bits(p[back_miss, 2], p[back_miss, 1]), "a lens-back miss sits at its section-1 point")
        rule(int(msgs[ABSORB_MISSING, 2]) == np.count_nonzero(back_miss) and int(msgs[OUTLINE_INTERSECTION, 1]) == 0,
             "a lens-back miss is counted in ABSORB_MISSING row 2 and is never clipped")
    return bad
