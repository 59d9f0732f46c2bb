"""Scenes, ray classes, exact intersections and error bars for the surface hit step (find_hit, find_hit_conic,
find_hit_asphere, illinois_search, handle_abnormal_f of csrc/ot_device.hpp), shared by the fixture generator
tests/golden/generate_golden_hit_step.py (run on the reference, with mpmath), tests/test_hit_host.py and
tests/test_gpu_hit_step.py.

A *scene* is one tested surface with its centre at POS -- as a leaf surface (`placed`) and as the front of a lens with a
flat back in constant media (`raytracer`).  A *class* is (surface, family): 97 rays aimed at a target point of the surface
and stepped back along the ray by the family's depth (3 mm unless noted).  Families:
  wide       s = (a, b, sqrt(1 - a^2 - b^2)), a, b uniform in +-0.35
  steep      (a, b, 1) normalised, a, b up to 1.5
  tilt<e>    like wide with a, b up to 2^e: the closed-form conic hit divides a cancelling numerator by A = 1 + k s_z^2, and
             for a paraboloid A = sin^2 of the angle to the axis.  Below 2^-27 s_z rounds to 1 and A == 0 (the linear branch)
  axis       s = (0, 0, 1) bitwise
  cone       k = -7.5: s_z^2 = (1 + delta) / 7.5, delta spread over +-2^-30 and, for every eighth ray, 0 (the nearest
             double to A == 0)
  near, far  depth 1e-3; depth 300 with a, b up to 0.01 and |s|^2 = 1 to 1e-20 (see _unitized)
  inside     start between z_min and z_max, in front of the surface
  on         start 2^-48 mm in front of the (float64) surface point: t ~ 0, the `z1 >= z` rule; on aspheres and the tilted
             surface every other ray starts up to 2^-21 mm (< C_EPS) beyond it: the `t1 < 0 -> -C_EPS` rule makes that a hit
  behind     start above z_max: the start comes back bitwise, not hit
  past       tilted surface: start 0.3 .. 1 mm beyond the plane but below z_max: the plane hit lies behind the start by
             more than C_EPS (handle_abnormal_f's `neg`), so the ray has no hit and ends on z = z_max.  Conics (k = -0.25,
             k = -1): start 0.1 .. 0.4 mm beyond the surface near its vertex: neither root is admissible, the fallback t2
             leaves the z range, no hit -- with the two roots' labels swapped the fallback would be the hit behind the start
  tangent    near-hemisphere: rays in a meridian plane that graze the sphere, D / |B| spread over 2^-4 .. 2^-20
  miss       aimed outside the aperture by 1e-3 .. 1 (ring: also into the hole); on spheres the last five miss the whole
             sphere (no real root)
  rim        aimed at the radius r + N_EPS + delta, delta = +-r 2^-e for e = 20, 30, 36, 40, 44, 48, 52 (ring: also at the
             inner edge ri - N_EPS)
Every eighth ray has w0 = 0.  The inputs are built from the bit generator with +, -, *, / and sqrt alone, so that every
machine regenerates the same bits; `<class>/checksum` of the archive ties them to it.

Truth (`exact_hit`, mpmath at 400 bits, stored as hi + lo): the smallest admissible root of the ray, on the binary values
of p, s and of the surface's parameters (rho = fl(1 / R), k, coefficients, centre, z_min, z_max as the surface carries
them), under the reference's own rules: z inside [z_min - N_EPS, z_max + N_EPS], not behind the start, then the mask
r^2 <= fl(r + N_EPS)^2 (ring: and >= fl(ri - N_EPS)^2).  Conics and planes from the quadratic with the geometric
A = s_x^2 + s_y^2 + (k + 1) s_z^2; aspheres, and rays that miss a tilted disc (they meet its radially continued edge),
from a bracketed root of z(t) - values(x(t), y(t)), values as the reference composes it (sag inside the mask, the edge value
outside).  A ray without a hit ends on z = z_max (closed forms) or on that continued surface (numeric); one that starts
above z_max keeps its start.

Bars, per ray and coordinate, u = 2^-53, o = start - centre, p the exact point, t the exact parameter:
  closed form   K u (|p|_inf + |o|_2 + |t|)                  (flat, conic, the plane hit of a tilted surface, no-hit points)
  tangent       the same times the exact |B| / D, the true sensitivity of a grazing intersection to its inputs
  numeric       1e-7 |s_j| + the closed-form bar; 1e-7 = C_EPS / 10 is the bracket width at which illinois_search leaves
There is no factor 1 / A and no term in R: the cancellation of (-B -+ D) / A is avoidable, so it is no part of the contract.
K = 32.  Roundings of the kernel's chain (find_hit_conic after this pin: q = -(B + sign(B) D), roots q / A and C / q):
o 3; rho and 1 / rho, 2 / rho 3; oz k1 1; B: one difference, three products, two sums 6; C: one difference, three products,
two sums 6; A 3; B B - C A 3; the root 1; q 1; the two quotients (ot_div: one unit each) 2; p + s t 2 -- 31, each on a
quantity whose share of the result is at most |o| or |t| relative, and one for the parameters of the truth itself.
Spheres of |R| <= 4096 mm keep the reference's -B -+ D, bit for bit.  The trace kernel is bound by f64 issue: the quotient
C / q cost the double-Gauss benchmark 4.3 % when every sphere took it and 2.1 % when its four surfaces of |R| > 256 mm did
(R = 469.5, 284.6, -2907 twice; six interleaved rounds each, profiles/hit_step), and no change may slow that kernel.  With
A = 1 nothing divides the reference's numerator, it only loses up to 2 u |R|: at most 2^-40 mm below the threshold, and below
u |o| for the spheres of these classes (R = 8, -5, 5).  The spheres R = 1e4 and 1e7, where the loss was 17 and 1.9e4 bars
before (sph1e4/steep, sph1e7/steep), take the stable roots.  This is a limit of the contract, not of the test: between some 600 mm and 4096 mm a sphere
may miss this bar (which has no term in R) by up to 2 u |R| / bar ~ 20, i.e. by 9e-13 mm; no class stands there.

`far` stands on the flat sphere R = 1e4, on the paraboloid and on an asphere, not on the sphere R = 8.  There the closed
form's discriminant B B - C (A = 1) is a difference of two numbers of size |o|^2 that leaves D^2 ~ R^2: D loses
u |o|^2 / (2 D) per rounding, which at 300 mm is some 2e-12 mm, about one bar -- 2.5e-12 mm = 1.2 bars on 97 such rays, alike for
the reference, for the kernel before this pin and for stable_form, while the class was tried; it is not in the archive -- and at the 5e4 mm of a distant object some 1e-8 mm.  It is avoidable (the terms of second
order in o are -|s x o|^2 by Lagrange's identity; that form measured 0.04 of the bar here), but the kernel that avoids it
no longer agrees with the reference's recorded traces of scenes with distant sources to the 1e-9 the existing parity checks
ask for, so D stays the reference's and the limit is recorded instead of pinned: the bar K u (|p| + |o| + |t|) holds for
starts up to ~30 D in front of a surface.

Verdicts.  Outside `rim` the exact hit radius is at least 1e-6 away from r + N_EPS (and from ri - N_EPS); the generator
asserts that, and every is_hit must equal the exact verdict.  Within `rim` a ray whose |delta| exceeds four times its bar
is decided the same way; the others are held to self-consistency only (`undecided`).
"""
from __future__ import annotations

import hashlib

import numpy as np

from focus_cases import write_npz  # noqa: F401  (archives with fixed time stamps)

LD = np.longdouble
U = 2.0 ** -53
K = 32
N_EPS, C_EPS = 1e-10, 1e-6
POS = (0.3, -0.2, 5.0)
N_RAYS = 97
DEPTH = 3.0
D1, D2 = 1.5, 7.0     # the lens: front vertex at POS, flat back at POS_z + D1 + D2
WL = 550.0
MP_PREC = 400
RIM_E = (20, 30, 36, 40, 44, 48, 52)
LADDER = (-4, -8, -12, -16, -20, -24, -28, -40)


def _geometric(r, n, a0, q):
    """a_j = a0 q^j / r^(2j) by repeated products (no pow)."""
    out, a = [], a0
    for _ in range(n):
        out.append(a)
        a = a * q / (r * r)
    return out


SURFACES = {
    "sph8": dict(kind="conic", r=3.0, R=8.0, k=0.0),
    "sph_m5": dict(kind="conic", r=2.0, R=-5.0, k=0.0),
    "sph1e4": dict(kind="conic", r=3.0, R=1e4, k=0.0),
    "sph1e7": dict(kind="conic", r=3.0, R=1e7, k=0.0),
    "hemi": dict(kind="conic", r=4.999, R=5.0, k=0.0),
    "con_m025": dict(kind="conic", r=3.0, R=7.8, k=-0.25),
    "con_m75": dict(kind="conic", r=3.0, R=12.0, k=-7.5),
    "con_p3": dict(kind="conic", r=2.0, R=-9.0, k=3.0),
    "par6": dict(kind="conic", r=3.0, R=6.0, k=-1.0),
    "par_m6": dict(kind="conic", r=3.0, R=-6.0, k=-1.0),
    "par1e5": dict(kind="conic", r=3.0, R=1e5, k=-1.0),
    "par1e7": dict(kind="conic", r=3.0, R=1e7, k=-1.0),
    "near_par": dict(kind="conic", r=3.0, R=6.0, k=-1.0000001),
    "asph_a": dict(kind="asphere", r=4.0, R=12.0, k=-0.8, coeff=[2e-3, -4e-5, 3e-7]),
    "asph_b": dict(kind="asphere", r=3.0, R=-15.0, k=0.3, coeff=[-1e-3, 2e-5]),
    "asph_c5": dict(kind="asphere", r=4.0, R=-16.0, k=2.0, coeff=[-8e-4, 2e-5, -3e-7, 2e-9, -5e-12]),
    "asph_n13": dict(kind="asphere", r=2.5, R=8.0, k=-2.5, coeff=_geometric(2.5, 13, 1e-3, -0.6)),
    "asph_par": dict(kind="asphere", r=3.0, R=1e9, k=-1.0, coeff=[1 / 12]),
    "tilted": dict(kind="tilted", r=3.0, normal=[0.0, -0.45, float(np.sqrt(1 - 0.45 * 0.45))]),
    "circle": dict(kind="circle", r=2.5),
    "ring": dict(kind="ring", r=3.0, ri=0.7),
}

# the paraboloid of scenes.surface_zoo, whose fixture rays (tests/golden/leaf_surfaces.npz, 1500 random rays) the reference
# itself misses by more than the 1e-12 of tests/test_gpu_parity.py::test_find_hit wherever their tilt is small: the
# archive carries the exact hits of exactly those rays (`zoo_parab/idx`), see zoo_parab_check
SURFACES["zoo_parab"] = dict(kind="conic", r=3.0, R=6.0, k=-1.0)
PLAIN_SPHERE_R = 4096.0   # OT_PLAIN_SPHERE_R of csrc/ot_device.hpp
ZOO_TOL = 1e-12   # atol = rtol of the comparisons with the reference's fixture and with the oracle

_T = tuple(f"tilt{e}" for e in LADDER)
PLAN = {
    # (no `far` on this sphere: see the module's docstring)
    "sph8": ("wide", "steep") + _T + ("axis", "near", "inside", "on", "behind", "miss", "rim"),
    "sph_m5": ("wide", "steep", "on", "miss"),
    "sph1e4": ("wide", "steep", "near", "far"),
    "sph1e7": ("wide", "steep", "on"),
    # (no `rim` here: at the rim of the near-hemisphere a ray along the axis grazes the surface, |B| / D ~ 30, which is the
    # subject of `tangent` and its bar)
    "hemi": ("wide", "steep", "tangent", "inside", "miss"),
    "con_m025": ("wide", "near", "miss"),
    "con_m75": ("wide", "cone", "miss"),
    "con_p3": ("wide", "on", "miss"),
    "par6": ("wide",) + _T + ("axis", "near", "far", "inside", "on", "behind", "miss", "rim"),
    "par_m6": ("wide", "tilt-12", "tilt-20", "axis", "on"),
    "par1e5": ("wide", "tilt-12", "tilt-24"),
    "par1e7": ("wide", "tilt-12"),
    "near_par": ("wide", "tilt-4", "tilt-12", "tilt-20", "tilt-28", "tilt-40"),
    "asph_a": ("wide", "steep", "near", "far", "inside", "on", "behind", "miss"),
    "asph_b": ("wide", "steep", "near", "inside", "on", "miss"),
    "asph_c5": ("wide", "steep"),
    "asph_n13": ("wide", "steep"),
    "asph_par": ("wide", "tilt-4", "tilt-12", "tilt-24", "tilt-40", "axis"),
    "tilted": ("wide", "steep", "near", "on", "past", "behind", "miss"),
    "circle": ("wide", "axis", "on", "behind", "miss", "rim"),
    "ring": ("wide", "miss", "rim"),
}
CLASSES = [(sn, fam) for sn, fams in PLAN.items() for fam in fams]
# added later, at the end of CLASSES so that the classes above keep their index and with it their rays: a start beyond a
# non-spherical conic but below z_max, B < 0.  Both roots are inadmissible there and the reference falls back to t2 -- which
# is outside the z range only if the labels t1 = (-B - D) / A, t2 = (-B + D) / A are the reference's, whichever of q / A and
# C / q carries them
EXTRA = {"con_m025": ("past",), "par6": ("past",)}
for _sn, _fams in EXTRA.items():
    CLASSES += [(_sn, _f) for _f in _fams]
    PLAN[_sn] = PLAN[_sn] + _fams


def key(sn: str, fam: str) -> str:
    return f"{sn}/{fam}"


# ---- surfaces and scenes in either package ---------------------------------------------------------------------------
def make_surface(ot, sn: str):
    d = SURFACES[sn]
    with ot.global_options.no_warnings():
        if d["kind"] == "conic":
            if d["k"] == 0.0:
                return ot.SphericalSurface(r=d["r"], R=d["R"])
            return ot.ConicSurface(r=d["r"], R=d["R"], k=d["k"])
        if d["kind"] == "asphere":
            return ot.AsphericSurface(r=d["r"], R=d["R"], k=d["k"], coeff=list(d["coeff"]))
        if d["kind"] == "tilted":
            return ot.TiltedSurface(r=d["r"], normal=list(d["normal"]))
        if d["kind"] == "ring":
            return ot.RingSurface(r=d["r"], ri=d["ri"])
        return ot.CircularSurface(r=d["r"])


def placed(ot, sn: str):
    sf = make_surface(ot, sn)
    sf.move_to(list(POS))
    return sf


def geometry(sf) -> np.ndarray:
    """What the truth needs of a placed surface, as the surface carries it: centre, z_min, z_max, the tilted normal."""
    n = getattr(sf, "normal", None)
    n = [0.0, 0.0, 1.0] if n is None else [float(v) for v in n]
    return np.array([float(v) for v in sf.pos] + [float(sf.z_min), float(sf.z_max)] + n, dtype=np.float64)


TRACED = tuple(sn for sn in PLAN if sn != "ring")   # a ring is no lens front: the leaf operator alone sees it
VARIANTS = ("plain", "asphere_behind", "data2d_behind", "no_pol", "continuous")


def raytracer(ot, sn: str, variant: str = "plain"):
    """The tested surface as the front of a lens (n = 1.5, flat back) in air.  The variants select other template
    instances of the trace kernel (hit levels, polarisation off, a continuous spectrum) around the same sections 0 .. 1."""
    const = lambda n: ot.RefractionIndex("Constant", n=n)
    RT = ot.Raytracer(outline=[-12, 12, -12, 12, -12, 40], n0=const(1.0), no_pol=(variant == "no_pol"))
    # (a monochromatic source is a spectrum of one line: `plain` runs the kernel with line tables, `continuous` the other)
    spectrum = ot.LightSpectrum("Gaussian", mu=540.0, sig=40.0) if variant == "continuous" else \
        ot.LightSpectrum("Monochromatic", wl=WL)
    RT.add(ot.RaySource(ot.Point(), divergence="Isotropic", div_angle=5, pos=[0, 0, -10], spectrum=spectrum))
    r = SURFACES[sn]["r"]
    with ot.global_options.no_warnings():
        RT.add(ot.Lens(make_surface(ot, sn), ot.CircularSurface(r=r), n=const(1.5), pos=[POS[0], POS[1], POS[2] + D1],
                       d1=D1, d2=D2))
        if variant == "asphere_behind":
            RT.add(ot.Lens(ot.AsphericSurface(r=4, R=12, k=-0.8, coeff=[2e-3, -4e-5, 3e-7]), ot.CircularSurface(r=4), de=0.5,
                           n=const(1.6), pos=[0, 0, 20]))
        if variant == "data2d_behind":
            Y, X = np.mgrid[-4:4:200j, -4:4:200j]
            RT.add(ot.Lens(ot.DataSurface2D(r=4.0, data=X ** 2 / 20 + Y ** 2 / 14 + 0.02 * np.sin(2 * X)),
                           ot.CircularSurface(r=4.0), de=0.5, n=const(1.6), pos=[0, 0, 20]))
    return RT


# ---- float64 surface functions (targets only: the truth does not rest on them) ------------------------------------------
def _sag64(d, r2):
    """Sag relative to the centre at squared radius r2 (conic, asphere; 0 for flat kinds; tilted: see _target_z)."""
    if d["kind"] not in ("conic", "asphere"):
        return np.zeros_like(r2)
    rho = 1 / d["R"]
    z = rho * r2 / (1 + np.sqrt(1 - (d["k"] + 1) * rho * rho * r2))
    for j, c in enumerate(d.get("coeff", ())):
        term = c * r2
        for _ in range(j):
            term = term * r2
        z = z + term
    return z


def _target_z(d, x, y):
    if d["kind"] == "tilted":
        n = d["normal"]
        return -(n[0] * x + n[1] * y) / n[2]
    return _sag64(d, x * x + y * y)


def _unit2(rng, k):
    """k points on the unit circle without a trigonometric function."""
    uv = rng.uniform(-1, 1, (4 * k + 64, 2))
    r2 = uv[:, 0] * uv[:, 0] + uv[:, 1] * uv[:, 1]
    keep = (r2 <= 1) & (r2 >= 0.01)
    uv, r2 = uv[keep][:k], r2[keep][:k]
    assert uv.shape[0] == k
    return uv[:, 0] / np.sqrt(r2), uv[:, 1] / np.sqrt(r2)


def _in_disc(rng, k, lo, hi):
    """k points with radius in [lo, hi] (uniform radius), relative to the centre."""
    c, s = _unit2(rng, k)
    rad = rng.uniform(lo, hi, k)
    return rad * c, rad * s


def _small(rng, k, amp):
    a, b = rng.uniform(-amp, amp, k), rng.uniform(-amp, amp, k)
    return np.stack((a, b, np.sqrt(1 - a * a - b * b)), axis=1)


def _unitized(s):
    """|s|^2 = 1 to some 1e-20 instead of 1e-16: s_x moves by whole units in its last place until the exact (rational)
    sum of squares is as close to 1 as they allow.  The closed forms take s for a unit vector; at t = 300 the 2^-53 a
    rounded normalisation leaves in |s|^2 - 1 would move the hit by t^2 / (2 D) times that, which is the input's error and
    not the kernel's."""
    from fractions import Fraction
    out = s.copy()
    for i in range(s.shape[0]):
        a, b, c = (Fraction(float(v)) for v in s[i])
        ulp = Fraction(float(np.spacing(abs(s[i, 0]))))
        j = round((1 - (a * a + b * b + c * c)) / (2 * abs(a) * ulp))
        out[i, 0] = float(a + (j if a > 0 else -j) * ulp)
    return out


def _normalized(v):
    return v / np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2 + v[:, 2] ** 2)[:, None]


def inputs(sn: str, fam: str) -> dict:
    """-> dict(p0 (n, 3), s0 (n, 3) f64, pol0 (n, 3) f32, w0, wl (n,) f32, aim (n,) f64: the aimed delta of `rim`, else 0)."""
    d = SURFACES[sn]
    n, r = N_RAYS, d["r"]
    rng = np.random.default_rng([20250, CLASSES.index((sn, fam))])
    pos = np.array(POS)
    depth = np.full(n, DEPTH)
    aim = np.zeros(n)
    x, y = _in_disc(rng, n, 0.0, 0.8 * r)
    if d["kind"] == "ring":
        x, y = _in_disc(rng, n, d["ri"] + 0.05, 0.8 * r)
    s = _small(rng, n, 0.35)
    if fam == "wide":
        pass
    elif fam == "steep":
        x, y = 0.5 * x, 0.5 * y
        ab = rng.uniform(-1.5, 1.5, (n, 2))
        s = _normalized(np.column_stack((ab, np.ones(n))))
    elif fam.startswith("tilt"):
        s = _small(rng, n, 2.0 ** int(fam[4:]))
    elif fam == "axis":
        s = np.tile([0.0, 0.0, 1.0], (n, 1))
    elif fam == "cone":
        x, y = 0.5 * x, 0.5 * y
        delta = rng.uniform(-1, 1, n) * 2.0 ** -30
        delta[::8] = 0.0
        sz2 = (1 + delta) / 7.5
        c, sn_ = _unit2(rng, n)
        st = np.sqrt(1 - sz2)
        s = np.stack((st * c, st * sn_, np.sqrt(sz2)), axis=1)
    elif fam == "near":
        depth[:] = 1e-3
    elif fam == "far":
        depth[:] = 300.0
        s = _unitized(_small(rng, n, 0.01))
    elif fam == "inside":
        s = _small(rng, n, 0.1)
        x, y = _in_disc(rng, n, 0.3 * r, 0.6 * r)
        zt = _target_z(d, x, y)
        zlow = min(0.0, float(_sag64(d, np.array(r * r))))   # z_min relative to the centre
        depth = rng.uniform(0.2, 0.8, n) * (zt - zlow) / s[:, 2]
    elif fam == "on":
        depth[:] = 2.0 ** -48
        if d["kind"] == "conic" and d["k"] == -1.0:
            s[::4] = [0.0, 0.0, 1.0]   # A == 0
        if d["kind"] in ("asphere", "tilted"):   # the numeric search starts at -C_EPS, the plane hit may lie C_EPS behind
            depth[1::2] = -rng.uniform(0.5, 1.0, n)[1::2] * 2.0 ** -21
    elif fam == "behind":
        zhigh = max(0.0, float(_sag64(d, np.array(r * r))))
        if d["kind"] == "tilted":
            zhigh = 0.45 / d["normal"][2] * r
        depth = -(zhigh - _target_z(d, x, y) + rng.uniform(1e-3, 1.0, n)) / s[:, 2]
    elif fam == "past" and d["kind"] == "conic":
        x, y = 0.25 * x, 0.25 * y   # near the vertex: the start, 0.1 .. 0.4 mm beyond the surface, stays below z_max
        depth = -rng.uniform(0.1, 0.4, n)
    elif fam == "past":
        y = -np.abs(y)   # the low half of the tilted disc: z_t <= centre, start below z_max = centre + 0.504 r
        depth = -rng.uniform(0.3, 1.0, n)
    elif fam == "tangent":
        R = d["R"]
        ct = rng.uniform(0.4, 0.85, n)           # polar angle of the grazing point, from the vertex
        st = np.sqrt(1 - ct * ct)
        c, sn_ = _unit2(rng, n)
        ratio = np.ldexp(1 + rng.random(n), -rng.integers(5, 21, n))   # D / |B| = R sin(alpha) / (R sin(alpha) + depth)
        tau = DEPTH * ratio / (1 - ratio) / R
        x, y = R * st * c, R * st * sn_
        tang = np.stack((ct * c, ct * sn_, st), axis=1)
        inward = np.stack((-st * c, -st * sn_, ct), axis=1)
        s = _normalized(tang + tau[:, None] * inward)
    elif fam == "miss":
        x, y = _in_disc(rng, n, r + N_EPS + 1e-3, r + N_EPS + 1.0)
        if d["kind"] == "ring":
            xi, yi = _in_disc(rng, n, 0.0, d["ri"] - N_EPS - 1e-3)
            x[::2], y[::2] = xi[::2], yi[::2]
        if d["kind"] == "conic" and d["k"] == 0.0 and abs(d["R"]) < 100:
            c, sn_ = _unit2(rng, 5)
            x[-5:], y[-5:] = 1.3 * abs(d["R"]) * c, 1.3 * abs(d["R"]) * sn_   # (inside the outline of `raytracer`)
            s[-5:] = _small(rng, 5, 0.01)
    elif fam == "rim":
        c, sn_ = _unit2(rng, n)
        e = np.array(RIM_E)[np.arange(n) % len(RIM_E)]
        sign = np.where((np.arange(n) // len(RIM_E)) % 2 == 0, 1.0, -1.0)
        aim = sign * np.ldexp(r, -e)
        rad = r + N_EPS + aim
        if d["kind"] == "ring":   # every other pair of rungs goes to the inner edge
            inner = (np.arange(n) // (2 * len(RIM_E))) % 2 == 1
            aim = np.where(inner, sign * np.ldexp(d["ri"], -e), aim)
            rad = np.where(inner, d["ri"] - N_EPS + aim, rad)
        x, y = rad * c, rad * sn_
    else:
        raise ValueError(fam)
    if fam in ("miss", "rim") and d["kind"] in ("conic", "asphere"):
        rr = np.minimum(x * x + y * y, (r - N_EPS) ** 2) if fam == "miss" else x * x + y * y
        z = _sag64(d, rr)
    else:
        z = _target_z(d, x, y)
    target = np.column_stack((x, y, z)) + pos
    p0 = target - depth[:, None] * s
    rng = np.random.default_rng([20251, CLASSES.index((sn, fam))])
    helper = np.array([1.0, 0.0, 0.0])
    e1 = _normalized(np.cross(s, helper[None, :]))
    e2 = np.cross(s, e1)
    c, sn_ = _unit2(rng, n)
    pol0 = (c[:, None] * e1 + sn_[:, None] * e2).astype(np.float32)
    w0 = rng.uniform(0.25, 1.0, n).astype(np.float32)
    w0[3::8] = 0.0
    assert n % 64 != 0
    return dict(p0=np.ascontiguousarray(p0), s0=np.ascontiguousarray(s), pol0=pol0, w0=w0,
                wl=np.full(n, WL, dtype=np.float32), aim=aim)


def checksum(inp: dict) -> str:
    h = hashlib.sha256()
    for k in ("p0", "s0", "pol0", "w0", "wl"):
        h.update(np.ascontiguousarray(inp[k]).tobytes())
    return h.hexdigest()[:16]


# ---- exact values (mpmath, where it is installed) ------------------------------------------------------------------------
def _mp():
    import mpmath
    mpmath.mp.prec = MP_PREC
    return mpmath


def _composite64(d, geom):
    """float64 values(x, y) of an asphere or tilted surface as the reference composes it: for locating the bracket only."""
    px, py, pz = geom[:3]
    r, re2 = d["r"], (d["r"] + N_EPS) ** 2

    def values(x, y):
        dx, dy = x - px, y - py
        r2 = dx * dx + dy * dy
        inside = r2 <= re2
        if d["kind"] == "tilted":
            rr = np.sqrt(r2)
            sc = np.where(inside, 1.0, (r - N_EPS) / np.where(rr > 0, rr, 1.0))
            return pz + _target_z(d, dx * sc, dy * sc)
        with np.errstate(invalid="ignore"):
            return pz + np.where(inside, _sag64(d, np.minimum(r2, re2)), _sag64(d, np.array((r - N_EPS) ** 2)))
    return values


class Exact:
    """Exact arithmetic on one placed surface: SURFACES[sn] and the geometry record of the archive."""

    def __init__(self, sn: str, geom):
        self.mp = mp = _mp()
        f = mp.mpf
        self.sn, self.d, self.geom = sn, SURFACES[sn], np.asarray(geom, dtype=np.float64)
        d = self.d
        self.pos = [f(float(v)) for v in geom[:3]]
        self.z_min, self.z_max = f(float(geom[3])), f(float(geom[4]))
        self.normal = [f(float(v)) for v in geom[5:8]]
        self.ne = f(N_EPS)
        self.re2 = f(d["r"] + N_EPS) ** 2
        self.ri2 = f(d["ri"] - N_EPS) ** 2 if d["kind"] == "ring" else None
        if d["kind"] in ("conic", "asphere"):
            self.rho = f(1 / d["R"])
            self.k1 = f(d["k"]) + 1
            self.coeff = [f(float(c)) for c in d.get("coeff", ())]

    # -- surface functions
    def sag(self, r2):
        mp = self.mp
        z = self.rho * r2 / (1 + mp.sqrt(1 - self.k1 * self.rho ** 2 * r2))
        term = r2
        for c in self.coeff:   # a_j r^(2j + 2)
            z += c * term
            term = term * r2
        return z

    def mask(self, x, y) -> bool:
        r2 = (x - self.pos[0]) ** 2 + (y - self.pos[1]) ** 2
        return bool(r2 <= self.re2 and (self.ri2 is None or r2 >= self.ri2))

    def radius(self, x, y):
        return self.mp.sqrt((x - self.pos[0]) ** 2 + (y - self.pos[1]) ** 2)

    def values(self, x, y):
        """The reference's Surface.values of a numeric surface: sag inside the mask, the continued edge outside."""
        mp, f = self.mp, self.mp.mpf
        dx, dy = x - self.pos[0], y - self.pos[1]
        r2 = dx * dx + dy * dy
        re = f(self.d["r"] - N_EPS)
        if self.d["kind"] == "tilted":
            if r2 > self.re2:
                rr = mp.sqrt(r2)
                dx, dy = re * dx / rr, re * dy / rr
            return self.pos[2] - (self.normal[0] * dx + self.normal[1] * dy) / self.normal[2]
        return self.pos[2] + (self.sag(r2) if r2 <= self.re2 else self.sag(re * re))

    def residual(self, pt):
        """The surface equation at a hit point (truth self-check)."""
        d, o = self.d, [pt[c] - self.pos[c] for c in range(3)]
        if d["kind"] in ("circle", "ring"):
            return o[2]
        if d["kind"] == "tilted":
            return sum(self.normal[c] * o[c] for c in range(3))
        if d["kind"] == "conic":   # rho r^2 - 2 z + (k + 1) rho z^2 = 0
            return self.rho * (o[0] ** 2 + o[1] ** 2) - 2 * o[2] + self.k1 * self.rho * o[2] ** 2
        return o[2] - self.sag(o[0] ** 2 + o[1] ** 2)

    def normal_at(self, x, y):
        """Exact unit normal of a conic at (x, y): n_r = -rho r / sqrt(1 - k rho^2 r^2), n_z = sqrt(1 - n_r^2)."""
        mp = self.mp
        dx, dy = x - self.pos[0], y - self.pos[1]
        q = mp.sqrt(1 - (self.k1 - 1) * self.rho ** 2 * (dx * dx + dy * dy))
        nx, ny = -self.rho * dx / q, -self.rho * dy / q
        return [nx, ny, mp.sqrt(1 - nx * nx - ny * ny)]

    # -- the hit
    def hit(self, p, s) -> dict:
        """-> dict(point [3 mpf], t, hit, numeric, cond (|B| / D of a conic hit, else 1), radius)."""
        mp, f, d = self.mp, self.mp.mpf, self.d
        p, s = [f(float(v)) for v in p], [f(float(v)) for v in s]
        along = lambda t: [p[c] + s[c] * t for c in range(3)]
        out = dict(numeric=False, cond=f(1), hit=False)
        z_lo, z_hi = self.z_min - self.ne, self.z_max + self.ne
        kind = d["kind"]
        behind = p[2] > self.z_max if kind == "conic" else p[2] > z_hi
        if behind:
            out.update(point=p, t=f(0), radius=self.radius(p[0], p[1]))
            return out
        t_plane = (self.z_max - p[2]) / s[2]
        if kind in ("circle", "ring"):
            pt = along(t_plane)
            out.update(point=pt, t=t_plane, hit=self.mask(pt[0], pt[1]), radius=self.radius(pt[0], pt[1]))
            return out
        if kind == "conic":
            o = [p[c] - self.pos[c] for c in range(3)]
            irho = 1 / self.rho
            A = s[0] ** 2 + s[1] ** 2 + self.k1 * s[2] ** 2
            B = s[0] * o[0] + s[1] * o[1] + s[2] * (self.k1 * o[2] - irho)
            C = o[0] ** 2 + o[1] ** 2 + o[2] * (self.k1 * o[2] - 2 * irho)
            roots, D = [], None
            if A == 0:
                if B != 0:
                    roots, D = [-C / (2 * B)], abs(B)
            else:
                disc = B * B - A * C
                if disc >= 0:
                    D = mp.sqrt(disc)
                    q = -(B + (D if B >= 0 else -D))
                    roots = [q / A] + ([C / q] if q != 0 else [])
            ok = sorted(t for t in roots if t >= 0 and z_lo <= p[2] + s[2] * t <= z_hi)
            out["radius"] = None   # no admissible root: no radius to compare with the edge of the mask
            if ok:
                pt = along(ok[0])
                out.update(radius=self.radius(pt[0], pt[1]), surface_point=pt)
                if self.mask(pt[0], pt[1]):
                    out.update(point=pt, t=ok[0], hit=True, cond=abs(B) / D if D != 0 else mp.inf)
                    return out
            out.update(point=along(t_plane), t=t_plane)
            return out
        if kind == "tilted":
            td = sum(s[c] * self.normal[c] for c in range(3))
            t = sum((self.pos[c] - p[c]) * self.normal[c] for c in range(3)) / td
            pt = along(t)
            if self.mask(pt[0], pt[1]):
                out.update(point=pt, t=t, hit=True, radius=self.radius(pt[0], pt[1]))
                if pt[2] < p[2] - f(C_EPS):   # behind the start: Surface._find_hit_handle_abnormal sends it to z = z_max
                    out.update(point=along(t_plane), t=t_plane, hit=False)
                return out
        # numeric: the first sign change of z(t) - values(x(t), y(t)) inside the reference's bracket
        out["numeric"] = True
        t1, t2 = (self.z_min - f(C_EPS) / 10 - p[2]) / s[2], (self.z_max + f(C_EPS) / 10 - p[2]) / s[2]
        if t1 < 0:
            t1 = -f(C_EPS)
        fun = lambda t: p[2] + s[2] * t - self.values(p[0] + s[0] * t, p[1] + s[1] * t)
        p64, s64 = np.array([float(v) for v in p]), np.array([float(v) for v in s])
        ts = np.linspace(float(t1), float(t2), 1025)
        f64 = p64[2] + s64[2] * ts - _composite64(d, self.geom)(p64[0] + s64[0] * ts, p64[1] + s64[1] * ts)
        change = np.nonzero(np.sign(f64[:-1]) * np.sign(f64[1:]) <= 0)[0]
        assert change.size >= 1 and np.ptp(change) <= 1, f"{self.sn}: {change.size} sign changes in the bracket"
        a, b = f(float(ts[change[0]])), f(float(ts[change[-1] + 1]))
        fa, fb = fun(a), fun(b)
        assert fa * fb <= 0
        for _ in range(240):   # bisection to 2^-240 of the cell (the edge of the mask makes f discontinuous)
            m = (a + b) / 2
            fm = fun(m)
            if fa * fm <= 0:
                b, fb = m, fm
            else:
                a, fa = m, fm
        t = (a + b) / 2
        pt = along(t)
        out.update(point=pt, t=t, hit=self.mask(pt[0], pt[1]), radius=self.radius(pt[0], pt[1]))
        return out


def split(x):
    """mpf -> (hi f64, lo f32): hi + lo carries x to 2^-77 relative."""
    hi = float(x)
    return hi, np.float32(float(x - hi))


def join(hi, lo):
    return hi.astype(LD) + lo.astype(LD)


# ---- bars and verdicts -------------------------------------------------------------------------------------------------
def closed_bar(g: dict, k: str, inp: dict) -> np.ndarray:
    """K u (|p|_inf + |o|_2 + |t|) per ray, times |B| / D for `tangent` (g: the archive)."""
    pt = np.abs(g[f"{k}/hi"]).max(axis=1)
    o = inp["p0"] - g[f"{k.split('/')[0]}/geom"][:3]
    bar = K * U * (pt + np.sqrt((o * o).sum(axis=1)) + np.abs(g[f"{k}/t"]))
    if k.endswith("/tangent"):
        bar = bar * g[f"{k}/cond"]
    return bar


def bars(g: dict, k: str, inp: dict) -> np.ndarray:
    """(n, 3): the closed-form bar, and for the rays the numeric search decides 1e-7 |s_j| on top."""
    bar = np.repeat(closed_bar(g, k, inp)[:, None], 3, axis=1)
    return bar + np.where(g[f"{k}/numeric"][:, None], (C_EPS / 10) * np.abs(inp["s0"]), 0.0)


def errors(g: dict, k: str, pts) -> np.ndarray:
    """|pts - truth| (n, 3) in longdouble."""
    return np.abs(np.asarray(pts).astype(LD) - join(g[f"{k}/hi"], g[f"{k}/lo"]))


def undecided(g: dict, k: str, inp: dict) -> np.ndarray:
    """The `rim` rays whose exact distance from the edge of the mask is within four times their bar."""
    if not k.endswith("/rim"):
        return np.zeros(inp["s0"].shape[0], dtype=bool)
    return np.abs(g[f"{k}/delta"]) <= 4 * bars(g, k, inp).max(axis=1)


def self_consistent(sn: str, geom, r_eps2: float, ri_eps2, pts, is_hit) -> bool:
    """is_hit == (dx dx + dy dy <= r_eps2) in float64 on the returned point (that a not-hit ray lies on z = z_max is the
    bar's business: `check` holds its point to the exact ray's point on that plane)."""
    dx, dy = pts[:, 0] - geom[0], pts[:, 1] - geom[1]
    r2 = dx * dx + dy * dy
    m = r2 <= r_eps2
    if ri_eps2 is not None:
        m &= ri_eps2 <= r2
    if SURFACES[sn]["kind"] == "conic":   # a conic's not-hit ray carries the point on z = z_max, not the one the mask saw
        return bool(np.all(m[is_hit]))
    return bool(np.array_equal(m, is_hit))


def check(g: dict, sn: str, fam: str, inp: dict, pts, is_hit, r_eps2=None, ri_eps2=None, sel=None) -> dict:
    """One class of results (the rays `sel`, default all) against the archive -> dict(ratio: worst error / bar, err: worst
    error, wrong: verdicts that differ where they are decided, undecided: count, consistent: the undecided rays' own rule)."""
    k = key(sn, fam)
    sel = np.ones(inp["s0"].shape[0], dtype=bool) if sel is None else np.asarray(sel, dtype=bool)
    und = undecided(g, k, inp) & sel
    err = errors(g, k, pts)
    ratio = err / bars(g, k, inp)
    if fam == "behind":
        ratio = np.where(np.asarray(pts) == inp["p0"], 0.0, np.inf)
    dec = ~und & sel
    out = dict(ratio=float(ratio[dec].max(initial=0.0)), err=float(err[dec].max(initial=0.0)),
               wrong=int(np.count_nonzero(np.asarray(is_hit)[dec] != g[f"{k}/hit"][dec])), undecided=int(und.sum()), consistent=True)
    if np.any(und):
        # either verdict is admissible: the point is the exact hit, or the exact ray's point on z = z_max
        geom = g[f"{sn}/geom"]
        p0, s0 = inp["p0"][und].astype(LD), inp["s0"][und].astype(LD)
        plane = p0 + s0 * ((LD(geom[4]) - p0[:, 2]) / s0[:, 2])[:, None]
        e_plane = np.abs(np.asarray(pts)[und].astype(LD) - plane) / bars(g, k, inp)[und]
        e_hit = ratio[und] if SURFACES[sn]["kind"] in ("circle", "ring") else \
            np.abs(np.asarray(pts)[und].astype(LD) - join(g[f"{k}/hit_hi"][und], g[f"{k}/hit_lo"][und])) / bars(g, k, inp)[und]
        e = np.where(np.asarray(is_hit)[und][:, None], e_hit, e_plane)
        out["ratio"] = max(out["ratio"], float(e.max()))
        if r_eps2 is not None:
            out["consistent"] = self_consistent(sn, geom, r_eps2, ri_eps2, np.asarray(pts)[und], np.asarray(is_hit)[und])
    return out


# ---- the kernel's closed forms restated in float64 NumPy (no fused operations) --------------------------------------------
def stable_form(sn: str, geom, p, s):
    """find_hit of a flat or conic surface as csrc/ot_device.hpp computes it after this pin -> (p_hit, is_hit)."""
    d = SURFACES[sn]
    px, py, pz, z_min, z_max = (float(v) for v in geom[:5])
    r_eps2 = (d["r"] + N_EPS) ** 2
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    sx, sy, sz = s[:, 0], s[:, 1], s[:, 2]
    along = lambda t: np.stack((x + sx * t, y + sy * t, z + sz * t), axis=1)

    def mask(ph):
        dx, dy = ph[:, 0] - px, ph[:, 1] - py
        r2 = dx * dx + dy * dy
        m = r2 <= r_eps2
        return m & ((d["ri"] - N_EPS) ** 2 <= r2) if d["kind"] == "ring" else m
    with np.errstate(all="ignore"):
        if d["kind"] in ("circle", "ring"):
            ph = along((pz - z) / sz)
            hit = mask(ph)
            beh = z > z_max + N_EPS
        else:
            k, rho = d["k"], 1 / d["R"]
            k1, inv_rho, two_inv_rho = k + 1, 1 / rho, 2 / rho
            z_lo, z_hi = z_min - N_EPS, z_max + N_EPS
            ox, oy, oz = x - px, y - py, z - pz
            ozk = oz * k1
            B = sx * ox + sy * oy + sz * (ozk - inv_rho)
            C = oy * oy + ox * ox + oz * (ozk - two_inv_rho)
            A = np.ones_like(B) if k == 0.0 else 1 + k * (sz * sz)
            D = np.sqrt(B * B - C * A)
            if k == 0.0 and abs(inv_rho) <= PLAIN_SPHERE_R:   # the reference's roots: A = 1, the numerator loses <= 2 u |R|
                t1, t2 = -B - D, -B + D
            else:
                q = -(B + np.where(B >= 0, D, -D))
                ta = q / A
                tb = np.where(q == 0, ta, C / q)
                t1, t2 = np.where(B >= 0, ta, tb), np.where(B >= 0, tb, ta)
            z1, z2 = z + sz * t1, z + sz * t2
            c1 = (z_lo <= z1) & (z1 <= z_hi) & (z1 >= z)
            c2 = (z_lo <= z2) & (z2 <= z_hi) & (z2 >= z) & (t2 < t1)
            ph = along(np.where(c1 & ~c2, t1, t2))
            hit = mask(ph)
            nh = ~hit | ~np.isfinite(D) | ((A == 0) & (B == 0)) | (ph[:, 2] < z_lo) | (ph[:, 2] > z_hi)
            ph = np.where(nh[:, None], along((z_max - z) / sz), ph)
            hit = hit & ~nh
            beh = z > z_max
        ph = np.where(beh[:, None], p, ph)
        return ph, hit & ~beh


def zoo_parab_check(g: dict, p, s, pts) -> tuple:
    """The rays of the zoo's paraboloid that a comparison with the reference at ZOO_TOL may leave out -> (idx, worst
    error / closed-form bar of `pts` against their exact hits).  idx: where the exact value shows the reference farther
    from it than ZOO_TOL (1 + |x|) -- chosen by the generator from the reference's numbers, never from a result."""
    idx = g["zoo_parab/idx"]
    o = p[idx] - g["zoo_parab/geom"][:3]
    bar = K * U * (np.abs(g["zoo_parab/hi"]).max(axis=1) + np.sqrt((o * o).sum(axis=1)) + np.abs(g["zoo_parab/t"]))
    err = np.abs(np.asarray(pts)[idx].astype(LD) - join(g["zoo_parab/hi"], g["zoo_parab/lo"]))
    return idx, float((err / bar[:, None]).max())


def from_behind(g: dict, sn: str, fam: str, inp: dict) -> np.ndarray:
    """The rays whose exact hit meets a conic from its back (n . s <= 0: past the equator of the near-hemisphere a ray
    leaves the sphere through the cap).  find_hit reports them as hits like any other; what the refraction step makes of
    them is not the hit step's business, so the trace test leaves their power alone."""
    d = SURFACES[sn]
    k = key(sn, fam)
    if d["kind"] != "conic":
        return np.zeros(inp["s0"].shape[0], dtype=bool)
    geom, rho = g[f"{sn}/geom"], 1 / d["R"]
    dx, dy = g[f"{k}/hi"][:, 0] - geom[0], g[f"{k}/hi"][:, 1] - geom[1]
    with np.errstate(invalid="ignore"):
        q = np.sqrt(1 - d["k"] * rho * rho * (dx * dx + dy * dy))
        nx, ny = -rho * dx / q, -rho * dy / q
        ns = nx * inp["s0"][:, 0] + ny * inp["s0"][:, 1] + np.sqrt(1 - nx * nx - ny * ny) * inp["s0"][:, 2]
    return g[f"{k}/hit"] & ~(ns > 2.0 ** -20)
