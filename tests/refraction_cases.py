"""Inputs, restatements and error bars for the refraction step (refract, refraction_polarization,
same_medium_polarization, fresnel_T2, refract_ideal / compute_polarization of csrc/ot_trace.hpp), shared by the fixture
generator tests/golden/generate_golden_refraction.py (run on the reference), tests/test_refraction_host.py and
tests/test_gpu_refraction_step.py.

A *scene* is one tested surface (a plane with a constant normal, or an ideal lens) between two constant media; a *class*
is a family of rays aimed at it:
  wide       angles of 0.05 .. 1.2 rad to the normal, s_z >= 0.25; for n1 > n2 rays beyond the critical angle as well, the
             transmitted ones with W >= 2^-8
  small<e>   sin(alpha) = 2^e [1, 2) at a random azimuth around the normal
  parallel   s0 bitwise equal to the normal of the compiled scene
  critical   flat normal, s0 = (sqrt(1 - c^2), 0, c), c the 129 consecutive doubles centred on sqrt(1 - (n2/n1)^2)
  ideal      an IdealLens: rays through the centre along the axis (direction bitwise unchanged) and rays whose bend
             |s' x s| is spread over 2^-16 .. 2^-3
Every ray starts DEPTH in front of its hit point, has wl = 550 and a float32-rounded pol0 perpendicular to s0 at a random
angle; every eighth ray has w0 = 0.  The inputs are built from the bit generator with +, -, *, / and sqrt alone (no sin, cos,
pow, no BLAS product), so that every machine regenerates the same bits.

The full product of normals, media and classes at 128 rays each would be some 32000 rays, which no archive of 1 MB holds
next to exact values.  Every normal x medium pair carries `wide` and `parallel`; the `small` ladders go where the step can
go wrong in different ways (see SMALL_PLAN), 128 rays per rung.
"""
from __future__ import annotations

import hashlib
from collections import namedtuple

import numpy as np

from focus_cases import write_npz  # noqa: F401  (archives with fixed time stamps)

LD = np.longdouble
U = 2.0 ** -53
WL = 550.0
DEPTH = 0.03          # mm between p0 and the hit point
D1 = D2 = 1.5         # the plate: front vertex at z = -D1, back face at z = +D2
R_PLATE = 3.0
HIT_HALF_WIDTH = 0.25  # hit points: |x|, |y| below this
N_CLASS, N_PARALLEL, N_CRITICAL, N_IDEAL = 128, 37, 129, 131
IDEAL_CENTRE = 19     # rays of the ideal class along the axis through the centre
IDEAL_R = 3.0
INV_SQRT2 = 1 / np.sqrt(2)

NORMALS = {"flat": (0.0, 0.0, 1.0), "tilt_a": (0.3, -0.2, 0.9), "tilt_b": (-0.05, 0.4, 1.0)}
MEDIA = {"1_1.5": (1.0, 1.5), "1_2.5": (1.0, 2.5), "1.7_1": (1.7, 1.0), "up": (1.5, 1.5000001), "down": (1.5000001, 1.5),
         "same": (1.33, 1.33)}
CRITICAL_MEDIA = {"1.5_1": (1.5, 1.0), "1.7_1": (1.7, 1.0), "1.6_1.33": (1.6, 1.33)}
SMALL_E = (-10, -20, -24, -26, -28, -30, -36, -40, -48)
SMALL_E_FLAT = (-100, -300, -500)   # below 2^-511 the reference's own normalize underflows to 0 / 0
# where the ladders of small angles stand: the flat normal (exact cross product) and both tilted ones at an ordinary index
# step, the two nearly matched pairs (where the reference itself fails) on one tilted normal each, and a few rungs for a
# dense medium on either side and for N == 1
SMALL_PLAN = {("flat", "1_1.5"): SMALL_E + SMALL_E_FLAT, ("tilt_a", "1_1.5"): SMALL_E, ("tilt_b", "up"): SMALL_E,
              ("tilt_a", "down"): SMALL_E, ("tilt_b", "1.7_1"): (-26, -40), ("tilt_a", "1_2.5"): (-26, -40),
              ("tilt_b", "same"): (-10, -30, -48)}
IDEAL_D = {"ideal_pos": 40.0, "ideal_neg": -40.0}

Scene = namedtuple("Scene", "name normal n1 n2 classes D")   # D: optical power of the ideal lens, else None


def unit_normal(key: str) -> np.ndarray:
    """The normal a TiltedSurface stores, value / np.linalg.norm(value); the flat one is exact.  (np.linalg.norm is the
    one library product in here, because the surface classes use it: the archive keeps the normal it was made with.)"""
    v = np.asarray(NORMALS[key], dtype=np.float64)
    return v if key == "flat" else v / np.linalg.norm(v)


def scenes() -> list:
    out = []
    for nk in NORMALS:
        for mk, (n1, n2) in MEDIA.items():
            classes = ["wide", "parallel"] + [f"small{e}" for e in SMALL_PLAN.get((nk, mk), ())]
            if nk == "flat" and mk in CRITICAL_MEDIA:
                classes.append("critical")
            out.append(Scene(f"{nk}/{mk}", nk, n1, n2, tuple(classes), None))
    for mk, (n1, n2) in CRITICAL_MEDIA.items():
        if mk not in MEDIA:
            out.append(Scene(f"flat/{mk}", "flat", n1, n2, ("parallel", "critical"), None))
    for name, D in IDEAL_D.items():
        out.append(Scene(name, "flat", 1.0, 1.0, ("ideal",), D))
    return out


def scene(name: str) -> Scene:
    return next(sc for sc in scenes() if sc.name == name)


# ---- inputs ----------------------------------------------------------------------------------------------------------
def _normalized(v):
    return v / np.sqrt(v[:, 0] ** 2 + v[:, 1] ** 2 + v[:, 2] ** 2)[:, None]


def _frame(n):
    """Two unit vectors that complete n to a right-handed orthonormal frame."""
    t1 = np.array([0.0, n[2], -n[1]])   # n x e_x
    t1 = t1 / np.sqrt(t1[1] * t1[1] + t1[2] * t1[2])
    return t1, _cross(n[None, :], t1[None, :])[0]


def _unit2(rng, k):
    """k points on the unit circle (cos, sin of a random azimuth) without a trigonometric function."""
    uv = rng.uniform(-1, 1, (4 * k + 64, 2))
    r2 = uv[:, 0] * uv[:, 0] + uv[:, 1] * uv[:, 1]
    uv, r2 = uv[(r2 <= 1) & (r2 >= 0.01)][:k], r2[(r2 <= 1) & (r2 >= 0.01)][:k]
    assert uv.shape[0] == k
    return uv[:, 0] / np.sqrt(r2), uv[:, 1] / np.sqrt(r2)


def _around(n, alpha_sin, alpha_cos, cs):
    t1, t2 = _frame(n)
    t = cs[0][:, None] * t1 + cs[1][:, None] * t2
    return n * alpha_cos[:, None] + t * alpha_sin[:, None]


def _directions(sc: Scene, cls: str, rng) -> np.ndarray:
    n = unit_normal(sc.normal)
    N = sc.n1 / sc.n2
    if cls == "wide":
        ca = rng.uniform(0.3623577544766736, 0.9987502603949663, 4096)   # cos(1.2) .. cos(0.05)
        s = _normalized(_around(n, np.sqrt(1 - ca * ca), ca, _unit2(rng, 4096)))
        ns = _rdot(s, np.broadcast_to(n, s.shape))
        arg = 1 - N * N * (1 - ns * ns)
        s = s[(s[:, 2] >= 0.25) & (np.abs(arg) >= 2.0 ** -16)]   # W >= 2^-8, and no verdict within rounding of the edge
        assert s.shape[0] >= N_CLASS
        return s[:N_CLASS]
    if cls.startswith("small"):
        a = np.ldexp(1 + rng.random(N_CLASS), int(cls[5:]))
        cs = _unit2(rng, N_CLASS)
        if sc.normal == "flat":   # the tiny components stay as they are (|s| = 1 to rounding without a division)
            return np.stack((a * cs[0], a * cs[1], np.sqrt(1 - a * a)), axis=1)
        return _normalized(_around(n, a, np.sqrt(1 - a * a), cs))
    if cls == "parallel":
        return np.tile(n, (N_PARALLEL, 1))
    if cls == "critical":
        c = np.empty(N_CRITICAL)
        c[N_CRITICAL // 2] = np.sqrt(1 - (sc.n2 / sc.n1) ** 2)
        for k in range(N_CRITICAL // 2):
            c[N_CRITICAL // 2 + k + 1] = np.nextafter(c[N_CRITICAL // 2 + k], 2.0)
            c[N_CRITICAL // 2 - k - 1] = np.nextafter(c[N_CRITICAL // 2 - k], 0.0)
        return np.stack((np.sqrt(1 - c * c), np.zeros_like(c), c), axis=1)
    raise ValueError(cls)


def _pol_for(s, rng) -> np.ndarray:
    """float32-rounded unit vectors perpendicular to s at a random angle."""
    helper = np.where(np.abs(s[:, 2:3]) > 0.9, [[1.0, 0.0, 0.0]], [[0.0, 0.0, 1.0]])
    e1 = _normalized(_cross(s, helper))
    e2 = _cross(s, e1)
    c, sn = _unit2(rng, s.shape[0])
    return (c[:, None] * e1 + sn[:, None] * e2).astype(np.float32)


def inputs(sc: Scene) -> dict:
    """-> dict(p0 (n, 3) f64, s0 (n, 3) f64, pol0 (n, 3) f32, w0 (n,) f32, wl (n,) f32, cls (n,) index into sc.classes)."""
    index = [s.name for s in scenes()].index(sc.name)
    S, H, C = [], [], []
    for ci, cls in enumerate(sc.classes):
        rng = np.random.default_rng([20241, index, ci])
        if cls == "ideal":
            f = 1000 / sc.D
            k = N_IDEAL - IDEAL_CENTRE
            st, cs = rng.uniform(0, 0.48, k), _unit2(rng, k)   # up to 0.5 rad off the axis
            s = np.stack((st * cs[0], st * cs[1], np.sqrt(1 - st * st)), axis=1)
            h, cs = abs(f) * np.ldexp(1 + rng.random(k), rng.integers(-16, -4, k)), _unit2(rng, k)   # the bend is ~ h / |f|
            hit = np.stack((h * cs[0], h * cs[1], np.zeros(k)), axis=1)
            s = np.concatenate((np.tile([0.0, 0.0, 1.0], (IDEAL_CENTRE, 1)), s))
            hit = np.concatenate((np.zeros((IDEAL_CENTRE, 3)), hit))
        else:
            s = _directions(sc, cls, rng)
            n = unit_normal(sc.normal)
            xy = rng.uniform(-HIT_HALF_WIDTH, HIT_HALF_WIDTH, (s.shape[0], 2))
            hit = np.column_stack((xy, -D1 + xy[:, 0] * (-n[0] / n[2]) + xy[:, 1] * (-n[1] / n[2])))
        S.append(s)
        H.append(hit)
        C.append(np.full(s.shape[0], ci))
    s0, hit, cls = np.concatenate(S), np.concatenate(H), np.concatenate(C)
    rng = np.random.default_rng([20242, index])
    pol0 = _pol_for(s0, rng)
    w0 = rng.uniform(0.25, 1.0, s0.shape[0]).astype(np.float32)
    w0[3::8] = 0.0
    assert s0.shape[0] % 64 != 0
    return dict(p0=hit - DEPTH * s0, s0=s0, pol0=pol0, w0=w0, wl=np.full(s0.shape[0], WL, dtype=np.float32), cls=cls)


def checksum(inp: dict) -> str:
    h = hashlib.sha256()
    for k in ("p0", "s0", "pol0", "w0", "wl", "cls"):
        h.update(np.ascontiguousarray(inp[k]).tobytes())
    return h.hexdigest()[:16]


# ---- scenes in either package (ot: optrace_amd, or the reference for the surfaces alone) ------------------------------
def front_surface(ot, sc: Scene):
    if sc.normal == "flat":
        return ot.CircularSurface(r=R_PLATE)
    return ot.TiltedSurface(r=R_PLATE, normal=list(NORMALS[sc.normal]))


VARIANTS = ("plain", "data_medium", "asphere_behind", "data2d_behind", "no_pol")


def raytracer(ot, sc: Scene, variant: str = "plain"):
    """One plate (or ideal lens) in an ambient medium n1, for the product and for the C oracle (CompiledScene).
    The variants select other template instances of the trace kernel without touching sections 0 .. 2."""
    const = lambda n: ot.RefractionIndex("Constant", n=n)
    RT = ot.Raytracer(outline=[-12, 12, -12, 12, -12, 40], n0=const(sc.n1), no_pol=(variant == "no_pol"))
    RT.add(ot.RaySource(ot.Point(), divergence="Isotropic", div_angle=5, pos=[0, 0, -10],
                        spectrum=ot.LightSpectrum("Monochromatic", wl=WL)))
    if sc.D is not None:
        RT.add(ot.IdealLens(r=IDEAL_R, D=sc.D, pos=[0, 0, 0]))
    else:
        n2 = const(sc.n2)
        if variant == "data_medium":   # a table of one value: the interpolation returns it exactly
            n2 = ot.RefractionIndex("Data", wls=np.linspace(380.0, 780.0, 41), vals=np.full(41, sc.n2))
        RT.add(ot.Lens(front_surface(ot, sc), ot.CircularSurface(r=R_PLATE), n=n2, pos=[0, 0, 0], d1=D1, d2=D2))
    if variant == "asphere_behind":
        RT.add(ot.Lens(ot.AsphericSurface(r=4, R=12, k=-0.8, coeff=[2e-3, -4e-5, 3e-7]), ot.CircularSurface(r=4), de=0.5,
                       n=const(1.6), pos=[0, 0, 8]))
    if variant == "data2d_behind":
        Y, X = np.mgrid[-4:4:200j, -4:4:200j]
        RT.add(ot.Lens(ot.DataSurface2D(r=4.0, data=X ** 2 / 20 + Y ** 2 / 14 + 0.02 * np.sin(2 * X)), ot.CircularSurface(r=4.0),
                       de=0.5, n=const(1.6), pos=[0, 0, 8]))
    return RT


# ---- the reference's formula lines, restated in float64 (raytracer.py:720-879, misc.py:94-169) -------------------------
def _rdot(a, b):
    return a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1] + a[:, 2] * b[:, 2]


def _cross(a, b):
    return np.stack((a[:, 1] * b[:, 2] - a[:, 2] * b[:, 1], a[:, 2] * b[:, 0] - a[:, 0] * b[:, 2],
                     a[:, 0] * b[:, 1] - a[:, 1] * b[:, 0]), axis=1)


def _polarization(s, s_, pol, no_pol):
    """-> A_ts, A_tp, pol' (f64; rows of unchanged direction keep pol)."""
    if no_pol:
        h = np.full(s.shape[0], INV_SQRT2)
        return h, h, pol.astype(np.float64)
    with np.errstate(all="ignore"):
        mask = np.any(s != s_, axis=1)
        ps = _normalized(_cross(s_, s))
        pp = _cross(ps, s)
        A_ts, A_tp = _rdot(ps, pol), _rdot(pp, pol)
        A_ts[~mask] = INV_SQRT2
        A_tp[~mask] = INV_SQRT2
        pp_ = _cross(ps, s_)
        new = ps * A_ts[:, None] + pp_ * A_tp[:, None]
    return A_ts, A_tp, np.where(mask[:, None], new, pol.astype(np.float64))


def _fresnel(n1, n2, ns, W, A_ts, A_tp):
    with np.errstate(all="ignore"):
        n1ca, n2cb = n1 * ns, n2 * W
        ts = 2 * n1ca / (n1ca + n2cb)
        tp = 2 * n1ca / (n2 * ns + n1 * W)
        return n2cb / n1ca * ((A_ts * ts) ** 2 + (A_tp * tp) ** 2)


def reference_step(n, s, pol, n1, n2, no_pol=False) -> dict:
    """One refraction in the reference's operation order, float64.  n (3,), s (k, 3), pol (k, 3) f32 ->
    dict(s_, T (0 where tir), pol_ (f64, before the float32 store), tir)."""
    n = np.broadcast_to(n, s.shape)
    n1, n2 = np.full(s.shape[0], n1), np.full(s.shape[0], n2)
    ns = _rdot(n, s)
    N = n1 / n2
    with np.errstate(all="ignore"):
        W = np.sqrt(1 - N ** 2 * (1 - ns ** 2))
        s_ = s * N[:, None] - n * (N * ns - W)[:, None]
    A_ts, A_tp, pol_ = _polarization(s, s_, pol, no_pol)
    T = _fresnel(n1, n2, ns, W, A_ts, A_tp)
    tir = ~np.isfinite(W)
    return dict(s_=s_, T=np.where(tir, 0.0, T), pol_=pol_, tir=tir, W=W)


def reference_ideal(D, pos, p_hit, s0, pol, no_pol=False) -> dict:
    f = 1000 / D
    fsz = f / s0[:, 2]
    s = np.stack((s0[:, 0] * fsz - (p_hit[:, 0] - pos[0]), s0[:, 1] * fsz - (p_hit[:, 1] - pos[1]), np.full(s0.shape[0], f)),
                 axis=1)
    s = _normalized(s) * np.sign(f)
    _, _, pol_ = _polarization(s0, s, pol, no_pol)
    return dict(s_=s, pol_=pol_)


def incidence_plane_form(n, s, pol, n1, n2, guard=None) -> dict:
    """float64 restatement (without fused operations) of the device's refraction_polarization + fresnel_T2: basis from
    m = n x s, squared amplitudes, one reciprocal.  guard=None: the form before the near-normal branch existed (only
    m == 0 is special); guard=g: mm < g takes A_ts^2 = A_tp^2 = (|pol|^2 - (s.pol)^2) / 2 and leaves pol alone."""
    n = np.broadcast_to(n, s.shape)
    pol = pol.astype(np.float64)
    N = n1 / n2
    ns = _rdot(n, s)
    with np.errstate(all="ignore"):
        W = np.sqrt(1 - N * N * (1 - ns * ns))
        q = N * ns - W
        m = _cross(n, s)
        mm, mp, sp, np_ = _rdot(m, m), _rdot(m, pol), _rdot(s, pol), _rdot(n, pol)
        inv = 1 / mm
        tp = ns * sp - np_
        ct = N - q * ns
        A_ts2, A_tp2 = mp * mp * inv, tp * tp * inv
        vec = W[:, None] * s - ct[:, None] * n
        pol_ = (mp[:, None] * m + tp[:, None] * vec) * inv[:, None]
        plain = ~(mm > 0)
        if guard is not None:
            near = (mm > 0) & (mm < guard)
            half = (_rdot(pol, pol) - sp * sp) / 2
            A_ts2, A_tp2 = np.where(near, half, A_ts2), np.where(near, half, A_tp2)
            plain = plain | near
        A_ts2, A_tp2 = np.where(~(mm > 0), 0.5, A_ts2), np.where(~(mm > 0), 0.5, A_tp2)
        pol_ = np.where(plain[:, None], pol, pol_)
        n1ca, n2cb = n1 * ns, n2 * W
        d1, d2 = n1ca + n2cb, n2 * ns + n1 * W
        den = d1 * d2
        T = 4 * n1ca * n2cb * (A_ts2 * (d2 * d2) + A_tp2 * (d1 * d1)) / (den * den)
    return dict(T=T, pol_=pol_)


# ---- exact values (mpmath, where it is installed) ------------------------------------------------------------------------
MP_PREC = 400   # bits; the worst cancellation of the classes (s' x s on a tilted normal at 2^-48) costs 100 of them


def _mp():
    import mpmath
    mpmath.mp.prec = MP_PREC
    return mpmath


def _mp_polarization(mp, s, s_, pol):
    cr = lambda a, b: [a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]]
    dot = lambda a, b: a[0] * b[0] + a[1] * b[1] + a[2] * b[2]
    ps = cr(s_, s)
    l2 = dot(ps, ps)
    if l2 == 0:
        return None
    ln = mp.sqrt(l2)
    ps = [v / ln for v in ps]
    pp, pp_ = cr(ps, s), cr(ps, s_)
    A_ts, A_tp = dot(ps, pol), dot(pp, pol)
    return A_ts, A_tp, [ps[c] * A_ts + pp_[c] * A_tp for c in range(3)]


def exact_step(n, s, pol, n1, n2):
    """The reference's formulas evaluated exactly on the binary values of one ray -> (T, [pol']) as mpf, or None where
    they have no value (total reflection, s' == s exactly)."""
    mp = _mp()
    f = mp.mpf
    n, s, pol, n1, n2 = [f(float(v)) for v in n], [f(float(v)) for v in s], [f(float(v)) for v in pol], f(n1), f(n2)
    ns = n[0] * s[0] + n[1] * s[1] + n[2] * s[2]
    N = n1 / n2
    arg = 1 - N * N * (1 - ns * ns)
    m = [n[1] * s[2] - n[2] * s[1], n[2] * s[0] - n[0] * s[2], n[0] * s[1] - n[1] * s[0]]
    if arg < 0 or n1 == n2 or m == [0, 0, 0]:   # s' x s = -q (n x s) is exactly zero: decided here, not by mpf rounding
        return None
    W = mp.sqrt(arg)
    q = N * ns - W
    s_ = [s[c] * N - n[c] * q for c in range(3)]
    r = _mp_polarization(mp, s, s_, pol)
    if r is None:
        return None
    A_ts, A_tp, pol_ = r
    n1ca, n2cb = n1 * ns, n2 * W
    ts, tp = 2 * n1ca / (n1ca + n2cb), 2 * n1ca / (n2 * ns + n1 * W)
    return n2cb / n1ca * ((A_ts * ts) ** 2 + (A_tp * tp) ** 2), pol_


def exact_ideal(D, pos, p_hit, s0, pol):
    """-> ([pol'], |s' x s|) as mpf, or None for an unchanged direction."""
    mp = _mp()
    f = mp.mpf
    s0, pol, p_hit = [f(float(v)) for v in s0], [f(float(v)) for v in pol], [f(float(v)) for v in p_hit]
    fl = 1000 / f(D)
    fsz = fl / s0[2]
    s = [s0[0] * fsz - (p_hit[0] - f(pos[0])), s0[1] * fsz - (p_hit[1] - f(pos[1])), fl]
    ln = mp.sqrt(s[0] ** 2 + s[1] ** 2 + s[2] ** 2) * mp.sign(fl)
    s = [v / ln for v in s]
    r = _mp_polarization(mp, s0, s, pol)
    return None if r is None else r[2]


def split(x):
    """mpf -> (hi f64, lo f32): hi + lo carries x to 2^-77 relative."""
    hi = float(x)
    return hi, np.float32(float(x - hi))


def join(hi, lo):
    return hi.astype(LD) + lo.astype(LD)


# ---- the bars of the GPU test -----------------------------------------------------------------------------------------
def sin_alpha(n, s) -> np.ndarray:
    """|n x s| in longdouble from the inputs."""
    n = np.broadcast_to(np.asarray(n, dtype=LD), s.shape)
    s = s.astype(LD)
    m = _cross(n, s)
    return np.sqrt(_rdot(m, m))


def bend(s, s_) -> np.ndarray:
    """|s' x s| in longdouble: the `a` of the ideal class."""
    m = _cross(s_.astype(LD), s.astype(LD))
    return np.sqrt(_rdot(m, m))


def w_bar(w0, T_exact, a):
    """|w_dev - w0 T_exact| <= w0 T_exact (2^-24 + 2^-30 + min(2^-24, 2^-49 / a)): the store's float32 rounding, ~30 double
    operations at the worst conditioning of the classes, and 16 times the rounding bound u / a of n x s and the two
    amplitudes -- capped, because below a ~ 2^-25 an exact answer is available without any basis."""
    with np.errstate(divide="ignore"):
        noise = np.minimum(LD(2.0 ** -24), LD(2.0 ** -49) / a)
    return w0.astype(LD) * T_exact * (LD(2.0 ** -24) + LD(2.0 ** -30) + noise)


def pol_bar(a):
    """|pol_dev - pol_exact| per component <= 2^-25 + 2^-30 + min(2^-25, 2^-49 / a)."""
    with np.errstate(divide="ignore"):
        noise = np.minimum(LD(2.0 ** -25), LD(2.0 ** -49) / a)
    return LD(2.0 ** -25) + LD(2.0 ** -30) + noise


def ulp32_distance(a, b) -> np.ndarray:
    """Distance of two float32 arrays of non-negative values in units of the last place."""
    a, b = np.ascontiguousarray(a, dtype=np.float32), np.ascontiguousarray(b, dtype=np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def nopol_T(n, s, n1, n2) -> np.ndarray:
    """The transmission for A_ts^2 = A_tp^2 = 1/2 (no_pol) in longdouble: some 20 operations at 2^-64 on a formula whose
    worst conditioning in the classes compared with it is 2^8 (W >= 2^-8), i.e. good to 2^-50."""
    n = np.broadcast_to(np.asarray(n, dtype=LD), s.shape)
    s, n1, n2 = s.astype(LD), LD(n1), LD(n2)
    ns = _rdot(n, s)
    N = n1 / n2
    with np.errstate(all="ignore"):
        W = np.sqrt(1 - N * N * (1 - ns * ns))
        return _fresnel(n1, n2, ns, W, LD(0.5) ** LD(0.5), LD(0.5) ** LD(0.5))


EXACT_CLASSES = ("wide", "small", "ideal")   # compared with the exact values; parallel and critical: with the oracle's bits


def against_exact(sc: Scene, inp: dict, g: dict, w1, pol1, s_out=None, no_pol=False) -> list:
    """Errors of a result (w1 (n,) f32, pol1 (n, 3) f32 or None) against the exact values of the archive `g`, per class:
    -> rows dict(cls, n, w_rel (largest |w - w0 T| / (w0 T)), w_over (largest error / bar), pol_abs, pol_over, gain (largest
    w / w0 of the rays with T <= 1), finite).  A row passes where w_over <= 1, pol_over <= 1, gain <= 1 and finite.
    (No ray may gain power -- except where the exact T itself exceeds 1: pol0 is a float32 vector whose length is 1 only to
    6e-8, and at nearly matched indices T = |pol_perp|^2 to 1e-15; there the w bar alone holds the weight down.)
    s_out: the direction behind the ideal lens (its `a` is |s' x s|)."""
    k = sc.name
    rows = []
    for ci, cls in enumerate(sc.classes):
        sel = (inp["cls"] == ci) & (inp["w0"] > 0) & np.isfinite(g[f"{k}/pol_hi"][:, 0])
        if not cls.startswith(EXACT_CLASSES) or not np.any(sel):
            continue
        s0, w0 = inp["s0"][sel], inp["w0"][sel]
        a = bend(s0, s_out[sel]) if sc.D is not None else sin_alpha(g[f"{k}/normal"], s0)
        row = dict(cls=cls, n=int(np.count_nonzero(sel)), w_rel=0.0, w_over=0.0, pol_abs=0.0, pol_over=0.0, gain=0.0, finite=True)
        if sc.D is None:
            T = nopol_T(g[f"{k}/normal"], s0, sc.n1, sc.n2) if no_pol else join(g[f"{k}/T_hi"][sel], g[f"{k}/T_lo"][sel])
            err = np.abs(w1[sel].astype(LD) - w0.astype(LD) * T)
            row.update(w_rel=float(np.max(err / (w0.astype(LD) * T))), w_over=float(np.max(err / w_bar(w0, T, a))),
                       gain=float(np.max(np.where(T <= 1, w1[sel] / w0, 0.0))), finite=bool(np.all(np.isfinite(w1[sel]))))
        if pol1 is not None:
            err = np.abs(pol1[sel].astype(LD) - join(g[f"{k}/pol_hi"][sel], g[f"{k}/pol_lo"][sel]))
            row.update(pol_abs=float(err.max()), pol_over=float(np.max(err / pol_bar(a)[:, None])),
                       finite=row["finite"] and bool(np.all(np.isfinite(pol1[sel]))))
        rows.append(row)
    return rows


def row_passes(row: dict) -> bool:
    return row["finite"] and row["w_over"] <= 1 and row["pol_over"] <= 1 and row["gain"] <= 1


def format_rows(title: str, rows: list) -> str:
    return "\n".join(f"{title:28s} {r['cls']:10s} n={r['n']:4d}  w rel {r['w_rel']:.2e} ({r['w_over']:.2f} of bar)  "
                     f"pol abs {r['pol_abs']:.2e} ({r['pol_over']:.2f} of bar)  w/w0 <= {r['gain']:.7f}"
                     + ("" if row_passes(r) else "   <-- FAILS") for r in rows)


def oracle_trace(RT, inp: dict):
    """The rays of `inp` through the C oracle on the compiled scene of RT -> (HostRays, counters)."""
    from optrace_amd.scene import CompiledScene
    import oracle_bridge as ob
    csc = CompiledScene(RT)
    rays = ob.HostRays(inp["s0"].shape[0], csc.nt, RT.no_pol)
    rays.set_initial(inp["p0"], inp["s0"], None if RT.no_pol else inp["pol0"], inp["w0"], inp["wl"])
    msgs, st = ob.trace(csc.desc, rays, None)
    assert st == 0
    return rays, msgs, csc
