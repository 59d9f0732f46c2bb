"""Surfaces, ray classes, the exact spline and error bars for the spline path of the trace kernel (OT_HIT_SPLINE: find_hit,
surf_values, surf_normal and data_gradient of csrc/ot_device.hpp on csrc/ot_spline.hpp with a PatchCache), shared by
tests/test_spline_host.py and tests/test_gpu_spline_step.py.  The parts that tests/hit_cases.py already has (POS, the lens,
N_EPS, C_EPS, K, U, the input helpers, checksum, the mpmath handle) are imported from there; the truth is computed at
test time, so there is no hi + lo archive and nothing for split / join to do.

A *scene* is one spline surface with its centre at POS -- as a leaf surface (`placed`) and as the front of a lens with a flat
back (`raytracer`).  A *class* is (surface, family), 97 rays, every eighth with w0 = 0, built from the bit generator with +,
-, *, / and sqrt alone.  `wide`, `steep`, `near`, `on`, `inside`, `miss` and `rim` are hit_cases' families.  The others aim
at points chosen from the knot array the surface carries (cell i is [t[i], t[i + 1]), 0-based; ulo = K + 1 and uhi = n - K - 2
are the first and last knot of the equidistant part; uniform_cell accepts the cells ulo + K - 1 .. uhi - K):
  knot      x, or y, or both on a knot of the equidistant part, and the neighbouring doubles of the placed coordinate below
            and above it.  The kernel sees x - centre, so with the centre at POS a target is on the knot to the grid of the
            placed coordinate (exactly wherever that grid holds the knot; `Targets.on_knot` counts them); a rotated surface
            sees the knot through its rotation, i.e. to a few units in the last place.  1-D: every other target on an axis
            (hypot exact), the others at a random azimuth
  seam      targets in the cells ulo + K - 2 .. ulo + K + 1 and uhi - K - 1 .. uhi - K + 2 (1-D: the upper ones, r >= 0):
            one table cell and three arithmetic cells on either side of the hand-over
  end       targets in the outermost knot cell; 2-D: also where the disc touches the data square (|x| = r or |y| = r, and up
            to N_EPS / 2 beyond it, where the argument is clamped); 1-D: r = 0 itself and radii below 1e-9.  (The 1-D
            tables are fitted to the mirrored profile -r .. r, so r = 0 is a data point in the middle of the knot array.)
  hop       steep rays (|a|, |b| in 0.75 .. 1.5) whose float64 Illinois iterates visit three or more patches
  stay      near-normal rays (a, b below 2^-8) aimed at the middle of an arithmetic cell: one patch for the whole search
  parallel  s = (0, 0, 1) bitwise at targets of `knot`, `seam` and `end`: x and y of the hit are the start's, and z is the
            surface value there

Truth (`Spline`, numpy.longdouble with a 64-bit mantissa, asserted): the piecewise polynomial of the knots and coefficients of
sf._tab (layout: include/optrace_amd.h), by the de Boor recurrence on the stored knots; S_x, S_y as its analytic derivative
(B' = K (B_{j,K-1} / (t_{j+K} - t_j) - B_{j+1,K-1} / (t_{j+K+1} - t_{j+1})), not the derivative tables); the 1-D spline
with FITPACK's extrapolation of the end polynomial, the 2-D one with its clamp; the mask r^2 <= (r + N_EPS)^2 and the edge
value at r - N_EPS along the direction of (x, y) outside it, composed as surf_values composes them.  The exact hit is the
first sign change of z(t) - values(x(t), y(t)) inside the reference's bracket (hit_cases.Exact.hit), located on 1025
float64 samples and bisected 80 times in longdouble.

Bars (u = 2^-53, K = 32; delta = the largest deviation of a stored knot of the equidistant part from t0 + (i - ulo) h):
  values     V = K u A0 + (|S_x| + |S_y|) delta,                        A0 = sum |c_ij| B_i B_j; for the absolute height
             p_z + sgn (S - offs) that Surface.values returns V + u |z|: the one rounding of the sum that carries the result
  gradient   G = K u A{x,y} + (|S_xx| + |S_xy| + |S_yy|) delta,          Ax = sum |c_ij| |B_i'| B_j; the second derivatives
             bounded by the largest second-derivative coefficient (convex hull); rotated by |cos|, |sin| of the surface
  normal     G_x + G_y + 4 u per component
  hits       hit_cases' numeric bar 1e-7 |s_j| + K u (|p|_inf + |o|_2 + |t|); verdicts exact wherever the exact radius is
             1e-6 from the edge of the mask (every class but `rim` and `end`), there wherever it is four bars away
  parallel   |z - (p_z + S(x, y))| <= V + K u (|p| + |o| + |t|)
Roundings of the cached path per value: dx 1, the rotation 3, (x - t0) inv_h 2, t0 + fl h 2, the local coordinate 2, a basis
polynomial 4 fused steps and its constant 6 (absolute, on values <= 11/24), a row sum 5, the sum of rows 5, the offset and
sign 1, the centre 1: 28, below K.  The gradient has the same count with B' for B and one product with inv_h more.
Those on the argument (the first ten) are errors of x of a few u |x|, the size of delta itself; they are part of the
delta term's |S_x| delta only while delta is a few u |t|, which holds for every table here (linspace grids; the host
accepts up to 1e-9 h).
"""
from __future__ import annotations

import functools
import math

import numpy as np

import hit_cases as hc
from hit_cases import C_EPS, D1, D2, K, N_EPS, POS, U, LD, N_RAYS, WL, DEPTH, checksum, _mp  # noqa: F401

SK = 4   # OT_SPL_K
OFFSET = 4.657165
BISECTIONS = 80


def _shape(X, Y):
    return X ** 2 / 20 + Y ** 2 / 14 + 0.02 * np.sin(2 * X)


def _f2(x, y):
    return x ** 2 / 16 + y ** 2 / 22 + 0.004 * x ** 3 + 0.01 * np.sin(1.5 * y)


def _f2_deriv(x, y):
    return x / 8 + 0.012 * x ** 2, y / 11 + 0.015 * np.cos(1.5 * y)


def _f1(r):
    return r ** 2 / 16 + 0.001 * r ** 4


SURFACES = {
    "d2_50": dict(kind="data2d", r=3.0, n=50),
    "d2_200": dict(kind="data2d", r=3.0, n=200),
    "d2_rot_flip": dict(kind="data2d", r=3.0, n=50, rotate=30.0, flip=True),
    "d1_50": dict(kind="data1d", r=3.0, n=50),
    "f2_rot": dict(kind="func2d", r=3.0, rotate=25.0),
    "f1": dict(kind="func1d", r=3.0),
}
_ALL = ("wide", "steep", "near", "on", "inside", "miss", "rim", "knot", "seam", "end", "stay", "parallel")
PLAN = {
    "d2_50": _ALL + ("hop",),
    "d2_200": _ALL,
    "d2_rot_flip": _ALL + ("hop",),
    "d1_50": _ALL + ("hop",),
    "f2_rot": _ALL,
    "f1": _ALL,
}
CLASSES = [(sn, fam) for sn, fams in PLAN.items() for fam in fams]
VARIANTS = ("plain", "no_pol", "continuous", "two_splines", "hurb")
Z_START = 2.0   # `two_splines`: the plane the starts are moved to, in front of the extra surface


def key(sn: str, fam: str) -> str:
    return f"{sn}/{fam}"


def assert_longdouble():
    assert np.finfo(LD).nmant >= 63, "numpy.longdouble has no 64-bit mantissa here: the truth of these tests needs one"


# ---- surfaces and scenes ---------------------------------------------------------------------------------------------------
def make_surface(ot, sn: str):
    d = SURFACES[sn]
    r = d["r"]
    with ot.global_options.no_warnings():
        if d["kind"] == "data2d":
            Y, X = np.mgrid[-r:r:d["n"] * 1j, -r:r:d["n"] * 1j]
            sf = ot.DataSurface2D(r=r, data=_shape(X, Y) + OFFSET)
        elif d["kind"] == "data1d":
            rr = np.linspace(0, r, d["n"])
            sf = ot.DataSurface1D(r=r, data=10 - np.sqrt(100 - rr ** 2))
        elif d["kind"] == "func2d":
            sf = ot.FunctionSurface2D(r=r, func=_f2, deriv_func=_f2_deriv)
        else:
            sf = ot.FunctionSurface1D(r=r, func=_f1)
        if d.get("rotate"):
            sf.rotate(d["rotate"])
        if d.get("flip"):
            sf.flip()
    return sf


def placed(ot, sn: str):
    sf = make_surface(ot, sn)
    sf.move_to(list(POS))
    return sf


def raytracer(ot, sn: str, variant: str = "plain"):
    """The tested surface as the front of a lens (n = 1.5, flat back) in air, like hit_cases.raytracer.  `two_splines` puts
    another DataSurface2D in front of it, as a filter of transmission 1: the rays pass it with their direction and weight
    bit for bit and reach the tested surface with a patch cache that has served another table; their starts are moved to
    z = Z_START, see `moved`.  (Not a lens: one of another index bends the rays by its own hit's 1e-7, which leaves nothing
    exact to hold the tested surface to, and one of the ambient index runs the same-medium refraction, which follows the
    reference into a polarisation of NaN for a few steep rays at its flat back -- the C oracle shows the same.)  `hurb`: a
    slit aperture with HURB behind the lens: the spline level with every feature."""
    const = lambda n: ot.RefractionIndex("Constant", n=n)
    RT = ot.Raytracer(outline=[-12, 12, -12, 12, -12, 40], n0=const(1.0), no_pol=(variant == "no_pol"),
                      use_hurb=(variant == "hurb"))
    spectrum = ot.LightSpectrum("Gaussian", mu=540.0, sig=40.0) if variant == "continuous" else \
        ot.LightSpectrum("Monochromatic", wl=WL)
    RT.add(ot.RaySource(ot.Point(), divergence="Isotropic", div_angle=5, pos=[0, 0, -10], spectrum=spectrum))
    r = SURFACES[sn]["r"]
    with ot.global_options.no_warnings():
        if variant == "two_splines":
            Y, X = np.mgrid[-9.5:9.5:60j, -9.5:9.5:60j]
            RT.add(ot.Filter(ot.DataSurface2D(r=9.5, data=(X ** 2 + Y ** 2 / 2) / 200 + 0.01 * np.sin(X) + 0.7),
                             spectrum=ot.TransmissionSpectrum("Constant", val=1), pos=[0, 0, Z_START + 0.2]))
        RT.add(ot.Lens(make_surface(ot, sn), ot.CircularSurface(r=r), n=const(1.5), pos=[POS[0], POS[1], POS[2] + D1],
                       d1=D1, d2=D2))
        if variant == "hurb":
            RT.add(ot.Aperture(ot.SlitSurface(dim=[9.0, 9.0], dimi=[1.0, 6.0]), pos=[0, 0, 20]))
    return RT


def moved(inp: dict) -> dict:
    """The rays of a class with their starts on z = Z_START (`two_splines`): the same lines to a rounding."""
    out = dict(inp)
    T = (inp["p0"][:, 2] - Z_START) / inp["s0"][:, 2]
    out["p0"] = np.ascontiguousarray(inp["p0"] - T[:, None] * inp["s0"])
    return out


# ---- the exact spline ------------------------------------------------------------------------------------------------------
def _basis(t, x, i, order: int = 1):
    """The K + 1 B-splines of degree K that do not vanish on cell i (0-based, t[i] <= x < t[i + 1] or its continuation) and
    their first derivatives, by the Cox-de Boor recurrence in the type of t and x -> (h[K + 1], d[K + 1])."""
    T = lambda k: t[i + k]
    h, h3 = [np.ones(x.shape, dtype=x.dtype)], None
    for j in range(1, SK + 1):
        hh, h = h, [np.zeros(x.shape, dtype=x.dtype) for _ in range(j + 1)]
        for q in range(j):
            tli, tlj = T(q + 1), T(q + 1 - j)
            f = hh[q] / (tli - tlj)
            h[q] = h[q] + f * (tli - x)
            h[q + 1] = f * (x - tlj)
        if j == SK - 1:
            h3 = h
    d = []
    for m in range(SK + 1):
        a = h3[m - 1] / (T(m) - T(m - SK)) if m >= 1 else 0
        b = h3[m] / (T(m + 1) - T(m + 1 - SK)) if m <= SK - 1 else 0
        d.append(SK * (a - b))
    return h, d


class Spline:
    """What the truth needs of a placed spline surface, as the surface carries it."""

    def __init__(self, sf):
        assert_longdouble()
        tab, n = np.asarray(sf._tab, dtype=np.float64), int(sf._nknots)
        self.one_d, self.n, self.nc = bool(sf._1D), n, n - SK - 1
        self.tab = tab
        self.t = tab[:n].copy()
        self.c = tab[n:2 * n].copy() if self.one_d else tab[n:n + self.nc ** 2].reshape(self.nc, self.nc).copy()
        self.r, self.pos = float(sf.r), np.array([float(v) for v in sf.pos])
        self.z_min, self.z_max = float(sf.z_min), float(sf.z_max)
        self.sgn, self.offs, self.angle = float(sf._sign), float(sf._offset), float(sf._angle)
        self.rot = (not self.one_d) and self.angle != 0.0
        self.deriv_unrot = (not self.one_d) and getattr(sf, "deriv_func", None) is not None
        self.cna, self.sna = math.cos(-self.angle), math.sin(-self.angle)
        self.cpa, self.spa = math.cos(self.angle), math.sin(self.angle)
        self.r_eps2, self.r_edge = (self.r + N_EPS) ** 2, self.r - N_EPS
        # the equidistant part as compile_surface (csrc/ot_scene_api.hip) describes it
        self.ulo, self.uhi = SK + 1, n - SK - 2
        t = self.t
        self.lo, self.hi = float(t[SK]), float(t[self.nc])
        self.inv_h = float(max(self.nc - SK - 1, 1)) / (self.hi - self.lo)
        self.h = float((t[self.uhi] - t[self.ulo]) / (self.uhi - self.ulo))
        idx = np.arange(self.ulo, self.uhi + 1)
        self.delta = float(np.max(np.abs(t[idx].astype(LD) - (LD(t[self.ulo]) + (idx - self.ulo) * LD(self.h)))))
        dev64 = np.abs(t[idx] - (t[self.ulo] + (idx - self.ulo) * self.h))
        self.uniform = bool(self.uhi - self.ulo >= 2 * SK and self.h > 0 and np.all(dev64 <= 1e-9 * self.h))
        assert self.uniform, "the tables of these classes have an equidistant part"
        self.t0, self.ku_inv_h = float(t[self.ulo]), 1.0 / self.h
        self.cells = (self.ulo + SK - 1, self.uhi - SK)   # first and last cell uniform_cell accepts
        # bound of the second derivatives: the largest coefficient of the twice differentiated spline (convex hull)
        tl = t.astype(LD)
        c = self.c[:self.nc].astype(LD) if self.one_d else self.c.astype(LD)

        def diff(a, axis, k):   # coefficients of the derivative along `axis` of a spline of degree k on knots tl[SK - k:]
            m = a.shape[axis]
            off = SK - k
            den = tl[off + k + 1:off + k + m] - tl[off + 1:off + m]
            sh = [1] * a.ndim
            sh[axis] = m - 1
            return k * np.diff(a, axis=axis) / den.reshape(sh)
        if self.one_d:
            self.h2 = float(np.max(np.abs(diff(diff(c, 0, SK), 0, SK - 1))))
        else:
            cx, cy = diff(c, 0, SK), diff(c, 1, SK)
            self.h2 = float(np.max(np.abs(diff(cx, 0, SK - 1))) + np.max(np.abs(diff(cx, 1, SK))) + np.max(np.abs(diff(cy, 1, SK - 1))))

    # -- the piecewise polynomial
    def cell(self, x):
        return np.clip(np.searchsorted(self.t.astype(x.dtype), x, side="right") - 1, SK, self.n - SK - 2)

    def eval1(self, rho):
        """-> S, S', A0, A1 at the radius rho (extrapolated beyond the knots like FITPACK's ext = 0)."""
        t = self.t.astype(rho.dtype)
        i = self.cell(rho)
        h, d = _basis(t, rho, i)
        S = dS = A0 = A1 = 0
        for a in range(SK + 1):
            c = self.c[i - SK + a].astype(rho.dtype)
            S, dS = S + c * h[a], dS + c * d[a]
            A0, A1 = A0 + np.abs(c) * h[a], A1 + np.abs(c) * np.abs(d[a])
        return S, dS, A0, A1

    def eval2(self, x, y):
        """-> S, S_x, S_y, A0, Ax, Ay at (x, y) of the spline's own frame (clamped to the knot range like fpbisp)."""
        dt = x.dtype
        t = self.t.astype(dt)
        x, y = np.clip(x, dt.type(self.lo), dt.type(self.hi)), np.clip(y, dt.type(self.lo), dt.type(self.hi))
        ix, iy = self.cell(x), self.cell(y)
        hx, dx = _basis(t, x, ix)
        hy, dy = _basis(t, y, iy)
        S = Sx = Sy = A0 = Ax = Ay = 0
        for a in range(SK + 1):
            for b in range(SK + 1):
                c = self.c[ix - SK + a, iy - SK + b].astype(dt)
                ac = np.abs(c)
                S, Sx, Sy = S + c * hx[a] * hy[b], Sx + c * dx[a] * hy[b], Sy + c * hx[a] * dy[b]
                A0, Ax, Ay = A0 + ac * hx[a] * hy[b], Ax + ac * np.abs(dx[a]) * hy[b], Ay + ac * hx[a] * np.abs(dy[b])
        return S, Sx, Sy, A0, Ax, Ay

    # -- the surface
    def own_frame(self, dx, dy):
        """(dx, dy) relative to the centre -> the arguments of the spline (2-D)."""
        T = dx.dtype.type
        if self.rot:
            dx, dy = dx * T(self.cna) - dy * T(self.sna), dx * T(self.sna) + dy * T(self.cna)
        return dx, T(self.sgn) * dy

    def world(self, xs, ys):
        """Arguments of the spline (2-D) -> (dx, dy) relative to the centre (float64, for aiming)."""
        yr = self.sgn * ys
        if self.rot:
            return xs * self.cpa - yr * self.spa, xs * self.spa + yr * self.cpa
        return xs, yr

    def inside(self, x, y):
        T = x.dtype.type
        dx, dy = x - T(self.pos[0]), y - T(self.pos[1])
        return dx * dx + dy * dy <= T(self.r + N_EPS) ** 2

    def point(self, x, y, inside_only: bool = False) -> dict:
        """Everything at absolute (x, y), in their type: z (Surface.values: the spline inside the mask, the edge value along
        the direction of (x, y) outside), V, inside, and for points inside the mask g (n, 2) = (dz/dx, dz/dy), G (n, 2),
        normal (n, 3), nbar (n,)."""
        T = x.dtype.type
        dx, dy = x - T(self.pos[0]), y - T(self.pos[1])
        ins = self.inside(x, y)
        rr = np.sqrt(dx * dx + dy * dy)
        safe = np.where(rr > 0, rr, T(1))
        if not inside_only:
            scale = np.where(ins, T(1), T(self.r_edge) / safe)
            ex, ey = dx * scale, dy * scale
        else:
            ex, ey = dx, dy
        ku = T(K * U)
        if self.one_d:
            rho = np.sqrt(ex * ex + ey * ey) if not inside_only else rr
            rho = np.where(ins, rho, T(self.r_edge)) if not inside_only else rho
            S, dS, A0, A1 = self.eval1(rho)
            V = ku * A0 + np.abs(dS) * T(self.delta)
            nr = T(self.sgn) * dS
            cs, sn = np.where(rr > 0, dx / safe, T(1)), np.where(rr > 0, dy / safe, T(0))
            g = np.stack((nr * cs, nr * sn), axis=1)
            Gr = ku * A1 + T(self.h2) * T(self.delta)
            G = np.stack((Gr * np.abs(cs), Gr * np.abs(sn)), axis=1)
        else:
            xs, ys = self.own_frame(ex, ey)
            S, Sx, Sy, A0, Ax, Ay = self.eval2(xs, ys)
            V = ku * A0 + (np.abs(Sx) + np.abs(Sy)) * T(self.delta)
            if self.deriv_unrot and self.rot:   # the derivatives at the unrotated coordinates (OT_SURF_FLAG_DERIV_UNROTATED)
                _, Sx, Sy, _, Ax, Ay = self.eval2(dx, T(self.sgn) * dy)
            nxn, nyn = Sx * T(self.sgn), Sy
            Gx, Gy = ku * Ax + T(self.h2) * T(self.delta), ku * Ay + T(self.h2) * T(self.delta)
            if self.rot:
                cp, sp = T(self.cpa), T(self.spa)
                g = np.stack((nxn * cp - nyn * sp, nxn * sp + nyn * cp), axis=1)
                G = np.stack((Gx * abs(cp) + Gy * abs(sp), Gx * abs(sp) + Gy * abs(cp)), axis=1)
            else:
                g, G = np.stack((nxn, nyn), axis=1), np.stack((Gx, Gy), axis=1)
        z = T(self.pos[2]) + T(self.sgn) * (S - T(self.offs))
        norm = np.sqrt(1 + g[:, 0] ** 2 + g[:, 1] ** 2)
        normal = np.stack((-g[:, 0] / norm, -g[:, 1] / norm, 1 / norm), axis=1)
        # Vz: the bar of the absolute height p_z + sgn (S - offs), the number Surface.values returns: V and the rounding of the
        # sum that carries it (no float64 lies closer to z than u |z|; near the vertex V itself is below 1e-18)
        return dict(z=z, V=V, Vz=V + T(U) * np.abs(z), inside=ins, g=g, G=G, normal=normal, nbar=G[:, 0] + G[:, 1] + T(4 * U))

    def values(self, x, y):
        return self.point(x, y)["z"]

    # -- the hit
    def hit(self, p, s) -> dict:
        """The exact hits of the rays (p, s) (n, 3) float64 -> dict(point (n, 3) LD, t, hit, radius, delta (radius minus the
        edge of the mask), behind): the first sign change of z(t) - values(x(t), y(t)) inside the reference's bracket."""
        n = p.shape[0]
        pl, sl = p.astype(LD), s.astype(LD)
        behind = pl[:, 2] > LD(self.z_max) + LD(N_EPS)
        t1 = (LD(self.z_min) - LD(C_EPS) / 10 - pl[:, 2]) / sl[:, 2]
        t2 = (LD(self.z_max) + LD(C_EPS) / 10 - pl[:, 2]) / sl[:, 2]
        t1 = np.where(t1 < 0, -LD(C_EPS), t1)
        fun = lambda t, P, S_: P[:, 2] + S_[:, 2] * t - self.values(P[:, 0] + S_[:, 0] * t, P[:, 1] + S_[:, 1] * t)
        w = np.linspace(0.0, 1.0, 1025)
        ts = t1.astype(np.float64)[:, None] + (t2 - t1).astype(np.float64)[:, None] * w[None, :]
        rep = lambda a: np.repeat(a, 1025, axis=0)
        f64 = fun(ts.ravel(), rep(p), rep(s)).reshape(n, 1025)
        sg = np.sign(f64)
        change = sg[:, :-1] * sg[:, 1:] <= 0
        first = np.argmax(change, axis=1)
        last = 1024 - 1 - np.argmax(change[:, ::-1], axis=1)
        ok = behind | (change.any(axis=1) & (last - first <= 1))
        assert np.all(ok), f"{np.count_nonzero(~ok)} rays without exactly one sign change in the bracket"
        rows = np.arange(n)
        a, b = ts[rows, first].astype(LD), ts[rows, np.minimum(last + 1, 1024)].astype(LD)
        a, b = np.maximum(a, t1), np.minimum(b, t2)
        fa = fun(a, pl, sl)
        assert np.all(behind | (fa * fun(b, pl, sl) <= 0))
        for _ in range(BISECTIONS):
            m = (a + b) / 2
            fm = fun(m, pl, sl)
            left = fa * fm <= 0
            b = np.where(left, m, b)
            a, fa = np.where(left, a, m), np.where(left, fa, fm)
        t = np.where(behind, LD(0), (a + b) / 2)
        pt = pl + sl * t[:, None]
        dx, dy = pt[:, 0] - LD(self.pos[0]), pt[:, 1] - LD(self.pos[1])
        radius = np.sqrt(dx * dx + dy * dy)
        return dict(point=pt, t=t, hit=self.inside(pt[:, 0], pt[:, 1]) & ~behind, radius=radius,
                    delta=radius - (LD(self.r) + LD(N_EPS)), behind=behind)


@functools.lru_cache(maxsize=None)
def _spline_of(ot_name: str, sn: str) -> Spline:
    import importlib
    return Spline(placed(importlib.import_module(ot_name), sn))


def spline(ot, sn: str) -> Spline:
    """The Spline of the placed surface `sn` (built once per package and surface; read-only)."""
    return _spline_of(ot.__name__, sn)


# ---- inputs ------------------------------------------------------------------------------------------------------------------
class Targets:
    """Target points of a class relative to the centre (float64) and what the preconditions test wants to know of them."""

    def __init__(self):
        self.on_knot = 0          # `knot`: coordinates that are a stored knot bit for bit, as the kernel sees them
        self.table_side = 0       # `seam`: targets in a cell of the table path
        self.arith_side = 0
        self.patches = None       # `hop`, `stay`: patches visited by the float64 iterates, per ray


def _cell_points(sp: Spline, rng, cells, k):
    """k coordinates inside knot cells drawn from `cells` (0.05 .. 0.95 of the cell) -> (values, cell indices)."""
    c = np.asarray(cells)[rng.integers(0, len(cells), k)]
    return sp.t[c] + rng.uniform(0.05, 0.95, k) * (sp.t[c + 1] - sp.t[c]), c


def _special_targets(sp: Spline, fam: str, rng, n: int, info: Targets):
    """(dx, dy) of the `knot`, `seam` and `end` targets, and for `knot` the step (-1, 0, 1) in units of the placed
    coordinate's last place that `inputs` applies to them."""
    r, t = sp.r, sp.t
    step = np.zeros((n, 2), dtype=np.int64)
    j = np.arange(n)
    lo_seam = [c for c in range(sp.ulo + SK - 2, sp.ulo + SK + 2)]
    hi_seam = [c for c in range(sp.uhi - SK - 1, sp.uhi - SK + 3)]
    if sp.one_d:
        c, sn_ = hc._unit2(rng, n)
        axis = j % 2 == 0
        c = np.where(axis, np.where(j % 4 == 0, 1.0, 0.0), c)
        sn_ = np.where(axis, np.where(j % 4 == 0, 0.0, -1.0), sn_)
        if fam == "knot":
            ks = np.arange(sp.ulo, sp.uhi + 1)
            ks = ks[(t[ks] > 0.02 * r) & (t[ks] < 0.97 * r)]
            rad = t[ks[rng.integers(0, ks.size, n)]]
            step[:, 0] = step[:, 1] = (j // 2) % 3 - 1
        elif fam == "seam":
            rad, cell = _cell_points(sp, rng, [q for q in hi_seam if t[q] > 0], n)
            info.table_side += int(np.count_nonzero(cell > sp.cells[1]))
            info.arith_side += int(np.count_nonzero(cell <= sp.cells[1]))
        else:
            rad, _ = _cell_points(sp, rng, [sp.n - SK - 2], n)
            rad[::3] = rng.uniform(0.0, 1e-9, n)[::3]
            rad[::9] = 0.0
        return rad * c, rad * sn_, step
    both_ok = lambda a, b: a * a + b * b <= (0.985 * r) ** 2
    free = lambda a: rng.uniform(-1, 1, n) * np.sqrt(np.maximum((0.97 * r) ** 2 - a * a, 0.0))
    if fam == "knot":
        ks = np.arange(sp.ulo, sp.uhi + 1)
        ks = ks[np.abs(t[ks]) < 0.66 * r]
        a, b = t[ks[rng.integers(0, ks.size, n)]], t[ks[rng.integers(0, ks.size, n)]]
        mode = j % 3   # 0: x on a knot, 1: y, 2: both
        st = (j // 3) % 3 - 1
        xs = np.where(mode == 1, rng.uniform(-0.66, 0.66, n) * r, a)
        ys = np.where(mode == 0, rng.uniform(-0.66, 0.66, n) * r, b)
        step[:, 0], step[:, 1] = np.where(mode != 1, st, 0), np.where(mode != 0, st, 0)
    elif fam == "seam":
        a, ca = _cell_points(sp, rng, lo_seam + hi_seam, n)
        b, cb = _cell_points(sp, rng, lo_seam + hi_seam, n)
        mode = j % 3
        mode = np.where((mode == 2) & ~both_ok(a, b), 0, mode)
        xs = np.where(mode == 1, free(b), a)
        ys = np.where(mode == 0, free(a), b)
        table = lambda c: (c < sp.cells[0]) | (c > sp.cells[1])
        side = np.where(mode == 0, table(ca), np.where(mode == 1, table(cb), table(ca) | table(cb)))
        info.table_side += int(np.count_nonzero(side))
        info.arith_side += int(np.count_nonzero(~side))
    else:
        a, _ = _cell_points(sp, rng, [SK, sp.n - SK - 2], n)
        touch = j % 3 == 2                       # where the disc touches the data square, and up to N_EPS / 2 beyond
        a = np.where(touch, np.where(j % 2 == 0, r, -r) + np.where(j % 2 == 0, 1.0, -1.0) * (j % 4 // 2) * rng.uniform(0, 0.5 * N_EPS, n), a)
        other = np.where(touch, rng.uniform(-1e-5, 1e-5, n) * (j % 5 != 0), free(a) * 0.9)
        swap = (j // 3) % 2 == 1
        xs, ys = np.where(swap, other, a), np.where(swap, a, other)
    dx, dy = sp.world(xs, ys)
    return dx, dy, step


def inputs(sp: Spline, sn: str, fam: str, info: Targets = None) -> dict:
    """-> dict(p0 (n, 3), s0 (n, 3) f64, pol0 (n, 3) f32, w0, wl (n,) f32, aim (n,): the aimed delta of `rim`, else 0)."""
    info = Targets() if info is None else info
    n, r = N_RAYS, sp.r
    rng = np.random.default_rng([20260, CLASSES.index((sn, fam))])
    depth = np.full(n, DEPTH)
    aim = np.zeros(n)
    step = np.zeros((n, 2), dtype=np.int64)
    x, y = hc._in_disc(rng, n, 0.0, 0.8 * r)
    s = hc._small(rng, n, 0.35)
    rel = lambda a, b: (sp.values(a + sp.pos[0], b + sp.pos[1]) - sp.pos[2]).astype(np.float64)
    if fam == "wide":
        pass
    elif fam == "steep":
        x, y = 0.5 * x, 0.5 * y
        s = hc._normalized(np.column_stack((rng.uniform(-1.5, 1.5, (n, 2)), np.ones(n))))
    elif fam == "near":
        depth[:] = 1e-3
    elif fam == "on":
        depth[:] = 2.0 ** -48
        depth[1::2] = -rng.uniform(0.5, 1.0, n)[1::2] * 2.0 ** -21   # beyond the surface by less than C_EPS: still a hit
    elif fam == "inside":
        s = hc._small(rng, n, 0.1)
        x, y = hc._in_disc(rng, n, 0.3 * r, 0.6 * r)
        depth = rng.uniform(0.2, 0.8, n) * (rel(x, y) - (sp.z_min - sp.pos[2])) / s[:, 2]
    elif fam == "miss":
        x, y = hc._in_disc(rng, n, r + N_EPS + 1e-3, r + N_EPS + 1.0)
    elif fam == "rim":
        c, sn_ = hc._unit2(rng, n)
        e = np.array(hc.RIM_E)[np.arange(n) % len(hc.RIM_E)]
        sign = np.where((np.arange(n) // len(hc.RIM_E)) % 2 == 0, 1.0, -1.0)
        aim = sign * np.ldexp(r, -e)
        x, y = (r + N_EPS + aim) * c, (r + N_EPS + aim) * sn_
    elif fam in ("knot", "seam", "end"):
        x, y, step = _special_targets(sp, fam, rng, n, info)
    elif fam == "parallel":
        parts = [_special_targets(sp, f, np.random.default_rng([20262, CLASSES.index((sn, fam)), q]), n, info)
                 for q, f in enumerate(("knot", "seam", "end"))]
        pick = np.arange(n) % 3
        x, y = (np.choose(pick, [pt[c] for pt in parts]) for c in range(2))
        step = np.where((pick == 0)[:, None], parts[0][2], 0)
        s = np.tile([0.0, 0.0, 1.0], (n, 1))
    elif fam in ("hop", "stay"):
        m = 8 * n   # candidates; the first n whose float64 iterates meet the class's condition are the class
        if fam == "hop":
            cx, cy = hc._in_disc(rng, m, 0.0, 0.4 * r)
            ab = rng.uniform(0.75, 1.5, (m, 2)) * np.where(rng.random((m, 2)) < 0.5, -1.0, 1.0)
            cs = hc._normalized(np.column_stack((ab, np.ones(m))))
        else:
            mid = lambda k: _cell_points(sp, rng, list(range(sp.cells[0], sp.cells[1] + 1)), k)[0]
            if sp.one_d:
                rad = mid(m)
                rad = rad[(rad > 0.05 * r) & (rad < 0.9 * r)]
                c, sn_ = hc._unit2(rng, rad.size)
                cx, cy = rad * c, rad * sn_
            else:
                a, b = mid(m), mid(m)
                keep = a * a + b * b < (0.9 * r) ** 2
                a, b = a[keep], b[keep]
                # the middle half of the cell in both coordinates
                ia, ib = sp.cell(a), sp.cell(b)
                a = sp.t[ia] + (0.25 + 0.5 * (a - sp.t[ia]) / (sp.t[ia + 1] - sp.t[ia])) * (sp.t[ia + 1] - sp.t[ia])
                b = sp.t[ib] + (0.25 + 0.5 * (b - sp.t[ib]) / (sp.t[ib + 1] - sp.t[ib])) * (sp.t[ib + 1] - sp.t[ib])
                cx, cy = sp.world(a, b)
            cs = hc._small(rng, cx.size, 2.0 ** -8)
        cz = rel(cx, cy)
        cp = np.column_stack((cx, cy, cz)) + sp.pos - DEPTH * cs
        visited = np.array([len(set(fast_form(sp, cp[q:q + 1], cs[q:q + 1])["patches"][0])) for q in range(cp.shape[0])])
        good = np.nonzero(visited >= 3 if fam == "hop" else visited == 1)[0][:n]
        assert good.size == n, f"{sn}/{fam}: only {good.size} of {cp.shape[0]} candidates meet the class's condition"
        x, y, s = cx[good], cy[good], cs[good]
        info.patches = visited[good]
    else:
        raise ValueError(fam)
    X, Y = x + sp.pos[0], y + sp.pos[1]
    for c, A in enumerate((X, Y)):   # `knot`: the neighbouring doubles of the placed coordinate
        A[step[:, c] < 0] = np.nextafter(A[step[:, c] < 0], -np.inf)
        A[step[:, c] > 0] = np.nextafter(A[step[:, c] > 0], np.inf)
    if fam in ("knot", "parallel"):
        dx, dy = X - sp.pos[0], Y - sp.pos[1]
        seen = (np.hypot(dx, dy), None) if sp.one_d else sp.own_frame(dx, dy)
        info.on_knot += sum(int(np.count_nonzero(np.isin(a, sp.t[sp.ulo:sp.uhi + 1]))) for a in seen if a is not None)
    z = sp.values(X, Y)
    target = np.column_stack((X, Y, z))
    p0 = target - depth[:, None] * s
    if fam == "parallel":
        p0[:, 0], p0[:, 1] = X, Y
    rng = np.random.default_rng([20261, CLASSES.index((sn, fam))])
    e1 = hc._normalized(np.cross(s, np.array([1.0, 0.0, 0.0])[None, :]))
    e2 = np.cross(s, e1)
    c, sn_ = hc._unit2(rng, n)
    pol0 = (c[:, None] * e1 + sn_[:, None] * e2).astype(np.float32)
    w0 = rng.uniform(0.25, 1.0, n).astype(np.float32)
    w0[3::8] = 0.0
    assert n % 64 != 0
    return dict(p0=np.ascontiguousarray(p0), s0=np.ascontiguousarray(s), pol0=pol0, w0=w0,
                wl=np.full(n, WL, dtype=np.float32), aim=aim)


@functools.lru_cache(maxsize=None)
def _case(ot_name: str, sn: str, fam: str, two: bool):
    sp = _spline_of(ot_name, sn)
    info = Targets()
    inp = inputs(sp, sn, fam, info)
    if two:
        inp = moved(inp)
    ex = sp.hit(inp["p0"], inp["s0"])
    for a in list(inp.values()) + [v for v in ex.values()]:
        a.setflags(write=False)
    return inp, ex, info


def case(ot, sn: str, fam: str, two_splines: bool = False):
    """-> (inputs, exact hits, Targets) of a class, computed once and shared (read-only)."""
    return _case(ot.__name__, sn, fam, bool(two_splines))


# ---- bars and verdicts -----------------------------------------------------------------------------------------------------
def hit_bars(sp: Spline, inp: dict, ex: dict) -> np.ndarray:
    """(n, 3): hit_cases' numeric bar, 1e-7 |s_j| + K u (|p|_inf + |o|_2 + |t|)."""
    o = inp["p0"] - sp.pos
    closed = K * U * (np.abs(ex["point"]).max(axis=1) + np.sqrt((o * o).sum(axis=1)) + np.abs(ex["t"])).astype(np.float64)
    return closed[:, None] + (C_EPS / 10) * np.abs(inp["s0"])


def undecided(sp: Spline, fam: str, inp: dict, ex: dict) -> np.ndarray:
    """Rays whose verdict either way is admissible: `rim` and `end` rays within four bars of the edge of the mask."""
    if fam not in ("rim", "end", "parallel"):
        return np.zeros(inp["s0"].shape[0], dtype=bool)
    xy_bar = hit_bars(sp, inp, ex)[:, :2].max(axis=1)
    return (np.abs(ex["delta"]) <= 4 * xy_bar) & ~ex["behind"]


def check(sp: Spline, fam: str, inp: dict, ex: dict, pts, is_hit, sel=None) -> dict:
    """One class of results against the exact hits, like hit_cases.check -> dict(ratio, err, wrong, undecided, consistent,
    zratio (`parallel`: worst |z - (p_z-free) S(x, y)| over its bar, else 0))."""
    n = inp["s0"].shape[0]
    pts, is_hit = np.asarray(pts), np.asarray(is_hit)
    sel = np.ones(n, dtype=bool) if sel is None else np.asarray(sel, dtype=bool)
    und = undecided(sp, fam, inp, ex) & sel
    bar = hit_bars(sp, inp, ex)
    err = np.abs(pts.astype(LD) - ex["point"])
    ratio = (err / bar).astype(np.float64)
    dec = ~und & sel
    out = dict(ratio=float(ratio[sel].max(initial=0.0)), err=float(err[sel].max(initial=0.0)),
               wrong=int(np.count_nonzero(is_hit[dec] != ex["hit"][dec])), undecided=int(und.sum()), consistent=True, zratio=0.0)
    if np.any(und):   # either verdict, but the one that the returned point's own radius gives
        dx, dy = pts[und, 0] - sp.pos[0], pts[und, 1] - sp.pos[1]
        out["consistent"] = bool(np.array_equal(dx * dx + dy * dy <= sp.r_eps2, is_hit[und]))
    if fam == "parallel":
        live = sel & ~ex["behind"]
        pt = sp.point(inp["p0"][live, 0].astype(LD), inp["p0"][live, 1].astype(LD))
        o = inp["p0"][live] - sp.pos
        zbar = pt["V"] + K * U * (np.abs(ex["point"][live]).max(axis=1) + np.sqrt((o * o).sum(axis=1)) + np.abs(ex["t"][live]))
        xy_same = np.all(pts[live, :2] == inp["p0"][live, :2])
        out["zratio"] = float(np.max(np.abs(pts[live, 2].astype(LD) - pt["z"]) / zbar)) if xy_same else np.inf
    return out


def passes(res: dict) -> bool:
    return res["ratio"] <= 1 and res["zratio"] <= 1 and res["wrong"] == 0 and res["consistent"]


def report(title, k, res) -> str:
    z = f", z {res['zratio']:.2e} of its bar" if k.endswith("/parallel") else ""
    return (f"{title:22s} {k:22s} {res['err']:.1e} mm = {res['ratio']:9.2e} of the bar, {res['wrong']:2d} wrong verdicts, "
            f"{res['undecided']:2d} undecided{z}" + ("" if passes(res) else "   <-- FAILS"))


def normal_ratio(sp: Spline, x, y, normals) -> float:
    """Worst error of unit normals at the absolute points (x, y) (inside the mask) over the normal bar."""
    pt = sp.point(np.asarray(x).astype(LD), np.asarray(y).astype(LD), inside_only=True)
    return float(np.max(np.abs(np.asarray(normals).astype(LD) - pt["normal"]) / pt["nbar"][:, None], initial=0.0))


# ---- the direction behind the surface ------------------------------------------------------------------------------------
REFRACTION_ROUNDINGS = 16   # refract of csrc/ot_trace.hpp: n . s 5, 1 - N^2 (1 - ns^2) 5, the root 1, s N + n (W - N ns) 5


def refracted(normal, s, n1: float, n2: float):
    """The exact refraction of unit directions s (n, 3) at unit normals (n, 3), longdouble: s' = N s + n (W - N (n . s)),
    W = sqrt(1 - N^2 (1 - (n . s)^2)), N = n1 / n2 (refraction_cases.reference_step's formula)."""
    s, nn = np.asarray(s).astype(LD), np.asarray(normal).astype(LD)
    N = LD(n1) / LD(n2)
    ns = (nn * s).sum(axis=1)
    W = np.sqrt(1 - N * N * (1 - ns * ns))
    return s * N + nn * (W - N * ns)[:, None]


def direction_check(sp: Spline, s0, p1, p2, s_end, n1: float = 1.0, n2: float = 1.5) -> float:
    """Worst error / bar of the direction a ray leaves the surface with at p1 against the exact refraction of s0 at the exact
    normal of the carried spline at p1's own (x, y).  The direction is (p2 - p1) / |p2 - p1|, p2 the next stored point; a ray
    that misses the lens's back is absorbed there with p2 == p1 and keeps its direction to the end: `s_end` is it, in full
    precision.  Bar per component: the refraction step's roundings REFRACTION_ROUNDINGS u, twice the normal bar
    (|ds'/dn| <= 2 for N < 1), and for a direction formed from two stored points 4 u (|p1| + |p2|) / |p2 - p1|."""
    p1l, p2l = np.asarray(p1).astype(LD), np.asarray(p2).astype(LD)
    d = p2l - p1l
    length = np.sqrt((d * d).sum(axis=1))
    stayed = length == 0
    safe = np.where(stayed, LD(1), length)
    got = np.where(stayed[:, None], np.asarray(s_end).astype(LD), d / safe[:, None])
    pt = sp.point(p1l[:, 0], p1l[:, 1], inside_only=True)
    exact = refracted(pt["normal"], s0, n1, n2)
    two_points = np.where(stayed, LD(0), 4 * U * (np.abs(p1l).max(axis=1) + np.abs(p2l).max(axis=1)) / safe)
    bar = REFRACTION_ROUNDINGS * U + 2 * pt["nbar"] + two_points
    return float(np.max(np.abs(got - exact) / bar[:, None], initial=0.0))


# ---- the trace kernel's path restated in float64 (no fused operations) -------------------------------------------------------
def _uniform4(u):
    u2 = u * u
    u4, v = u2 * u2, 1.0 - u
    v2 = v * v
    return [v2 * v2 * (1.0 / 24), (((-4.0 * u + 12.0) * u - 6.0) * u - 12.0) * u * (1.0 / 24) + 11.0 / 24,
            (((6.0 * u - 12.0) * u - 6.0) * u + 12.0) * u * (1.0 / 24) + 11.0 / 24,
            ((((-4.0 * u + 4.0) * u + 6.0) * u + 4.0) * u + 1.0) * (1.0 / 24), u4 * (1.0 / 24)]


def _uniform3(u):
    u2, v = u * u, 1.0 - u
    return [v * v * v * (1.0 / 6), ((3.0 * u - 6.0) * u2 + 4.0) * (1.0 / 6), (((-3.0 * u + 3.0) * u + 3.0) * u + 1.0) * (1.0 / 6),
            u2 * u * (1.0 / 6)]


def _uniform4_deriv(u):
    v, u2 = 1.0 - u, u * u
    return [-(v * v * v) * (1.0 / 6), (((-4.0 * u + 9.0) * u - 3.0) * u - 3.0) * (1.0 / 6), (((2.0 * u - 3.0) * u - 1.0) * u + 1.0) * 0.5,
            (((-4.0 * u + 3.0) * u + 3.0) * u + 1.0) * (1.0 / 6), u2 * u * (1.0 / 6)]


def _fpbspl(t, x, l, k):
    h = [1.0] + [0.0] * k
    for j in range(1, k + 1):
        hh = h[:j]
        h[0] = 0.0
        for i in range(1, j + 1):
            tli, tlj = t[l + i - 1], t[l + i - j - 1]
            if tli == tlj:
                h[i] = 0.0
            else:
                f = hh[i - 1] / (tli - tlj)
                h[i - 1] = h[i - 1] + f * (tli - x)
                h[i] = f * (x - tlj)
    return h


def _interval(t, n, k1, inv_h, x):
    nk1 = n - k1
    g = (x - t[k1 - 1]) * inv_h
    l = k1 + ((int(g) if g < nk1 - k1 else nk1 - k1) if g > 0.0 else 0)
    while x < t[l - 1] and l != k1:
        l -= 1
    while x >= t[l] and l != nk1:
        l += 1
    return l


def _basis_table(t, k, x, l):
    """bspl_basis<K>(t, K + 1, n - K - 2, x, l): the equidistant polynomials on the stored knots, or fpbspl."""
    ulo, uhi = k + 1, len(t) - k - 2
    if l - k >= ulo and l + k - 1 <= uhi:
        tl = t[l - 1]
        return (_uniform4 if k == 4 else _uniform3)((x - tl) / (t[l] - tl))
    return _fpbspl(t, x, l, k)


class _Lane:
    """One lane's PatchCache and the restatement's diagnostics."""

    def __init__(self):
        self.key, self.patch, self.prev = None, None, None
        self.patches = []


class FastForm:
    """find_hit<OT_HIT_SPLINE> and surf_normal<true> of the trace kernel for one ray at a time, in float64.  `mistake` plants
    one: "round" (the cell index from round instead of floor), "stale_grad" (the gradient from the patch the cache held
    before its last refresh), "rotate_unrot" (the derivatives' arguments rotated although deriv_unrot is set)."""

    def __init__(self, sp: Spline, mistake: str = None):
        self.sp, self.mistake = sp, mistake
        self.t = [float(v) for v in sp.t]

    def uniform_cell(self, x):
        sp = self.sp
        if not math.isfinite(x):
            return False, 0, 0.0
        q = (x - sp.t0) * sp.ku_inv_h
        fl = float(round(q)) if self.mistake == "round" else math.floor(q)
        l = sp.ulo + int(fl) + 1
        u = (x - (sp.t0 + fl * sp.h)) * sp.ku_inv_h
        return (l - SK >= sp.ulo) and (l + SK - 1 <= sp.uhi), l, u

    def _load(self, lane, keyv, getter):
        if lane.key != keyv:
            lane.prev = lane.patch
            lane.patch = getter()
            lane.key = keyv
        lane.patches.append(keyv)

    def spl1(self, x, lane):
        sp, t, k1 = self.sp, self.t, SK + 1
        ok, l, u = self.uniform_cell(x)
        if ok:
            h = _uniform4(u)
        else:
            l = _interval(t, sp.n, k1, sp.inv_h, x)
            h = _basis_table(t, SK, x, l)
        self._load(lane, l - k1, lambda: [float(sp.c[l - k1 + j]) for j in range(k1)])
        v = 0.0
        for j in range(k1):
            v = v + lane.patch[j] * h[j]
        return v

    def spl2(self, x, y, lane):
        sp, t, k1 = self.sp, self.t, SK + 1
        ax, ay = min(max(x, sp.lo), sp.hi), min(max(y, sp.lo), sp.hi)
        fx, lx, ux = self.uniform_cell(ax)
        fy, ly, uy = self.uniform_cell(ay)
        if fx and fy:
            hx, hy = _uniform4(ux), _uniform4(uy)
        else:
            lx, ly = _interval(t, sp.n, k1, sp.inv_h, ax), _interval(t, sp.n, k1, sp.inv_h, ay)
            hx, hy = _basis_table(t, SK, ax, lx), _basis_table(t, SK, ay, ly)
        self._load(lane, (lx - k1, ly - k1), lambda: [[float(sp.c[lx - k1 + i, ly - k1 + j]) for j in range(k1)] for i in range(k1)])
        v = 0.0
        for i in range(k1):
            row = 0.0
            for j in range(k1):
                row = row + lane.patch[i][j] * hy[j]
            v = v + row * hx[i]
        return v

    def values_rel(self, x, y, lane):
        sp = self.sp
        if sp.one_d:
            v = self.spl1(math.hypot(x, y), lane)
        else:
            xr, yr = (x * sp.cna - y * sp.sna, x * sp.sna + y * sp.cna) if sp.rot else (x, y)
            v = self.spl2(xr, sp.sgn * yr, lane)
        return sp.sgn * (v - sp.offs)

    def mask(self, x, y):
        dx, dy = x - self.sp.pos[0], y - self.sp.pos[1]
        return dx * dx + dy * dy <= self.sp.r_eps2

    def values(self, x, y, lane):
        sp = self.sp
        if self.mask(x, y):
            return sp.pos[2] + self.values_rel(x - sp.pos[0], y - sp.pos[1], lane)
        if sp.one_d:
            return self.edge_val
        dx, dy = x - sp.pos[0], y - sp.pos[1]
        rr = math.sqrt(dx * dx + dy * dy)
        c, sn_ = (dx / rr, dy / rr) if rr > 0.0 else (1.0, 0.0)
        return sp.pos[2] + self.values_rel(sp.r_edge * c, sp.r_edge * sn_, lane)

    @functools.cached_property
    def edge_val(self):
        return self.sp.pos[2] + self.values_rel(self.sp.r - N_EPS, 0.0, _Lane())

    # the derivative tables (the leaf path and the cached gradient's fallback)
    def table_gradient(self, xr, ys):
        sp, t, n = self.sp, self.t, self.sp.n
        nc = sp.nc
        if sp.one_d:
            dc = sp.tab[2 * n:3 * n]
            ok, l, u = self.uniform_cell(xr)
            if ok:
                h = _uniform3(u)
            else:
                l = _interval(t, n, SK + 1, sp.inv_h, xr)
                # spl1_eval<K - 1>: bspl_basis<3>(t, OT_SPL_K + 1, n - OT_SPL_K - 2, x, l, h)
                if l - 3 >= SK + 1 and l + 3 - 1 <= n - SK - 2:
                    h = _uniform3((xr - t[l - 1]) / (t[l] - t[l - 1]))
                else:
                    h = _fpbspl(t, xr, l, 3)
            v = 0.0
            for j in range(4):
                v = v + float(dc[l - (SK + 1) + j]) * h[j]
            return v, None
        cx = sp.tab[n + nc * nc:n + nc * nc + (nc - 1) * nc].reshape(nc - 1, nc)
        cy = sp.tab[n + nc * nc + (nc - 1) * nc:n + nc * nc + 2 * (nc - 1) * nc].reshape(nc, nc - 1)
        t1 = t[1:-1]

        def ev(tx, kx, ty, ky, c):
            ax = min(max(xr, tx[kx]), tx[len(tx) - kx - 1])
            ay = min(max(ys, ty[ky]), ty[len(ty) - ky - 1])
            lx, ly = _interval(tx, len(tx), kx + 1, sp.inv_h, ax), _interval(ty, len(ty), ky + 1, sp.inv_h, ay)
            hx, hy = _basis_table(tx, kx, ax, lx), _basis_table(ty, ky, ay, ly)
            v = 0.0
            for i in range(kx + 1):
                for j in range(ky + 1):
                    v = v + float(c[lx - kx - 1 + i, ly - ky - 1 + j]) * hx[i] * hy[j]
            return v
        return ev(t1, SK - 1, t, SK, cx), ev(t, SK, t1, SK - 1, cy)

    def gradient(self, x, y, lane):
        """data_gradient -> gx, gy, whether the cached patch served."""
        sp, k1 = self.sp, SK + 1
        patch = lane.prev if (self.mistake == "stale_grad" and lane.prev is not None) else lane.patch
        if sp.one_d:
            r = math.hypot(x, y)
            ok, l, u = self.uniform_cell(r)
            cached = lane.key is not None and ok and lane.key == l - k1
            if cached:
                dh = _uniform4_deriv(u)
                v = 0.0
                for j in range(k1):
                    v = v + patch[j] * dh[j]
                d1 = v * sp.ku_inv_h
            else:
                d1 = self.table_gradient(r, None)[0]
            nr = sp.sgn * d1
            rr = math.sqrt(x * x + y * y)
            return (nr * (x / rr), nr * (y / rr), cached) if rr > 0.0 else (nr, 0.0, cached)
        xr, yr = x, y
        if sp.rot and (not sp.deriv_unrot or self.mistake == "rotate_unrot"):
            xr, yr = x * sp.cna - y * sp.sna, x * sp.sna + y * sp.cna
        ys = sp.sgn * yr
        cx_, cy_ = min(max(xr, sp.lo), sp.hi), min(max(ys, sp.lo), sp.hi)
        fx, lx, ux = self.uniform_cell(cx_)
        fy, ly, uy = self.uniform_cell(cy_)
        cached = lane.key is not None and fx and fy and lane.key == (lx - k1, ly - k1)
        if cached:
            hx, hy, dx, dy = _uniform4(ux), _uniform4(uy), _uniform4_deriv(ux), _uniform4_deriv(uy)
            gx = gy = 0.0
            for i in range(k1):
                rx = ry = 0.0
                for j in range(k1):
                    rx = rx + patch[i][j] * hy[j]
                    ry = ry + patch[i][j] * dy[j]
                gx = gx + rx * dx[i]
                gy = gy + ry * hx[i]
            nxn, nyn = gx * sp.ku_inv_h * sp.sgn, gy * sp.ku_inv_h
        else:
            nxn, nyn = self.table_gradient(xr, ys)
            nxn = nxn * sp.sgn
        if sp.rot:
            return nxn * sp.cpa - nyn * sp.spa, nxn * sp.spa + nyn * sp.cpa, cached
        return nxn, nyn, cached

    def ray(self, p, s):
        """-> point (3,), hit, ill, normal (3,) (nan where there is no hit), patches visited, cached."""
        sp = self.sp
        lane = _Lane()
        px, py, pz = (float(v) for v in p)
        sx, sy, sz = (float(v) for v in s)
        along = lambda t: (px + sx * t, py + sy * t, pz + sz * t)
        t1, t2 = (sp.z_min - C_EPS / 10 - pz) / sz, (sp.z_max + C_EPS / 10 - pz) / sz
        if t1 < 0:
            t1 = -C_EPS
        w = math.isfinite(t1) and math.isfinite(t2) and not ((t2 - t1) < C_EPS)
        p1, p2 = along(t1), along(t2)
        f1, f2 = p1[2] - self.values(p1[0], p1[1], lane), p2[2] - self.values(p2[0], p2[1], lane)
        ill = f1 * f2 > 0
        tf, ff = t1, f1
        it = 1
        while w:
            ts = t1 - f1 / (f2 - f1) * (t2 - t1)
            q = along(ts)
            fts = q[2] - self.values(q[0], q[1], lane)
            prod = fts * f2
            if prod < 0:
                t1, f1 = t2, f2
            elif prod > 0:
                f1 = 0.5 * f1
            elif prod == 0:
                t1, f1 = ts, fts
            if prod < 0 or prod > 0 or prod == 0:
                t2, f2 = ts, fts
            if abs(t2 - t1) < C_EPS / 10:
                tf, ff = ts, fts
                break
            if it == 200:
                break
            it += 1
        ph = along(tf)
        hit = bool(self.mask(ph[0], ph[1]))
        beh = pz > sp.z_max + N_EPS
        if ((ph[2] < pz - C_EPS) or abs(ff) > C_EPS) and not beh:
            ph, hit = along((sp.z_max - pz) / sz), False
        if beh:
            ph, hit = (px, py, pz), False
        normal, cached = (math.nan,) * 3, False
        if hit:
            gx, gy, cached = self.gradient(ph[0] - sp.pos[0], ph[1] - sp.pos[1], lane)
            nrm = math.sqrt(gx * gx + gy * gy + 1.0)
            normal = (-gx / nrm, -gy / nrm, 1.0 / nrm)
        return ph, hit, ill, normal, lane.patches, cached


def fast_form(sp: Spline, p, s, mistake: str = None) -> dict:
    """The trace kernel's hit step and normal for the rays (p, s) in float64 -> dict(point (n, 3), hit, ill, normal (n, 3),
    patches (list of the patch keys each ray's evaluations used, in order), cached (the gradient came from the patch))."""
    ff = FastForm(sp, mistake)
    rows = [ff.ray(p[q], s[q]) for q in range(p.shape[0])]
    return dict(point=np.array([r[0] for r in rows]), hit=np.array([r[1] for r in rows], dtype=bool),
                ill=np.array([r[2] for r in rows], dtype=bool), normal=np.array([r[3] for r in rows]),
                patches=[r[4] for r in rows], cached=np.array([r[5] for r in rows], dtype=bool))
