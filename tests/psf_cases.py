"""The definition of `Raytracer.huygens_psf` ("Huygens PSF") restated in NumPy longdouble: the truth of
tests/test_gpu_psf.py and tests/test_psf_host.py, and what both share.  No device is needed here.

A record list is six float64 planes, q (3) | tau0 | kappa | a, as `ot_psf_rays` writes them and `ot_psf_sum` reads them; a dead
record is six zeros.  With delta = x - c, ax = |R| and sg = sign(R) the phase of ray i at an image point is, in turns,

    tau = tau0 + sg kappa e,    e = num / den,    num = delta . delta - 2 ax delta . q,    den = |delta - ax q| + ax.

Bound of the phase as float64 arithmetic forms it (`truth` returns its sum), eps = 2^-52, every product, sum, root and quotient within one
eps of its operands' exact result:
  delta      each component (index + 1/2 - n_px / 2) * (size / n_px): two roundings, 2 eps |delta_c|
  dd         delta . delta, three products and two sums of numbers that carry 2 eps each: 8 eps dd
  dq         delta . q, S = sum |delta_c q_c|: three fused steps and the 2 eps of delta: 5 eps S
  num        one fused step on dd and 2 ax dq: b_num = eps (8 dd + 10 ax S + |num|)
  dist       sqrt(num + ax^2 q . q): the argument carries b_num + eps (4 ax^2 q . q + dist^2), the root halves the relative error
             and adds its own: b_dist = (b_num + eps (4 ax^2 q . q + dist^2)) / (2 dist) + eps dist   (dist > 0 for a live record)
  den        b_den = b_dist + eps den
  e          b_e = b_num / den + |e| b_den / den + 2 eps |e|
  tau        one fused step: b_tau = kappa b_e + eps (|tau0| + kappa |e|)
The reduction r = tau - rint(tau) is exact.  Sine and cosine of 2 pi r are good to a few eps, which the second term of the sum's
bound carries: per image point, for Re and Im alike,

    |U_dev - U_true| <= sum_i a_i 2 pi b_tau_i + (n + 40) eps A,        A = sum a_i.

For every input of the tests (|R| <= 100 mm, size <= 1 mm, lambda >= 380 nm) b_tau stays under 1e-9 turns; `truth` asserts it."""
import ctypes as C

import numpy as np

from wavefront_cases import EPS, LD

PI = 4 * np.arctan(LD(1))
B_TAU_MAX = 1e-9  # turns


def image_points(n_px, size, dz):
    """delta of the n_px^2 image points, row by row, and of the point on the axis: (n_px^2 + 1, 3) longdouble."""
    a = (np.arange(n_px, dtype=LD) + LD(0.5) - LD(n_px) / 2) * LD(size) / LD(n_px)
    x, y = np.meshgrid(a, a)  # x along columns
    d = np.stack([x.ravel(), y.ravel(), np.full(n_px * n_px, LD(dz))], axis=1)
    return np.concatenate([d, np.array([[0, 0, dz]], dtype=LD)], axis=0)


def truth(rec, radius, n_px, size, dz, points=None, block=256):
    """rec (6, n) float64 -> (Re U, Im U, bound), each (n_px^2 + 1,) longdouble, the last point on the axis -- or, with `points`,
    those of the list alone --, then A, sum a^2 and the largest phase bound met."""
    q, tau0, kappa, a = (np.asarray(rec[:3], dtype=LD), *(np.asarray(r, dtype=LD) for r in rec[3:6]))
    n = a.shape[0]
    ax, sg = LD(abs(radius)), LD(1 if radius > 0 else -1)
    A = a.sum()
    delta = image_points(n_px, size, dz)
    if points is not None:
        delta = delta[np.asarray(points)]
    re, im, bound = (np.zeros(delta.shape[0], dtype=LD) for _ in range(3))
    qq = (q * q).sum(axis=0)
    live = np.asarray(rec[5]) != 0
    worst = 0.0
    for s in range(0, delta.shape[0], block):
        d = delta[s:s + block]  # (b, 3)
        dd = (d * d).sum(axis=1)[:, None]
        dq = d @ q  # (b, n)
        S = np.abs(d) @ np.abs(q)
        num = dd - 2 * ax * dq
        dist2 = ((d[:, :, None] - ax * q[None]) ** 2).sum(axis=1)
        dist = np.sqrt(dist2)
        den = dist + ax
        e = num / den
        tau = tau0 + sg * kappa * e
        r = tau - np.rint(tau)
        re[s:s + block] = (a * np.cos(2 * PI * r)).sum(axis=1)
        im[s:s + block] = (a * np.sin(2 * PI * r)).sum(axis=1)
        b_num = EPS * (8 * dd + 10 * ax * S + np.abs(num))
        with np.errstate(divide="ignore", invalid="ignore"):
            b_dist = np.where(dist > 0, (b_num + EPS * (4 * ax * ax * qq + dist2)) / (2 * dist), 0) + EPS * dist
        b_den = b_dist + EPS * den
        b_e = b_num / den + np.abs(e) * b_den / den + 2 * EPS * np.abs(e)
        b_tau = kappa * b_e + EPS * (np.abs(tau0) + kappa * np.abs(e))
        if live.any():
            worst = max(worst, float(b_tau[:, live].max()))
        bound[s:s + block] = (a * (2 * PI * b_tau)).sum(axis=1)
    assert worst < B_TAU_MAX, f"phase bound {worst:.3e} turns: the inputs leave the range the bound is stated for"
    return re, im, bound + (n + 40) * EPS * A, A, (a * a).sum(), worst


def synthetic_records(n, seed, radius, na=0.2):
    """n records of a bundle about the axis, every fifth or so dead (six zeros): unit q on the cap of half angle asin(na) on the
    side of the focus the sign of `radius` says, tau0 within +-5 turns, wavelengths over 380 .. 780 nm, index 1 .. 1.8."""
    rng = np.random.default_rng(seed)
    st, phi = na * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    q = np.stack([st * np.cos(phi), st * np.sin(phi), -np.sign(radius) * np.sqrt(1 - st * st)])
    q /= np.sqrt((q * q).sum(axis=0))
    lam = rng.uniform(380e-6, 780e-6, n)
    rec = np.concatenate([q, [rng.uniform(-5, 5, n), rng.uniform(1, 1.8, n) / lam, np.sqrt(rng.uniform(0.5, 1.5, n))]], axis=0)
    dead = rng.uniform(0, 1, n) < 0.2
    dead[0] = False
    rec[:, dead] = 0
    return np.ascontiguousarray(rec)


def perfect_wave(n_rings, na, wavelength, radius):
    """Records of a perfect spherical wave of numerical aperture `na` in air: equal amplitudes on a stratified disc of ring k
    holding 6 k + 3 points (equal areas per point), every path equal.  -> rec (6, n)"""
    pts = []
    for k in range(n_rings):
        m = 6 * k + 3
        rho = (k + 0.5) / n_rings  # (the annulus k / n .. (k + 1) / n has 2 k + 1 parts of the area and 3 (2 k + 1) points)
        ang = (np.arange(m) + 0.5 * (k % 2)) * 2 * np.pi / m
        pts.append(np.stack([rho * np.cos(ang), rho * np.sin(ang)]))
    xy = np.concatenate(pts, axis=1) * na
    n = xy.shape[1]
    q = np.stack([xy[0], xy[1], -np.sign(radius) * np.sqrt(1 - (xy * xy).sum(axis=0))])
    return np.concatenate([q, [np.zeros(n), np.full(n, 1 / (wavelength * 1e-6)), np.ones(n)]], axis=0)


def check_empty(psf, n_px):
    """Without a usable ray: N = power = 0, an all-NaN intensity, every other figure NaN."""
    import optrace_amd as ot
    assert isinstance(psf, ot.HuygensPSF) and psf.N == 0 and psf.power == 0
    assert psf.intensity.shape == (n_px, n_px) and np.all(np.isnan(psf.intensity))
    for val in (psf.wavelength, psf.strehl, psf.noise_floor, psf.peak):
        assert np.isnan(val)


def entry_point_argument_checks(lib):
    """`ot_psf_rays` and `ot_psf_sum` refuse bad arguments with their OT_ERR_* code and their name in `ot_last_error`, before a
    device is looked for and so without a launch: the addresses below are never dereferenced."""
    from optrace_amd import _capi
    st = C.c_void_p()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    INVALID, UNSUPPORTED = -1, -3
    d3 = C.c_double * 3
    nan, inf = float("nan"), float("inf")

    def rays(N=100, nt=4, p=a, w=a, n=a, wl=a):
        r = _capi.Rays()
        r.N, r.nt, r.p, r.w, r.n, r.wl = N, nt, p, w, n, wl
        return r

    def refused(code, name, rc):
        assert rc == code, (name, rc)
        assert name.encode() in lib.ot_last_error(), lib.ot_last_error()

    good = rays()
    rays_ = lambda R, first, count, k, c, radius, opl, mom, rec: lib.ot_psf_rays(R, first, count, k, c, radius, opl, mom, rec, st)
    ok = [C.byref(good), 0, 10, 2, d3(0, 0, 0), 5.0, a, a, a]
    for i in (0, 4, 6, 7, 8):
        refused(INVALID, "ot_psf_rays: null argument", rays_(*[None if j == i else x for j, x in enumerate(ok)]))
    for missing in ("p", "w", "n", "wl"):
        refused(INVALID, "ot_psf_rays: null argument", rays_(C.byref(rays(**{missing: None})), *ok[1:]))
    for first, count in ((-1, 10), (0, -1), (95, 10)):
        refused(INVALID, "ot_psf_rays: ray range", rays_(ok[0], first, count, *ok[3:]))
    for k in (-1, 3, 100):
        refused(INVALID, "ot_psf_rays: section", rays_(*ok[:3], k, *ok[4:]))
    for radius in (0.0, nan, inf):
        refused(INVALID, "ot_psf_rays: focus or radius", rays_(*ok[:5], radius, *ok[6:]))
    refused(INVALID, "ot_psf_rays: focus or radius", rays_(*ok[:4], d3(inf, 0, 0), *ok[5:]))
    assert rays_(ok[0], 0, 0, *ok[3:]) == 0

    sum_ = lambda n, rec, radius, n_px, size, dz, ws, field, centre: lib.ot_psf_sum(n, rec, radius, n_px, size, dz, ws, field, centre, st)
    ok = [a, 5.0, 64, 0.1, 0.0, a, a, a]
    for i in (0, 5, 6, 7):
        refused(INVALID, "ot_psf_sum: null argument", sum_(10, *[None if j == i else x for j, x in enumerate(ok)]))
    refused(INVALID, "ot_psf_sum", sum_(-1, *ok))
    refused(INVALID, "ot_psf_sum: n_px below 1", sum_(10, *ok[:2], 0, *ok[3:]))
    refused(UNSUPPORTED, "ot_psf_sum: n_px above 1024", sum_(10, *ok[:2], 1025, *ok[3:]))
    refused(UNSUPPORTED, "ot_psf_sum: n_px above 1024", sum_(0, *ok[:2], 1025, *ok[3:]))  # (the limits hold whatever n is)
    for size in (0.0, -1.0, inf, nan):
        refused(INVALID, "ot_psf_sum: size", sum_(10, *ok[:3], size, *ok[4:]))
    for dz in (inf, nan):
        refused(INVALID, "ot_psf_sum: dz", sum_(10, *ok[:4], dz, *ok[5:]))
    for radius in (0.0, nan, inf):
        refused(INVALID, "ot_psf_sum: radius", sum_(10, ok[0], radius, *ok[2:]))
    assert sum_(0, *ok[:2], 1024, *ok[3:]) == 0

    # the workspace formula of the binding is the library's
    for n, n_px in ((1, 1), (63, 2), (257, 33), (257, 64), (70001, 8), (1000000, 128), (10 ** 7, 256), (5, 1024), (130000, 31)):
        assert lib.ot_psf_workspace(n, n_px) == _capi.psf_ws(n, n_px) > 0, (n, n_px)
    assert lib.ot_psf_workspace(-1, 8) == 0 and lib.ot_psf_workspace(10, 0) == 0 and lib.ot_psf_workspace(10, 1025) == 0
