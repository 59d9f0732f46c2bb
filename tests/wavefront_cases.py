"""The definition of `Raytracer.wavefront_analysis` ("Wavefront analysis") restated in NumPy longdouble: the truth of
tests/test_gpu_wavefront.py, and what both wavefront test files share.  No device is needed here.

Beside every reduced sum stands the sum of the absolute values of its terms, which the rounding of a sum in any order is
measured against.  A term is taken at the level where the device adds or subtracts stored numbers: 1 - s_x^2 counts as
1 + s_x^2, q - s (s . q) as |q| + |s| sum |s_c q_c|, and a Zernike polynomial as the sum of the absolute values of its monomials,
norm * sum_k |c_k| rho^(n - m - 2 k) * (|x| + |y|)^m.  Differences the device forms from the results of an earlier pass (the
means of the moments record) are formed here from the same numbers, so they are exact inputs on both sides."""
import ctypes as C
import math

import numpy as np

from optrace_amd.wavefront import WavefrontAnalysis, noll_indices

LD = np.longdouble
EPS = np.finfo(np.float64).eps
M_OPS = 40  # operations per term the bounds of the reduced sums allow for


def sum_bound(n_terms, abs_sum):
    """|rounded sum - sum| for n_terms terms of M_OPS operations each, added in any order."""
    return (n_terms + M_OPS) * EPS * np.asarray(abs_sum, dtype=np.float64)


def zernike_abs(j, x, y):
    """Sum of the absolute values of the monomials of Z_j."""
    n, m = noll_indices(j)
    m = abs(m)
    f = math.factorial
    t = x * x + y * y
    radial = sum(f(n - k) / (f(k) * f((n + m) // 2 - k) * f((n - m) // 2 - k)) * t ** ((n - m) // 2 - k) for k in range((n - m) // 2 + 1))
    return math.sqrt((2 if m else 1) * (n + 1)) * radial * (np.abs(x) + np.abs(y)) ** m


def zernike_ld(j, x, y):
    """Z_j in longdouble, by the definition in words (`optrace_amd.wavefront.zernike`, which works in float64)."""
    n, m = noll_indices(j)
    ma = abs(m)
    f = math.factorial
    rho, theta = np.hypot(x, y), np.arctan2(y, x)
    radial = sum(LD((-1) ** k * f(n - k) // (f(k) * f((n + ma) // 2 - k) * f((n - ma) // 2 - k))) * rho ** (n - 2 * k)
                 for k in range((n - ma) // 2 + 1))
    if m == 0:
        return np.sqrt(LD(n + 1)) * radial
    return np.sqrt(LD(2 * (n + 1))) * radial * (np.cos(ma * theta) if m > 0 else np.sin(ma * theta))


def section_rays(p, w, k, first, end):
    """Step 1 for the rays [first, end): (index of the used rays, p[k], s, w, L), longdouble."""
    p, w = np.asarray(p[first:end], dtype=LD), np.asarray(w[first:end, k], dtype=LD)
    d = p[:, k + 1] - p[:, k]
    L = np.sqrt((d * d).sum(axis=1))
    used = np.nonzero((w > 0) & (L > 0))[0]
    return used, p[used, k], d[used] / L[used, None], w[used], L[used]


def focus_sums(p, w, k, first, end, origin):
    """Steps 2 and 3: (sums[17] as `ot_wavefront_focus` lays them out, sums of |terms|[17], rays used)."""
    used, pk, s, wu, _ = section_rays(p, w, k, first, end)
    q = pk - np.asarray(origin, dtype=LD)
    sq = (s * q).sum(axis=1)
    asq = np.abs(s * q).sum(axis=1)
    val, mag = np.zeros(17, dtype=LD), np.zeros(17, dtype=LD)
    val[0] = mag[0] = wu.sum()
    val[1] = mag[1] = used.shape[0]
    val[2:5], mag[2:5] = (wu[:, None] * q).sum(axis=0), (wu[:, None] * np.abs(q)).sum(axis=0)
    val[5:8], mag[5:8] = (wu[:, None] * s).sum(axis=0), (wu[:, None] * np.abs(s)).sum(axis=0)
    for slot, (a, b) in enumerate(((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))):
        val[8 + slot] = (wu * ((a == b) - s[:, a] * s[:, b])).sum()
        mag[8 + slot] = (wu * ((a == b) + np.abs(s[:, a] * s[:, b]))).sum()
    val[14:17] = (wu[:, None] * (q - s * sq[:, None])).sum(axis=0)
    mag[14:17] = (wu[:, None] * (np.abs(q) + np.abs(s) * asq[:, None])).sum(axis=0)
    return val, mag, used.shape[0]


def sphere_from_sums(val, origin):
    """Host part of steps 2 and 3 in longdouble: (focus, signed radius, cond(A))."""
    A = np.array([[val[8], val[9], val[10]], [val[9], val[11], val[12]], [val[10], val[12], val[13]]], dtype=LD)
    # (3 x 3: Cramer's rule keeps longdouble, which np.linalg does not)
    c = np.empty(3, dtype=LD)
    detA = _det3(A)
    for i in range(3):
        B = A.copy()
        B[:, i] = val[14:17]
        c[i] = _det3(B) / detA
    focus = np.asarray(origin, dtype=LD) + c
    d = focus - (np.asarray(origin, dtype=LD) + val[2:5] / val[0])
    R = np.sqrt((d * d).sum())
    return focus, (R if (d * val[5:8]).sum() > 0 else -R), np.linalg.cond(A.astype(np.float64))


def _det3(A):
    return (A[0, 0] * (A[1, 1] * A[2, 2] - A[1, 2] * A[2, 1]) - A[0, 1] * (A[1, 0] * A[2, 2] - A[1, 2] * A[2, 0])
            + A[0, 2] * (A[1, 0] * A[2, 1] - A[1, 1] * A[2, 0]))


def paths(p, n, w, k, first, end, focus, radius):
    """Steps 4 to 6 (first half) per ray of [first, end): dict of dense float arrays with NaN / w = 0 for rays that are not used,
    n_missed, and the per-ray bounds on opl, u, v that the issue states."""
    count = end - first
    used, pk, s, wu, _ = section_rays(p, w, k, first, end)
    pp, nn = np.asarray(p[first:end], dtype=LD)[used], np.asarray(n[first:end], dtype=LD)[used]
    c, R = np.asarray(focus, dtype=LD), LD(radius)
    o = pk - c
    b = (s * o).sum(axis=1)
    oo = (o * o).sum(axis=1)
    D = b * b - (oo - R * R)
    hit = D >= 0
    n_missed = int(np.count_nonzero(~hit))
    with np.errstate(invalid="ignore"):
        t = -b - np.sign(R) * np.sqrt(D)
    seg = np.sqrt(((pp[:, 1:k + 1] - pp[:, :k]) ** 2).sum(axis=2))  # (n, k)
    inner = (nn[:, :k] * seg).sum(axis=1)
    opl = inner + nn[:, k] * t
    h = o + t[:, None] * s
    u, v = h[:, 0] / abs(R), h[:, 1] / abs(R)
    with np.errstate(invalid="ignore", divide="ignore"):
        b_t = 8 * EPS * (b * b + oo + R * R) / (2 * np.sqrt(D)) + 4 * EPS * np.abs(t)
    b_opl = (k + 8) * 4 * EPS * inner + nn[:, k] * b_t
    b_u = (b_t * np.abs(s[:, 0]) + 4 * EPS * (np.abs(o[:, 0]) + np.abs(t * s[:, 0]))) / abs(R) + 2 * EPS * np.abs(u)
    b_v = (b_t * np.abs(s[:, 1]) + 4 * EPS * (np.abs(o[:, 1]) + np.abs(t * s[:, 1]))) / abs(R) + 2 * EPS * np.abs(v)
    out = {}
    for key, arr in (("opl", opl), ("u", u), ("v", v), ("b_opl", b_opl), ("b_u", b_u), ("b_v", b_v), ("D", D), ("o", np.sqrt(oo))):
        full = np.full(count, np.nan, dtype=LD)
        full[used[hit]] = arr[hit]
        out[key] = full
    out["w"] = np.zeros(count, dtype=LD)
    out["w"][used[hit]] = wu[hit]
    out["n_missed"], out["n_max"] = n_missed, float(nn[:, :k + 1].max()) if used.shape[0] else 1.0
    return out


def first_moments(u, v, opl, w, wl=None):
    """(values, sums of |terms|) of slots 0 .. 7 of the moments record; minimum and maximum are exact."""
    sel = w > 0
    u, v, opl, w = (np.asarray(a, dtype=LD)[sel] for a in (u, v, opl, w))
    val, mag = np.zeros(8, dtype=LD), np.zeros(8, dtype=LD)
    val[0] = mag[0] = w.sum()
    val[1] = mag[1] = w.shape[0]
    for slot, a in ((2, opl), (3, u), (4, v)) + (((5, np.asarray(wl, dtype=LD)[sel]),) if wl is not None else ()):
        val[slot], mag[slot] = (w * a).sum(), (w * np.abs(a)).sum()
    val[6], val[7] = (opl.min(), opl.max()) if w.shape[0] else (np.inf, -np.inf)
    return val, mag


def means_of(mom):
    """(mean opl, mean u, mean v) as the device forms them from its record: float64 quotients."""
    mom = np.asarray(mom, dtype=np.float64)
    return mom[2] / mom[0], mom[3] / mom[0], mom[4] / mom[0]


def central_moments(u, v, opl, w, mom):
    """Slots 8 and 9 about the means of the record `mom`: (sum w opd^2, its |terms|, max (du^2 + dv^2))."""
    sel = w > 0
    u, v, opl, w = (np.asarray(a, dtype=LD)[sel] for a in (u, v, opl, w))
    mo, mu, mv = (LD(a) for a in means_of(mom))
    t = w * (opl - mo) ** 2
    return t.sum(), t.sum(), ((u - mu) ** 2 + (v - mv) ** 2).max() if w.shape[0] else LD(0)


def unit_disc(u, v, w, mom, pupil_radius, pr=None):
    """Steps 6 (second half): (selection of the entries that count, x, y, radius) about the record's means.  pr: the largest
    distance as the device reported it, where the record does not hold its square."""
    _, mu, mv = (LD(a) for a in means_of(mom))
    if pr is None:  # (the record's last slot: the root of its largest squared distance, as the device took it)
        pr = LD(mom[10]) if pupil_radius is None else LD(pupil_radius)
    pr = LD(pr)
    sel = np.asarray(w) > 0
    u, v = np.asarray(u, dtype=LD), np.asarray(v, dtype=LD)
    x, y = np.zeros_like(u), np.zeros_like(v)
    if pr > 0:
        x[sel], y[sel] = (u[sel] - mu) / pr, (v[sel] - mv) / pr
    if pupil_radius is not None:
        sel = sel & ~(x * x + y * y > 1)
    return sel, x, y, pr


def normal_equations(u, v, opl, w, mom, pupil_radius, J, pr=None):
    """Step 7: (G, |terms| of G, g, |terms| of g, entries that count)."""
    sel, x, y, _ = unit_disc(u, v, w, mom, pupil_radius, pr)
    x, y, wd = x[sel], y[sel], np.asarray(w, dtype=LD)[sel]
    opd = np.asarray(opl, dtype=LD)[sel] - LD(means_of(mom)[0])
    Z = np.array([zernike_ld(j, x, y) for j in range(1, J + 1)], dtype=LD).reshape(J, -1)
    Za = np.array([zernike_abs(j, x, y) for j in range(1, J + 1)], dtype=LD).reshape(J, -1)
    return ((Z * wd) @ Z.T, (Za * wd) @ Za.T, (Z * wd) @ opd, (Za * wd) @ np.abs(opd), int(sel.sum()))


def pupil_map(u, v, opl, w, mom, pupil_radius, n_grid):
    """Step 8: (weight sums, w opd sums, |w opd| sums), each (n_grid, n_grid) longdouble, row from y, column from x.  The cell
    indices are formed in float64, as the rule is stated."""
    sel, x, y, _ = unit_disc(u, v, w, mom, pupil_radius)
    x, y = x[sel].astype(np.float64), y[sel].astype(np.float64)
    wd = np.asarray(w, dtype=LD)[sel]
    opd = np.asarray(opl, dtype=LD)[sel] - LD(means_of(mom)[0])
    ix = np.clip(np.floor((x + 1) / 2 * n_grid), 0, n_grid - 1).astype(np.int64)
    iy = np.clip(np.floor((y + 1) / 2 * n_grid), 0, n_grid - 1).astype(np.int64)
    out = [np.zeros((n_grid, n_grid), dtype=LD) for _ in range(3)]
    for dst, val in zip(out, (wd, wd * opd, wd * np.abs(opd))):
        np.add.at(dst, (iy, ix), val)
    return out


def check_empty(wa, n_zernike, n_grid):
    """Without a usable ray: N = power = 0, a zero weight map, every other figure NaN."""
    assert isinstance(wa, WavefrontAnalysis) and wa.N == 0 and wa.power == 0
    for val in (wa.wavelength, wa.opl_mean, wa.rms, wa.pv, wa.opd_min, wa.opd_max, wa.pupil_centre, wa.pupil_radius, wa.zernike,
                wa.opd_map, wa.rms_waves, wa.pv_waves, wa.strehl):
        assert np.all(np.isnan(val))
    assert wa.zernike.shape == (n_zernike,) and wa.opd_map.shape == (n_grid, n_grid)
    assert np.array_equal(wa.weight_map, np.zeros((n_grid, n_grid)))


def entry_point_argument_checks(lib):
    """Every `ot_wavefront_*` entry point refuses bad arguments with its OT_ERR_* code and its name in `ot_last_error`, before a
    device is looked for and so without a launch: the addresses below are never dereferenced."""
    from optrace_amd import _capi
    st = C.c_void_p()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    INVALID, UNSUPPORTED = -1, -3
    d3 = C.c_double * 3
    nan, inf = float("nan"), float("inf")

    def rays(N=100, nt=4, p=a, w=a, n=a):
        r = _capi.Rays()
        r.N, r.nt, r.p, r.w, r.n = N, nt, p, w, n
        return r

    def refused(code, name, rc):
        assert rc == code, (name, rc)
        assert name.encode() in lib.ot_last_error(), lib.ot_last_error()

    good = rays()
    focus = lambda R, first, count, k, org, ws, out: lib.ot_wavefront_focus(R, first, count, k, org, ws, out, st)
    ok = [C.byref(good), 0, 10, 2, d3(0, 0, 0), a, a]
    for i in (0, 4, 5, 6):
        refused(INVALID, "ot_wavefront_focus: null argument", focus(*[None if j == i else x for j, x in enumerate(ok)]))
    refused(INVALID, "ot_wavefront_focus: null argument", focus(C.byref(rays(p=None)), *ok[1:]))
    refused(INVALID, "ot_wavefront_focus: null argument", focus(C.byref(rays(w=None)), *ok[1:]))
    for first, count in ((-1, 10), (0, -1), (95, 10)):
        refused(INVALID, "ot_wavefront_focus: ray range", focus(ok[0], first, count, *ok[3:]))
    for k in (-1, 3, 100):
        refused(INVALID, "ot_wavefront_focus: section", focus(*ok[:3], k, *ok[4:]))
    refused(INVALID, "ot_wavefront_focus: origin", focus(*ok[:4], d3(0, nan, 0), *ok[5:]))
    assert focus(ok[0], 0, 0, *ok[3:]) == 0

    paths_ = lambda R, first, count, k, c, radius, *out: lib.ot_wavefront_paths(R, first, count, k, c, radius, *out, st)
    ok = [C.byref(good), 0, 10, 2, d3(0, 0, 0), 5.0, a, a, a, a, a]
    for i in (0, 4, 6, 7, 8, 9, 10):
        refused(INVALID, "ot_wavefront_paths: null argument", paths_(*[None if j == i else x for j, x in enumerate(ok)]))
    refused(INVALID, "ot_wavefront_paths: null argument", paths_(C.byref(rays(n=None)), *ok[1:]))
    for first, count in ((-1, 10), (0, -1), (95, 10)):
        refused(INVALID, "ot_wavefront_paths: ray range", paths_(ok[0], first, count, *ok[3:]))
    for k in (-1, 3):
        refused(INVALID, "ot_wavefront_paths: section", paths_(*ok[:3], k, *ok[4:]))
    for radius in (0.0, nan, inf):
        refused(INVALID, "ot_wavefront_paths: focus or radius", paths_(*ok[:5], radius, *ok[6:]))
    refused(INVALID, "ot_wavefront_paths: focus or radius", paths_(*ok[:4], d3(inf, 0, 0), *ok[5:]))
    assert paths_(ok[0], 0, 0, *ok[3:]) == 0

    moments = lambda n, *rest: lib.ot_wavefront_moments(n, *rest, st)
    ok = [a, a, a, a, None, a, a]  # (wl may be null)
    for i in (0, 1, 2, 3, 5, 6):
        refused(INVALID, "ot_wavefront_moments: null argument", moments(10, *[None if j == i else x for j, x in enumerate(ok)]))
    refused(INVALID, "ot_wavefront_moments", moments(-1, *ok))
    assert moments(0, *ok) == 0

    map_ = lambda n, u, v, opl, w, mom, pr, n_grid, out: lib.ot_wavefront_map(n, u, v, opl, w, mom, pr, n_grid, out, st)
    ok = [a, a, a, a, a, nan, 64, a]
    for i in (0, 1, 2, 3, 4, 7):
        refused(INVALID, "ot_wavefront_map: null argument", map_(10, *[None if j == i else x for j, x in enumerate(ok)]))
    refused(INVALID, "ot_wavefront_map", map_(-1, *ok))
    refused(INVALID, "ot_wavefront_map: n_grid", map_(10, *ok[:6], 0, a))
    refused(UNSUPPORTED, "ot_wavefront_map: n_grid above 1024", map_(10, *ok[:6], 1025, a))
    refused(UNSUPPORTED, "ot_wavefront_map: n_grid above 1024", map_(0, *ok[:6], 1025, a))  # (the limits hold whatever n is)
    for pr in (0.0, -1.0, inf):
        refused(INVALID, "ot_wavefront_map: pupil radius", map_(10, *ok[:5], pr, 64, a))
    assert map_(0, *ok[:6], 1024, a) == 0

    zern = lambda n, u, v, opl, w, mom, pr, J, ws, out: lib.ot_wavefront_zernike(n, u, v, opl, w, mom, pr, J, ws, out, st)
    ok = [a, a, a, a, a, nan, 15, a, a]
    for i in (0, 1, 2, 3, 4, 7, 8):
        refused(INVALID, "ot_wavefront_zernike: null argument", zern(10, *[None if j == i else x for j, x in enumerate(ok)]))
    refused(INVALID, "ot_wavefront_zernike", zern(-1, *ok))
    refused(INVALID, "ot_wavefront_zernike: no polynomials", zern(10, *ok[:6], 0, a, a))
    refused(UNSUPPORTED, "ot_wavefront_zernike: more than 36", zern(10, *ok[:6], 37, a, a))
    for pr in (0.0, -1.0, inf):
        refused(INVALID, "ot_wavefront_zernike: pupil radius", zern(10, *ok[:5], pr, 15, a, a))
    assert zern(0, *ok[:6], 36, a, a) == 0
