"""The definition of the chromatic analysis (DESIGN.md "Chromatic analysis"; include/optrace_amd.h, ot_chromatic_*) in NumPy
longdouble, written from that text and using nothing of the package's chromatic code.

Storage as in the header: p (N, nt, 3) f64, p[r, i] where section i of ray r starts; w (N, nt) f32; wl (N,) f32; rays r in
[first, first + count); section k.  A ray is used when w[r, k] > 0 and d = p[r, k + 1] - p[r, k] has a length L > 0.  Positions and
weights of rays that are not used are never read into arithmetic: a NaN there does no harm.

Beside every sum stands the sum of the absolute values of its terms, which `sum_bound` turns into the bound of a sum added in any
order.  A crossing point is a per-ray value that the definition forms in float64; `crossings` forms it so, hands it to the sums
as an exact input and checks it against a longdouble evaluation from the stored positions.  The second-pass slots 5-8 take the
centroid as an exact input -- the device's own, formed from its record, when one is
given: its rounding is an input of that pass and not its error."""
import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps
M, FOCUS_M, MAX_BANDS, NO_BAND = 10, 17, 32, 255
M_OPS = 40  # operations per term the bounds of the reduced sums allow for
SUMS = [0, 2, 3, 4, 5, 6, 7]
COUNTS = [1, 9]


def sum_bound(n_terms, abs_sum):
    """|rounded sum - sum| for n_terms terms of M_OPS operations each, added in any order."""
    return (np.asarray(n_terms, dtype=np.float64) + M_OPS) * EPS * np.asarray(abs_sum, dtype=np.float64)


def used_rays(p, w, first, count, k):
    """-> (used (count,) bool, p0 (count, 3), d (count, 3), L (count,)) in longdouble; the entries of rays not used are 0."""
    wk = w[first:first + count, k]
    alive = wk > 0
    p0, d = np.zeros((count, 3), dtype=LD), np.zeros((count, 3), dtype=LD)
    p0[alive] = p[first:first + count, k][alive].astype(LD)
    d[alive] = p[first:first + count, k + 1][alive].astype(LD) - p0[alive]
    L = np.sqrt((d * d).sum(axis=1))
    used = alive & (L > 0)  # (a NaN length is no length)
    p0[~used], d[~used], L[~used] = 0, 0, 0
    return used, p0, d, L


def band_keys(wl, used, bands):
    """The band of every ray by the rule of `huygens_stack`: "lines": every distinct wavelength of the used rays, ascending; an int
    K: K equal bands over [min, max] of the used rays' wavelengths (one band where they are equal); an array: K + 1 ascending edges.
    Band b holds e[b] <= wl < e[b + 1], the last band its upper edge too; wavelengths compare as float64.
    -> (key (count,) int, NO_BAND for rays not used or in no band; K; edges float64 or None)"""
    wl64 = np.asarray(wl).astype(np.float64)
    key = np.full(wl64.shape[0], NO_BAND, dtype=np.int64)
    if isinstance(bands, str):
        lines = np.unique(wl64[used])
        assert lines.shape[0] <= MAX_BANDS
        key[used] = np.searchsorted(lines, wl64[used])
        return key, max(lines.shape[0], 1), None
    if isinstance(bands, (int, np.integer)):
        if not used.any():
            return key, 1, None
        lo, hi = wl64[used].min(), wl64[used].max()
        if lo == hi:
            edges = np.array([lo, hi])
        else:
            edges = lo + (hi - lo) * (np.arange(bands + 1, dtype=np.float64) / bands)
            edges[-1] = hi
    else:
        edges = np.asarray(bands, dtype=np.float64)
    K = edges.shape[0] - 1
    b = np.searchsorted(edges, wl64, side="right") - 1
    b[wl64 == edges[-1]] = K - 1
    inside = used & (b >= 0) & (b < K)
    key[inside] = b[inside]
    return key, K, edges


def focus_sums(p, w, first, count, k, key, K, origin):
    """-> (val, mag): (K, 17) longdouble, per band sum w | rays | sum w q (3) | sum w s (3) | sum w (I - s s^T): xx xy xz yy yz zz |
    sum w (I - s s^T) q (3), q = p[k] - origin, s = d / L; mag: the sums of the absolute values of the terms."""
    used, p0, d, L = used_rays(p, w, first, count, k)
    val, mag = np.zeros((K, FOCUS_M), dtype=LD), np.zeros((K, FOCUS_M), dtype=LD)
    o = np.asarray(origin, dtype=np.float64).astype(LD)
    for b in range(K):
        m = used & (np.asarray(key) == b)
        wt = w[first:first + count, k][m].astype(LD)
        q, s = p0[m] - o, d[m] / L[m][:, None]
        sq, asq = (s * q).sum(axis=1), np.abs(s * q).sum(axis=1)
        # (value, the absolute values of its elementary terms) per slot, as tests/wavefront_cases.py::focus_sums bounds them
        terms = [(wt, wt), (np.ones_like(wt), np.ones_like(wt))]
        terms += [(wt * q[:, c], wt * np.abs(q[:, c])) for c in range(3)] + [(wt * s[:, c], wt * np.abs(s[:, c])) for c in range(3)]
        terms += [(wt * ((i == j) - s[:, i] * s[:, j]), wt * ((i == j) + np.abs(s[:, i] * s[:, j]))) for i in range(3) for j in range(i, 3)]
        terms += [(wt * (q[:, c] - s[:, c] * sq), wt * (np.abs(q[:, c]) + np.abs(s[:, c]) * asq)) for c in range(3)]
        for slot, (t, a) in enumerate(terms):
            val[b, slot], mag[b, slot] = t.sum(), a.sum()
    return val, mag


def solve3(A, b):
    """Cramer's rule in longdouble."""
    A = np.asarray(A, dtype=LD)
    det = lambda m: (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) - m[0, 1] * (m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0])
                     + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))
    D = det(A)
    x = np.zeros(3, dtype=LD)
    for c in range(3):
        Ac = A.copy()
        Ac[:, c] = b
        x[c] = det(Ac) / D
    return x


def system(f):
    f = np.asarray(f)
    return np.array([[f[8], f[9], f[10]], [f[9], f[11], f[12]], [f[10], f[12], f[13]]], dtype=f.dtype), f[14:17]


def foci(sums, origin):
    """(K, 17) sums -> (K, 3) longdouble foci: the solution of [sum w (I - s s^T)] (c - origin) = sum w (I - s s^T) q; NaN for a
    band without a ray and where the system is singular -- the wavefront analysis's test: rank below 3 at NumPy's tolerance."""
    out = np.full((len(sums), 3), np.nan, dtype=LD)
    for b, f in enumerate(sums):
        A, rhs = system(f)
        A64 = A.astype(np.float64)
        if f[1] > 0 and np.all(np.isfinite(A64)) and np.linalg.matrix_rank(A64) == 3:
            out[b] = np.asarray(origin, dtype=np.float64).astype(LD) + solve3(A, rhs)
    return out


def crossings(p, w, first, count, k, z0):
    """-> (used, in the plane sums (used and d_z != 0), x, y): where a ray crosses z = z0, formed as the definition says in float64
    and in its order -- d = p[k + 1] - p[k], t = (z0 - p_z) / d_z, x = p_x + t d_x, y = p_y + t d_y, five IEEE operations each with
    one result -- and handed on as longdouble: the crossing point is a per-ray value of the definition, an exact input of the sums
    as a stored position is for the footprints.  0 for rays outside the plane sums."""
    used, _, _, _ = used_rays(p, w, first, count, k)
    p0 = np.where(used[:, None], p[first:first + count, k], 0.0).astype(np.float64)
    d = np.where(used[:, None], p[first:first + count, k + 1], 0.0).astype(np.float64) - p0
    inside = used & (d[:, 2] != 0)
    t = np.zeros(count)
    t[inside] = (np.float64(z0) - p0[inside, 2]) / d[inside, 2]
    x, y = p0[:, 0] + t * d[:, 0], p0[:, 1] + t * d[:, 1]
    if np.isfinite(z0):
        # The same points in longdouble from the stored positions, so that the float64 values above do not stand alone: d, z0 - p_z,
        # the quotient, the product and the sum round once each, which puts x within 3 eps (|p_x| + |t d_x|) of the truth; 4 allowed.
        # (The bound of a sum, (n + 40) eps sum w |x|, does not cover this where p_x and t d_x cancel, as they do near a focus.)
        q0 = np.where(used[:, None], p[first:first + count, k], 0.0).astype(LD)
        e = np.where(used[:, None], p[first:first + count, k + 1], 0.0).astype(LD) - q0
        tl = np.zeros(count, dtype=LD)
        tl[inside] = (LD(np.float64(z0)) - q0[inside, 2]) / e[inside, 2]
        for c, got in ((0, x), (1, y)):
            off = np.abs(got.astype(LD) - (q0[:, c] + tl * e[:, c]))
            assert np.all(off <= 4 * EPS * (np.abs(q0[:, c]) + np.abs(tl * e[:, c]))), f"crossing points, coordinate {c}: off by {off.max()}"
    return used, inside, x.astype(LD), y.astype(LD)


def records(p, w, wl, first, count, k, key, K, z0, centroid=None):
    """-> (val, mag): (K, 10) longdouble records and, for the slots that are sums, the sums of the absolute values of their terms.
    centroid (K, 2) f64: what slots 5-8 are taken about, default the f64 quotients of the f64-rounded slots 2, 3 and 0."""
    used, inside, x, y = crossings(p, w, first, count, k, z0)
    key = np.asarray(key)
    val, mag = np.zeros((K, M), dtype=LD), np.zeros((K, M), dtype=LD)
    for b in range(K):
        m = inside & (key == b)
        wt = w[first:first + count, k][m].astype(LD)
        xb, yb, lam = x[m], y[m], np.asarray(wl)[first:first + count][m].astype(LD)
        val[b, 9] = np.count_nonzero(used & ~inside & (key == b))
        val[b, 1] = wt.shape[0]
        if not wt.shape[0]:
            val[b, 5:8] = np.nan
            continue
        val[b, 0] = mag[b, 0] = wt.sum()
        val[b, 2], mag[b, 2] = (wt * xb).sum(), (wt * np.abs(xb)).sum()
        val[b, 3], mag[b, 3] = (wt * yb).sum(), (wt * np.abs(yb)).sum()
        val[b, 4] = mag[b, 4] = (wt * lam).sum()
        if centroid is None:
            W = np.float64(val[b, 0])
            cx, cy = np.float64(val[b, 2]) / W, np.float64(val[b, 3]) / W
        else:
            cx, cy = (np.float64(v) for v in centroid[b])
        dx, dy = xb - LD(cx), yb - LD(cy)
        val[b, 5] = mag[b, 5] = (wt * dx * dx).sum()
        val[b, 6] = mag[b, 6] = (wt * dy * dy).sum()
        val[b, 7], mag[b, 7] = (wt * dx * dy).sum(), (wt * np.abs(dx * dy)).sum()
        val[b, 8] = (dx * dx + dy * dy).max()
    return val, mag


def record_centroid(rec):
    """The centroid the device forms from its record (K, 10) f64: two IEEE quotients per band."""
    rec = np.asarray(rec, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([rec[:, 2] / rec[:, 0], rec[:, 3] / rec[:, 0]], axis=1)


def reference_band(wavelengths, counts, reference):
    """The band with rays whose mean wavelength lies nearest to `reference`; the lower index on a tie; -1 if there is none."""
    best, best_d = -1, None
    for b, (lam, n) in enumerate(zip(wavelengths, counts)):
        if n > 0 and lam == lam and (best_d is None or abs(lam - reference) < best_d):
            best, best_d = b, abs(lam - reference)
    return best


def band_wavelengths(p, w, wl, first, count, k, key, K, bands):
    """-> (mean wavelength per band, used rays per band): what the reference band is chosen by.  A line is its band's mean
    wavelength; other bands have the power-weighted mean over their rays in the plane sums, which is the same on every plane and
    no number where there is no such ray."""
    used, inside, _, _ = crossings(p, w, first, count, k, 0.0)
    wt = w[first:first + count, k].astype(LD)
    lam = np.asarray(wl)[first:first + count].astype(LD)
    key = np.asarray(key)
    n_used = np.array([np.count_nonzero(used & (key == b)) for b in range(K)])
    if isinstance(bands, str):
        lines = np.unique(np.asarray(wl)[first:first + count][used].astype(np.float64))
        return np.concatenate([lines, np.full(K - lines.shape[0], np.nan)]).astype(LD), n_used
    masks = [inside & (key == b) for b in range(K)]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.array([(wt * lam)[m].sum() / wt[m].sum() for m in masks], dtype=LD), n_used


def default_reference(p, w, wl, first, count, k):
    """The power-weighted mean wavelength of all used rays."""
    used, _, _, _ = used_rays(p, w, first, count, k)
    wt = w[first:first + count, k][used].astype(LD)
    with np.errstate(invalid="ignore", divide="ignore"):
        return (wt * np.asarray(wl)[first:first + count][used].astype(LD)).sum() / wt.sum()


def evaluate(p, w, wl, first, count, k, bands, z=None, reference=None, origin=(0.0, 0.0, 0.0)):
    """The whole definition -> dict of the figures of `ot.ChromaticAnalysis`, longdouble throughout."""
    used, _, _, _ = used_rays(p, w, first, count, k)
    key, K, edges = band_keys(np.asarray(wl)[first:first + count], used, bands)
    fsum, _ = focus_sums(p, w, first, count, k, key, K, origin)
    focus = foci(fsum, origin)
    wt = np.where(used, w[first:first + count, k], 0).astype(LD)
    lam = np.asarray(wl)[first:first + count].astype(LD)
    ref = reference_band(*band_wavelengths(p, w, wl, first, count, k, key, K, bands), default_reference(p, w, wl, first, count, k)
                         if reference is None else reference)
    assert ref >= 0, "no band has a ray that crosses a plane"
    z0 = np.float64(focus[ref, 2]) if z is None else np.float64(z)
    val, _ = records(p, w, wl, first, count, k, key, K, z0)
    some = val[:, 1] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        W = np.where(some, val[:, 0], np.nan)
        centroid = val[:, 2:4] / W[:, None]
        out = dict(n_bands=K, band_edges=edges, reference_band=ref, z=z0, focus=focus, key=key,
                   band_N=val[:, 1], band_power=val[:, 0], N=val[:, 1].sum(), power=val[:, 0].sum(), n_parallel=val[:, 9].sum(),
                   wavelengths=val[:, 4] / W, centroid=centroid, rms_x=np.sqrt(val[:, 5] / W), rms_y=np.sqrt(val[:, 6] / W),
                   cov_xy=val[:, 7] / W, rms_radius=np.sqrt((val[:, 5] + val[:, 6]) / W), max_radius=np.sqrt(val[:, 8]) + 0 * W,
                   focal_shift=focus[:, 2] - focus[ref, 2], lateral_shift=centroid - centroid[ref])
    fz = focus[np.isfinite(focus[:, 2].astype(np.float64)), 2]
    out["axial_colour"] = fz.max() - fz.min() if fz.shape[0] else LD(np.nan)
    shift = np.sqrt((out["lateral_shift"] ** 2).sum(axis=1))
    out["lateral_colour"] = np.nanmax(shift) if np.any(np.isfinite(shift.astype(np.float64))) else LD(np.nan)
    # the polychromatic spot, directly over all rays of the plane sums
    _, inside, x, y = crossings(p, w, first, count, k, z0)
    m = inside & (key != NO_BAND)
    Wall = wt[m].sum()
    ca = np.array([(wt[m] * x[m]).sum(), (wt[m] * y[m]).sum()]) / Wall
    out["centroid_all"] = ca
    out["rms_radius_all"] = np.sqrt((wt[m] * ((x[m] - ca[0]) ** 2 + (y[m] - ca[1]) ** 2)).sum() / Wall)
    return out


def check_focus_sums(sums, val, mag, what=""):
    """Device sums (K, 17) against the truth: counts equal, every sum within (n + 40) eps sum |terms|."""
    sums = np.asarray(sums, dtype=np.float64)
    assert np.array_equal(sums[:, 1], val[:, 1].astype(np.float64)), f"{what}: counts {sums[:, 1]} against {val[:, 1]}"
    err = np.abs(sums.astype(LD) - val).astype(np.float64)
    bound = sum_bound(val[:, 1:2].astype(np.float64), mag.astype(np.float64))
    bound[:, 1] = 0
    assert np.all(err <= bound), f"{what}: focus sums off by {(err - bound).max():.3e} beyond the bound"
    with np.errstate(invalid="ignore", divide="ignore"):
        return float(np.nanmax(np.where(bound > 0, err / bound, 0.0), initial=0.0))


def check_record(rec, val, mag, what=""):
    """The bounds of the feature on a device record `rec` (K, 10) against the truth (val, mag) of `records` taken about the
    record's own centroid: counts equal, slot 8 within 4 eps relative, sums within (n + 40) eps sum |terms|; NaN where the truth
    has NaN."""
    rec = np.asarray(rec, dtype=np.float64)
    assert np.array_equal(rec[:, COUNTS], val[:, COUNTS].astype(np.float64)), f"{what}: counts {rec[:, COUNTS]} against {val[:, COUNTS]}"
    err8 = np.abs(rec[:, 8].astype(LD) - val[:, 8])
    assert np.all(err8 <= 4 * EPS * val[:, 8]), f"{what}: slot 8 off by {err8.astype(np.float64)}"
    empty = val[:, 1] == 0
    assert np.all(np.isnan(rec[empty][:, 5:8])) and np.all(rec[empty][:, [0, 1, 2, 3, 4, 8]] == 0), f"{what}: an empty band's record"
    n, worst = val[:, 1].astype(np.float64), 0.0
    for s in SUMS:
        err = np.abs(rec[~empty, s].astype(LD) - val[~empty, s]).astype(np.float64)
        bound = sum_bound(n[~empty], mag[~empty, s].astype(np.float64))
        assert np.all(err <= bound), f"{what}: slot {s}: error {err} above {bound}"
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0), initial=0.0)))
    print(f"{what}: sums use at most {worst:.3g} of their bound; slot 8 off by at most {float(err8.max()):.3g}")
