"""The definition of the field analysis (DESIGN.md "Field analysis"; include/optrace_amd.h, ot_field_sums) in NumPy longdouble,
written from that text and using nothing of the package's field code.

Storage as in the header: p (N, nt, 3) f64, p[r, i] where section i of ray r starts; w (N, nt) f32; wl (N,) f32; field f owns the
rays [first_f, first_f + count_f); section k.  A ray is used when w[r, k] > 0 and d = p[r, k + 1] - p[r, k] has a length above 0;
its band is its key byte, 255: none.  Positions and weights of rays that are not used are never read into arithmetic.

With q = p[r, k] - origin: m = (d_x, d_y) / d_z and a = (q_x, q_y) - q_z m, formed in float64 in this order (`lines`), are per-ray
values of the definition and enter the sums as exact inputs; `lines` also forms them in longdouble from the stored positions and
holds the float64 values to a few eps of their operands' magnitudes.  Beside every sum stands the sum of the absolute values of its
terms, which `sum_bound` turns into the bound of a sum added in any order.  The second-pass slots 8-17 take the means as exact
inputs -- the device's own, formed from its record, when they are given: their rounding is an input of that pass, not its error."""
import numpy as np

from chromatic_cases import EPS, LD, NO_BAND, band_keys, reference_band, sum_bound, used_rays  # noqa: F401  (shared with the tests)

M, M1, MAX_FIELDS, MAX_BANDS = 18, 8, 64, 32
SUMS = [0, 2, 3, 4, 5, 6] + list(range(8, 18))
COUNTS = [1, 7]
# (i, j) of the products of slots 8 .. 17 in (da_x, da_y, dm_x, dm_y)
PAIRS = [(0, 0), (0, 1), (1, 1), (0, 2), (0, 3), (1, 2), (1, 3), (2, 2), (2, 3), (3, 3)]


def lines(p, w, first, count, k, origin):
    """-> (used, inside (used and d_z != 0), am (count, 4) float64: a_x, a_y, m_x, m_y; 0 outside the sums)."""
    used, _, _, _ = used_rays(p, w, first, count, k)
    o = np.asarray(origin, dtype=np.float64)
    p0 = np.where(used[:, None], p[first:first + count, k], 0.0).astype(np.float64)
    d = np.where(used[:, None], p[first:first + count, k + 1], 0.0).astype(np.float64) - p0
    inside = used & (d[:, 2] != 0)
    q = p0 - o
    am = np.zeros((count, 4))
    with np.errstate(all="ignore"):
        for c in range(2):
            am[inside, 2 + c] = d[inside, c] / d[inside, 2]
            am[inside, c] = q[inside, c] - q[inside, 2] * am[inside, 2 + c]
    # the same in longdouble from the stored positions, so that the float64 values do not stand alone: d rounds once and the
    # quotient once (m within 2 eps |m|); q rounds once, the product and the difference once each on top of m's error (a within
    # 4 eps (|q_x| + |q_z m_x|))
    pl = np.where(used[:, None], p[first:first + count, k], 0.0).astype(LD)
    dl = np.where(used[:, None], p[first:first + count, k + 1], 0.0).astype(LD) - pl
    ql = pl - o.astype(LD)
    fin = inside & np.all(np.isfinite(am), axis=1)
    for c in range(2):
        ml = np.zeros(count, dtype=LD)
        ml[fin] = dl[fin, c] / dl[fin, 2]
        al = ql[:, c] - ql[:, 2] * ml
        off_m = np.abs(am[:, 2 + c].astype(LD) - ml)[fin]
        off_a = np.abs(am[:, c].astype(LD) - al)[fin]
        assert np.all(off_m <= 2 * EPS * np.abs(ml[fin])), f"slopes, coordinate {c}: off by {off_m.max()}"
        assert np.all(off_a <= 4 * EPS * (np.abs(ql[fin, c]) + np.abs(ql[fin, 2] * ml[fin]))), f"intercepts, coordinate {c}"
    return used, inside, am


def record_means(rec):
    """The means the device forms from its records (..., 18) f64: four IEEE quotients per cell."""
    rec = np.asarray(rec, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return rec[..., 2:6] / rec[..., 0:1]


def records(p, w, wl, fields, k, key, key_first, K, origin, means=None):
    """fields: [(first, count), ...]; key[r - key_first]: the band of ray r.  -> (val, mag): (F, K, 18) longdouble records and, for
    the slots that are sums, the sums of the absolute values of their terms.  means (F, K, 4) f64: what slots 8-17 are taken
    about, default the f64 quotients of the f64-rounded slots 2-5 and 0."""
    F = len(fields)
    key = np.asarray(key)
    val, mag = np.zeros((F, K, M), dtype=LD), np.zeros((F, K, M), dtype=LD)
    for f, (first, count) in enumerate(fields):
        val[f, :, 8:] = np.nan
        if not count:
            continue
        used, inside, am = lines(p, w, first, count, k, origin)
        kf = key[first - key_first:first - key_first + count]
        for b in range(K):
            m = inside & (kf == b)
            val[f, b, 7] = np.count_nonzero(used & ~inside & (kf == b))
            wt = w[first:first + count, k][m].astype(LD)
            val[f, b, 1] = wt.shape[0]
            if not wt.shape[0]:
                continue
            x = am[m].astype(LD)
            val[f, b, 0] = mag[f, b, 0] = wt.sum()
            for c in range(4):
                val[f, b, 2 + c], mag[f, b, 2 + c] = (wt * x[:, c]).sum(), (wt * np.abs(x[:, c])).sum()
            val[f, b, 6] = mag[f, b, 6] = (wt * np.asarray(wl)[first:first + count][m].astype(LD)).sum()
            if means is None:
                W = np.float64(val[f, b, 0])
                mean = np.array([np.float64(val[f, b, 2 + c]) / W for c in range(4)])
            else:
                mean = np.asarray(means[f][b], dtype=np.float64)
            dx = x - mean.astype(LD)
            for s, (i, j) in enumerate(PAIRS):
                val[f, b, 8 + s], mag[f, b, 8 + s] = (wt * dx[:, i] * dx[:, j]).sum(), (wt * np.abs(dx[:, i] * dx[:, j])).sum()
    return val, mag


def check_records(rec, val, mag, what=""):
    """Device records (F, K, 18) against the truth (val, mag) of `records` taken about the records' own means: counts equal, sums
    within (n + 40) eps sum |terms|, a cell without a ray 0 in slots 0-6 and NaN in slots 8-17.  -> largest share of a bound used."""
    rec = np.asarray(rec, dtype=np.float64).reshape(val.shape)
    assert np.array_equal(rec[..., COUNTS], val[..., COUNTS].astype(np.float64)), f"{what}: counts {rec[..., COUNTS]} against {val[..., COUNTS]}"
    empty = val[..., 1] == 0
    assert np.all(np.isnan(rec[empty][:, 8:])) and np.all(rec[empty][:, :7] == 0), f"{what}: the record of a cell without a ray"
    n, worst = val[..., 1].astype(np.float64), 0.0
    for s in SUMS:
        err = np.abs(rec[~empty][:, s].astype(LD) - val[~empty][:, s]).astype(np.float64)
        bound = sum_bound(n[~empty], mag[~empty][:, s].astype(np.float64))
        assert np.all(err <= bound), f"{what}: slot {s}: error {err} above {bound}"
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0), initial=0.0)))
    print(f"{what}: sums use at most {worst:.3g} of their bound")
    return worst


def directions(field):
    """(F, 2) -> unit vectors, (0, 1) on the axis."""
    out = []
    for x, y in np.asarray(field, dtype=np.float64).reshape(-1, 2):
        h = np.hypot(x, y)
        out.append((x / h, y / h) if np.isfinite(h) and h > 0 else (0.0, 1.0))
    return np.array(out)


def direct(p, w, first, count, k, mask, origin, z, t):
    """The figures of one cell -- the rays of [first, first + count) picked by `mask` -- evaluated directly over its rays in
    longdouble, means and all: dict of band_N, band_power, centroid (2), focus_t, focus_s, focus_rms, rms_t, rms_s, rms_radius on
    the plane z, rms_radius_best.  t: the tangential unit vector."""
    used, inside, am = lines(p, w, first, count, k, origin)
    m = inside & mask
    wt, x = w[first:first + count, k][m].astype(LD), am[m].astype(LD)
    n, o = wt.shape[0], np.asarray(origin, dtype=np.float64).astype(LD)
    nan = LD(np.nan)
    out = dict(band_N=n, band_power=wt.sum())
    if not n:
        out.update(centroid=np.array([nan, nan]), focus_t=nan, focus_s=nan, focus_rms=nan, rms_t=nan, rms_s=nan, rms_radius=nan,
                   rms_radius_best=nan)
        return out
    W = wt.sum()
    zeta = LD(np.float64(z)) - o[2]
    mean = (wt[:, None] * x).sum(axis=0) / W
    dx = x - mean
    out["centroid"] = o[:2] + mean[:2] + zeta * mean[2:]
    tx, ty = LD(t[0]), LD(t[1])

    def along(ux, uy):
        da, dm = ux * dx[:, 0] + uy * dx[:, 1], ux * dx[:, 2] + uy * dx[:, 3]
        V = (wt * dm * dm).sum()
        focus = o[2] - (wt * da * dm).sum() / V if n > 1 and V > 0 else nan
        return focus, np.sqrt((wt * (da + zeta * dm) ** 2).sum() / W)

    out["focus_t"], out["rms_t"] = along(tx, ty)
    out["focus_s"], out["rms_s"] = along(-ty, tx)
    V = (wt * (dx[:, 2] ** 2 + dx[:, 3] ** 2)).sum()
    out["focus_rms"] = o[2] - (wt * (dx[:, 0] * dx[:, 2] + dx[:, 1] * dx[:, 3])).sum() / V if n > 1 and V > 0 else nan
    radius = lambda at: np.sqrt((wt * ((dx[:, 0] + at * dx[:, 2]) ** 2 + (dx[:, 1] + at * dx[:, 3]) ** 2)).sum() / W)
    out["rms_radius"] = radius(zeta)
    out["rms_radius_best"] = radius(out["focus_rms"] - o[2]) if np.isfinite(np.float64(out["focus_rms"])) else nan
    return out
