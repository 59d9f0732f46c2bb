"""The definition of the beam footprints (DESIGN.md "Footprints"; include/optrace_amd.h, ot_footprint_moments) in NumPy longdouble,
written from that text and using nothing of the package's footprint code.

Storage as in the header: p (N, nt, 3) f64, p[r, i] where section i of ray r starts; w (N, nt) f32, the ray's weight in section
i; rays r in [first, first + count).  Per section i: the living rays T = {w[r, i] > 0}, the arriving rays A = {w[r, i - 1] > 0}
(A = T in section 0, with w_in = w[r, 0]).  Positions and weights of rays outside T and A are never read into arithmetic: a NaN
there does no harm.

Beside every sum stands the sum of the absolute values of its terms, which `sum_bound` turns into the bound of a sum added in
any order.  The second-pass slots 13-15 take the centroid as an exact input -- the device's own, formed from its record, when one is
given: its rounding is an input of that pass and not its error."""
import numpy as np

LD = np.longdouble
EPS = np.finfo(np.float64).eps
M = 17
M_OPS = 40  # operations per term the bounds of the reduced sums allow for
SUMS = [0, 2, 4, 5, 6, 13, 14, 15]
COUNTS = [1, 3]
EXTREMES = list(range(7, 13))


def sum_bound(n_terms, abs_sum):
    """|rounded sum - sum| for n_terms terms of M_OPS operations each, added in any order."""
    return (n_terms + M_OPS) * EPS * np.asarray(abs_sum, dtype=np.float64)


def sets(w, first, count, i):
    """-> (alive, arriving): boolean masks over the rays [first, first + count) of section i."""
    ws = w[first:first + count]
    alive = ws[:, i] > 0
    return alive, (ws[:, i - 1] > 0 if i else alive)


def records(p, w, first, count, axis, centroid=None):
    """-> (val, mag): (nt, 17) longdouble records and, for the slots that are sums, the sums of the absolute values of their terms
    (0 elsewhere).  axis (nt, 2); centroid (nt, 2) f64: what slots 13-15 are taken about, default the f64 quotients of the
    f64-rounded slots 4, 5 and 0."""
    nt = w.shape[1]
    axis = np.asarray(axis, dtype=np.float64).reshape(nt, 2)
    val, mag = np.zeros((nt, M), dtype=LD), np.zeros((nt, M), dtype=LD)
    for i in range(nt):
        alive, arriving = sets(w, first, count, i)
        wt = w[first:first + count, i][alive].astype(LD)
        w_in = w[first:first + count, i - 1 if i else 0][arriving].astype(LD)
        pt = p[first:first + count, i][alive].astype(LD)  # (n, 3): the living rays' alone
        val[i, 0] = mag[i, 0] = wt.sum()
        val[i, 1] = wt.shape[0]
        val[i, 2] = mag[i, 2] = w_in.sum()
        val[i, 3] = w_in.shape[0]
        if not wt.shape[0]:
            val[i, 7:13] = np.nan
            continue
        for c in range(3):
            val[i, 4 + c] = (wt * pt[:, c]).sum()
            mag[i, 4 + c] = (wt * np.abs(pt[:, c])).sum()
            val[i, 7 + 2 * c], val[i, 8 + 2 * c] = pt[:, c].min(), pt[:, c].max()
        if centroid is None:
            W = np.float64(val[i, 0])
            cx, cy = np.float64(val[i, 4]) / W, np.float64(val[i, 5]) / W
        else:
            cx, cy = (np.float64(v) for v in centroid[i])
        dx, dy = pt[:, 0] - LD(cx), pt[:, 1] - LD(cy)
        val[i, 13] = mag[i, 13] = (wt * dx * dx).sum()
        val[i, 14] = mag[i, 14] = (wt * dy * dy).sum()
        val[i, 15] = (wt * dx * dy).sum()
        mag[i, 15] = (wt * np.abs(dx * dy)).sum()
        ux, uy = pt[:, 0] - LD(axis[i, 0]), pt[:, 1] - LD(axis[i, 1])
        val[i, 16] = (ux * ux + uy * uy).max()
    return val, mag


def record_centroid(rec):
    """The centroid the device forms from its record (nt, 17) f64: two IEEE quotients per section."""
    rec = np.asarray(rec, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([rec[:, 4] / rec[:, 0], rec[:, 5] / rec[:, 0]], axis=1)


def cells(p, w, first, count, axis, rec, n_px, i):
    """Cell (row, column) of every living ray of section i, formed in f64 from the record `rec` (nt, 17) exactly as written:
    R = sqrt(rec[i, 16]), column = min(floor(((x - ax) + R) / (2 R) n_px), n_px - 1), not below 0 (|x - ax| <= R holds up to the
    rounding of the root), row likewise from y; cell 0, 0 when R = 0.  -> (rows, columns, weights f64) of the living rays."""
    alive, _ = sets(w, first, count, i)
    x = p[first:first + count, i, 0][alive].astype(np.float64)
    y = p[first:first + count, i, 1][alive].astype(np.float64)
    wt = w[first:first + count, i][alive].astype(np.float64)
    R = np.sqrt(np.float64(rec[i, 16]))
    if not R > 0:
        z = np.zeros(x.shape[0], dtype=np.int64)
        return z, z, wt
    ax, ay = (np.float64(a) for a in np.asarray(axis, dtype=np.float64).reshape(-1, 2)[i])
    fn = np.float64(n_px)
    col = np.floor(((x - ax) + R) / (2.0 * R) * fn)
    row = np.floor(((y - ay) + R) / (2.0 * R) * fn)
    clip = lambda q: np.clip(q, 0, n_px - 1).astype(np.int64)
    return clip(row), clip(col), wt


def maps(p, w, first, count, axis, rec, n_px):
    """-> (val, n_terms): (nt, n_px, n_px) longdouble sums of w per cell (all terms are positive: the sum is its own magnitude)
    and the number of rays per cell."""
    nt = w.shape[1]
    val, cnt = np.zeros((nt, n_px * n_px), dtype=LD), np.zeros((nt, n_px * n_px), dtype=np.int64)
    for i in range(nt):
        row, col, wt = cells(p, w, first, count, axis, rec, n_px, i)
        np.add.at(val[i], row * n_px + col, wt.astype(LD))
        np.add.at(cnt[i], row * n_px + col, 1)
    return val.reshape(nt, n_px, n_px), cnt.reshape(nt, n_px, n_px)


def check_record(rec, val, mag, what=""):
    """The bounds of the feature on a device record `rec` (nt, 17) against the truth (val, mag) of `records` taken about the
    record's own centroid: counts equal, extremes bit-equal, slot 16 within 4 eps relative, sums within
    (n + 40) eps sum |terms|."""
    rec = np.asarray(rec, dtype=np.float64)
    assert np.array_equal(rec[:, COUNTS], val[:, COUNTS].astype(np.float64)), f"{what}: counts"
    assert np.array_equal(rec[:, EXTREMES], val[:, EXTREMES].astype(np.float64), equal_nan=True), f"{what}: extremes"
    err16 = np.abs(rec[:, 16].astype(LD) - val[:, 16])
    assert np.all(err16 <= 4 * EPS * val[:, 16]), f"{what}: slot 16 off by {err16.astype(np.float64)}"
    n_t, n_a = val[:, 1].astype(np.float64), val[:, 3].astype(np.float64)
    worst = 0.0
    for s in SUMS:
        n = n_a if s == 2 else n_t
        err = np.abs(rec[:, s].astype(LD) - val[:, s]).astype(np.float64)
        bound = sum_bound(n, mag[:, s].astype(np.float64))
        assert np.all(err <= bound), f"{what}: slot {s}: error {err} above {bound}"
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0))))
    print(f"{what}: sums use at most {worst:.3g} of their bound; slot 16 off by at most {float(err16.max()):.3g}")
