"""The definition of `Raytracer.ray_fans` ("Ray fans"; include/optrace_amd.h, ot_fans_*) restated in NumPy longdouble:
the truth of tests/test_gpu_fans.py and tests/test_fans_host.py, written from that text and using nothing of the package's fans
code.  No device is needed here.

Beside every reduced sum stands the sum of the absolute values of its terms, which `wavefront_cases.sum_bound` turns into the bound
of a sum added in any order, (n + 40) eps sum |terms|.  Differences the device forms from the results of an earlier pass (the
means of a band's record, the pupil centre and radius of the moments record) are formed here from the same numbers, so they are
exact inputs on both sides.  Unit-disc coordinates, slab tests and bin indices are formed in float64 with the definition's own
expressions, one IEEE operation each: a ray then lands in the device's bin.

The transverse aberration is a per-ray value.  With d = p[k + 1] - p[k] and t = (f_z - p_z) / d_z, ex = p_x + t d_x - f_x takes seven
roundings from stored numbers: d_x, d_z and f_z - p_z (relative eps / 2 each, of themselves), the quotient, the product t d_x, and
the two sums.  To first order t d_x carries 5 of them, eps / 2 |t d_x| each, the first sum eps / 2 (|p_x| + |t d_x|), the second
eps / 2 (|p_x| + |t d_x| + |f_x|): together below 3.5 eps (|p_x| + |t d_x| + |f_x|).  `transverse` allows 4 eps of that magnitude,
which leaves the second-order terms their room."""
import numpy as np

from wavefront_cases import sum_bound

LD = np.longdouble
EPS = np.finfo(np.float64).eps
M, BIN_M, MAX_BINS, MAX_BANDS, NO_BAND = 13, 6, 256, 32, 255
SUMS1, SUMS2 = [0, 2, 3, 4, 5], [8, 9, 10, 11]  # the slots of a record that are sums, by pass


def transverse(p, w_out, first, count, k, focus):
    """Step 2 for the rays [first, first + count) of p (N, nt, 3): dict of ex, ey (longdouble, NaN for rays without weight and for
    parallel ones), their per-ray bounds b_ex, b_ey, w (float32: w_out with 0 for the parallel rays) and n_parallel."""
    w_out = np.asarray(w_out, dtype=np.float32)
    f = np.asarray(focus, dtype=np.float64).astype(LD)
    alive = w_out > 0
    p0 = np.where(alive[:, None], p[first:first + count, k], 0.0).astype(LD)
    d = np.where(alive[:, None], p[first:first + count, k + 1], 0.0).astype(LD) - p0
    flat = alive & (d[:, 2] == 0)
    used = alive & ~flat
    t = np.zeros(count, dtype=LD)
    t[used] = (f[2] - p0[used, 2]) / d[used, 2]
    out = {"w": np.where(flat, np.float32(0), w_out), "n_parallel": int(np.count_nonzero(flat))}
    for c, name in ((0, "ex"), (1, "ey")):
        e = np.full(count, np.nan, dtype=LD)
        b = np.full(count, np.nan, dtype=LD)
        e[used] = p0[used, c] + t[used] * d[used, c] - f[c]
        b[used] = 4 * EPS * (np.abs(p0[used, c]) + np.abs(t[used] * d[used, c]) + abs(f[c]))
        out[name], out["b_" + name] = e, b
    return out


def check_transverse(ex, ey, w, n_parallel, truth, what=""):
    """The device's planes against `transverse`: NaN where the truth has NaN, within the per-ray bound elsewhere; w and the count
    of parallel rays equal."""
    assert np.array_equal(np.asarray(w, dtype=np.float32), truth["w"]), f"{what}: weights"
    assert int(n_parallel) == truth["n_parallel"], f"{what}: {n_parallel} parallel rays, expected {truth['n_parallel']}"
    worst = 0.0
    for got, name in ((ex, "ex"), (ey, "ey")):
        e, b = truth[name], truth["b_" + name]
        none = np.isnan(e.astype(np.float64))
        assert np.array_equal(np.isnan(got), none), f"{what}: {name}: NaN in other places than the truth"
        err = np.abs(np.asarray(got)[~none].astype(LD) - e[~none])
        assert np.all(err <= b[~none]), f"{what}: {name} off by {float((err - b[~none]).max()):.3e} beyond the bound"
        if err.shape[0]:
            with np.errstate(invalid="ignore", divide="ignore"):
                worst = max(worst, float(np.nanmax(np.where(b[~none] > 0, err / b[~none], 0.0))))
    return worst


def record_means(rec):
    """(K, 3) float64: mean opl, ex, ey as the device forms them from its records, three IEEE quotients per band."""
    rec = np.asarray(rec, dtype=np.float64).reshape(-1, M)
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([rec[:, 2] / rec[:, 0], rec[:, 3] / rec[:, 0], rec[:, 4] / rec[:, 0]], axis=1)


def band_records(opl, ex, ey, w, wl, key, K, means=None):
    """Step 4 -> (val, mag): (K, 13) longdouble records and, for the slots that are sums, the sums of |terms|.  means (K, 3) f64:
    what pass 2 is taken about, default the f64 quotients of the f64-rounded sums of pass 1."""
    key, w = np.asarray(key), np.asarray(w)
    val, mag = np.zeros((K, M), dtype=LD), np.zeros((K, M), dtype=LD)
    for b in range(K):
        m = (key == b) & (w > 0)
        n = int(np.count_nonzero(m))
        val[b, 1] = n
        if not n:
            val[b, 9:12] = np.nan
            continue
        wt, l, x, y, lam = (np.asarray(a)[m].astype(LD) for a in (w, opl, ex, ey, wl))
        val[b, 0] = mag[b, 0] = wt.sum()
        for slot, a in ((2, l), (3, x), (4, y), (5, lam)):
            val[b, slot], mag[b, slot] = (wt * a).sum(), (wt * np.abs(a)).sum()
        val[b, 6], val[b, 7] = l.min(), l.max()
        if means is None:
            W = np.float64(val[b, 0])
            mo, mx, my = (np.float64(val[b, s]) / W for s in (2, 3, 4))
        else:
            mo, mx, my = (np.float64(a) for a in means[b])
        d, dx, dy = l - LD(mo), x - LD(mx), y - LD(my)
        val[b, 8] = mag[b, 8] = (wt * d * d).sum()
        val[b, 9] = mag[b, 9] = (wt * dx * dx).sum()
        val[b, 10] = mag[b, 10] = (wt * dy * dy).sum()
        val[b, 11], mag[b, 11] = (wt * dx * dy).sum(), (wt * np.abs(dx * dy)).sum()
        val[b, 12] = (dx * dx + dy * dy).max()
    return val, mag


def check_records(rec, val, mag, what=""):
    """A device record (K, 13) against `band_records` taken about the record's own means: counts and the extremes of opl equal,
    slot 12 within 4 eps relative (two subtractions, two squares, one sum), sums within (n + 40) eps sum |terms|; an empty band:
    zeros, NaN in slots 9 .. 11."""
    rec = np.asarray(rec, dtype=np.float64).reshape(-1, M)
    assert np.array_equal(rec[:, 1], val[:, 1].astype(np.float64)), f"{what}: counts {rec[:, 1]} against {val[:, 1]}"
    assert np.array_equal(rec[:, 6:8], val[:, 6:8].astype(np.float64)), f"{what}: the extremes of opl"
    err12 = np.abs(rec[:, 12].astype(LD) - val[:, 12])
    assert np.all(err12 <= 4 * EPS * val[:, 12]), f"{what}: slot 12 off by {err12.astype(np.float64)}"
    empty = val[:, 1] == 0
    assert np.all(np.isnan(rec[empty][:, 9:12])) and np.all(rec[empty][:, [0, 1, 2, 3, 4, 5, 6, 7, 8, 12]] == 0), f"{what}: an empty band"
    n, worst = val[:, 1].astype(np.float64), 0.0
    for s in SUMS1 + SUMS2:
        err = np.abs(rec[~empty, s].astype(LD) - val[~empty, s]).astype(np.float64)
        bound = sum_bound(n[~empty], mag[~empty, s].astype(np.float64))
        assert np.all(err <= bound), f"{what}: slot {s}: error {err} above {bound}"
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0), initial=0.0)))
    return worst


def unit_disc(u, v, w, mom, pupil_radius):
    """Step 1, the unit-disc coordinates, in float64 and in the order of the definition (`wf_unit_disc`): centre = slots 3 and 4
    over slot 0 of the moments record, radius = its slot 10 or the caller's.  -> (entries that count, x, y)"""
    mom = np.asarray(mom, dtype=np.float64)
    u, v = np.asarray(u, dtype=np.float64), np.asarray(v, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):  # (no entry that counts: no centre, and nothing reads it)
        cu, cv = mom[3] / mom[0], mom[4] / mom[0]
    pr = np.float64(mom[10] if pupil_radius is None else pupil_radius)
    sel = np.asarray(w) > 0
    x, y = np.zeros_like(u), np.zeros_like(v)
    if pr > 0:
        x[sel], y[sel] = (u[sel] - cu) / pr, (v[sel] - cv) / pr
    if pupil_radius is not None:
        sel = sel & ~(x * x + y * y > 1)
    return sel, x, y


def bin_index(c, n_bins):
    """min(floor((c + 1) / 2 n_bins), n_bins - 1), not below 0, in float64."""
    return np.clip(np.floor((np.asarray(c, dtype=np.float64) + 1.0) / 2.0 * n_bins), 0, n_bins - 1).astype(np.int64)


def fan_bins(u, v, opl, ex, ey, w, key, K, mom, pupil_radius, rec, n_bins, slab):
    """Step 5 -> (val, mag, passed): (K, 2, n_bins, 6) longdouble sums and sums of |terms|; passed (2,): the rays of any band that
    pass each slab test.  rec (K, 13): the records whose mean opl the path differences are taken against."""
    sel, x, y = unit_disc(u, v, w, mom, pupil_radius)
    key = np.asarray(key)
    sel = sel & (key < K)
    mean = record_means(rec)[:, 0]
    val, mag = np.zeros((K, 2, n_bins, BIN_M), dtype=LD), np.zeros((K, 2, n_bins, BIN_M), dtype=LD)
    passed = []
    for fan, (cut, c) in enumerate(((x, y), (y, x))):
        m = sel & (np.abs(cut) <= np.float64(slab))
        passed.append(int(np.count_nonzero(m)))
        b, at = key[m].astype(np.int64), bin_index(c[m], n_bins)
        wt = np.asarray(w)[m].astype(LD)
        opd = np.asarray(opl)[m].astype(LD) - mean[b].astype(LD)
        terms = (wt, np.ones_like(wt), wt * c[m].astype(LD), wt * np.asarray(ex)[m].astype(LD), wt * np.asarray(ey)[m].astype(LD), wt * opd)
        for s, t in enumerate(terms):
            np.add.at(val[:, fan, :, s], (b, at), t)
            np.add.at(mag[:, fan, :, s], (b, at), np.abs(t))
    return val, mag, np.array(passed)


def check_bins(out, val, mag, what="", factor=1.0):
    """Device bins (K, 2, n_bins, 6) against `fan_bins`: counts equal, every other sum within factor (n + 40) eps sum |terms|, n
    the rays of its bin."""
    out = np.asarray(out, dtype=np.float64).reshape(val.shape)
    n = val[..., 1].astype(np.float64)
    assert np.array_equal(out[..., 1], n), f"{what}: the bins' counts"
    worst = 0.0
    for s in (0, 2, 3, 4, 5):
        err = np.abs(out[..., s].astype(LD) - val[..., s]).astype(np.float64)
        bound = factor * sum_bound(n, mag[..., s].astype(np.float64))
        assert np.all(err <= bound), f"{what}: bin slot {s}: off by {(err - bound).max():.3e} beyond the bound"
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0), initial=0.0)))
    return worst


def figures(rec, bins):
    """The figures of `ot.RayFans` from records and bins, longdouble: dict."""
    rec, bins = np.asarray(rec).astype(LD), np.asarray(bins).astype(LD)
    some = rec[:, 1] > 0
    with np.errstate(invalid="ignore", divide="ignore"):
        W = np.where(some, rec[:, 0], LD(np.nan))
        mean = rec[:, 2] / W
        lam = rec[:, 5] / W
        rms = np.sqrt(rec[:, 8] / W)
        Wb = np.where(bins[..., 1] > 0, bins[..., 0], LD(np.nan))
        return dict(wavelengths=lam, opl_mean=mean, opd_rms=rms, opd_min=rec[:, 6] - mean, opd_max=rec[:, 7] - mean,
                    opd_pv=rec[:, 7] - rec[:, 6] + 0 * W, opd_rms_waves=rms / (lam * LD(1e-6)), centroid=rec[:, 3:5] / W[:, None],
                    rms_x=np.sqrt(rec[:, 9] / W), rms_y=np.sqrt(rec[:, 10] / W), rms_radius=np.sqrt((rec[:, 9] + rec[:, 10]) / W),
                    max_radius=np.sqrt(rec[:, 12]) + 0 * W, weight=bins[..., 0], count=bins[..., 1], pupil=bins[..., 2] / Wb,
                    ex=bins[..., 3] / Wb, ey=bins[..., 4] / Wb, opd=bins[..., 5] / Wb)
