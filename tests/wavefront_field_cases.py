"""The definition of `Raytracer.wavefront_field` (DESIGN.md "Wavefront across the field"; include/optrace_amd.h, ot_wavefield_*) in
NumPy longdouble, written from that text and using nothing of the package's wavefront-field code: the truth of
tests/test_gpu_wavefront_field.py and tests/test_wavefront_field_host.py.

Storage as in the header: p (N, nt, 3) f64, n (N, nt) f64, w (N, nt) f32, wl (N,) f32; field f owns the rays [first_f, first_f +
count_f); section k.  A ray is used when w[r, k] > 0 and p[r, k + 1] - p[r, k] has a length above 0; its band is its key byte,
255: none.  Rays that are not used, or that have no band, never enter arithmetic.  A cell is a (field, band).

Beside every sum stands the sum of the absolute values of its terms, which `sum_bound` turns into the bound of a sum added in any
order.  The per-ray float64 values u, v and opl are values of the definition: they enter the sums of the moments and of the normal
equations as exact inputs, and `check_planes` holds them to the rounding bounds tests/wavefront_cases.py states for the paths of a
single bundle.  The second pass of the moments and the normal equations take the means and the pupil of the device's own records
as exact inputs: their rounding is an input of that pass, not its error."""
import numpy as np

import chromatic_cases as cc
import wavefront_cases as wc
from chromatic_cases import EPS, LD, NO_BAND, sum_bound  # noqa: F401  (shared with the tests)

FOCUS_M, M, PUPIL_M, MAX_FIELDS, MAX_BANDS, MAX_J = 17, 9, 4, 64, 32, 36
SUMS = [0, 2, 3, 4, 5, 8]


def band_of(key, key_first, first, count):
    return np.asarray(key)[first - key_first:first - key_first + count]


def focus_sums(p, w, fields, k, key, key_first, K, origin):
    """Step 2 -> (val, mag) (F, K, 17) longdouble: per cell the sums of `ot_wavefront_focus` over its used rays and the sums of the
    absolute values of their terms."""
    val, mag = np.zeros((len(fields), K, FOCUS_M), dtype=LD), np.zeros((len(fields), K, FOCUS_M), dtype=LD)
    for f, (first, count) in enumerate(fields):
        if count:
            with np.errstate(all="ignore"):
                val[f], mag[f] = cc.focus_sums(p, w, first, count, k, band_of(key, key_first, first, count), K, origin)
    return val, mag


def has_sphere(s):
    s = np.asarray(s, dtype=np.float64)
    return bool(np.all(np.isfinite(s)) and s[3] != 0)


def paths(p, n, w, fields, k, key, key_first, K, spheres, span):
    """Step 3 -> dict: dense longdouble planes u, v, opl, w of `span` entries from ray key_first on (entry r - key_first: ray r;
    NaN / w = 0 where the ray is not used, has no band, no sphere or misses it), the per-ray bounds b_u, b_v, b_opl, `inside`: the
    entries of the fields, n_missed and n_no_sphere (F, K)."""
    spheres = np.asarray(spheres, dtype=np.float64).reshape(len(fields), K, 4)
    out = {name: np.full(span, np.nan, dtype=LD) for name in ("u", "v", "opl", "b_u", "b_v", "b_opl")}
    out["w"], out["inside"] = np.zeros(span, dtype=LD), np.zeros(span, dtype=bool)
    n_missed, n_no = np.zeros((len(fields), K), dtype=np.int64), np.zeros((len(fields), K), dtype=np.int64)
    for f, (first, count) in enumerate(fields):
        if not count:
            continue
        out["inside"][first - key_first:first - key_first + count] = True
        kf = band_of(key, key_first, first, count)
        used = cc.used_rays(p, w, first, count, k)[0]
        for b in range(K):
            idx = first + np.nonzero(used & (kf == b))[0]
            if not idx.shape[0]:
                continue
            if not has_sphere(spheres[f, b]):
                n_no[f, b] = idx.shape[0]
                continue
            one = wc.paths(p[idx], n[idx], w[idx], k, 0, idx.shape[0], spheres[f, b, :3], spheres[f, b, 3])
            n_missed[f, b] = one["n_missed"]
            for name in ("u", "v", "opl", "b_u", "b_v", "b_opl", "w"):
                out[name][idx - key_first] = one[name]
    out["n_missed"], out["n_no_sphere"] = n_missed, n_no
    return out


def check_planes(u, v, opl, w_out, truth, what=""):
    """The device's planes against `paths`: the same entries used, w_out the stored weight, u, v and opl within the per-ray bounds;
    entries of the fields that are not used hold w_out = 0 and NaN."""
    u, v, opl, w_out = (np.asarray(a) for a in (u, v, opl, w_out))
    inside, hit = truth["inside"], truth["w"] > 0
    assert np.array_equal(w_out[inside].astype(LD), truth["w"][inside]), f"{what}: the weights of the planes"
    rest = inside & ~hit
    assert np.all(np.isnan(u[rest])) and np.all(np.isnan(v[rest])) and np.all(np.isnan(opl[rest])), f"{what}: entries that are not used"
    for name, got in (("u", u), ("v", v), ("opl", opl)):
        err = np.abs(got[hit].astype(LD) - truth[name][hit])
        assert np.all(err <= truth["b_" + name][hit]), f"{what}: {name} off by {err.max()} somewhere"


def counted(w_out, key, key_first, first, count, K):
    """Per band the entries of a field that count: key a band and w_out > 0.  -> list of index arrays into the planes."""
    kf = band_of(key, key_first, first, count)
    wf = np.asarray(w_out)[first - key_first:first - key_first + count]
    return [first - key_first + np.nonzero((kf == b) & (wf > 0))[0] for b in range(K)]


def moments(u, v, opl, w_out, wl, fields, key, key_first, K, means=None, centre=None):
    """Step 4 -> (val, mag (F, K, 9), pupil (F, 4)) longdouble from the float64 planes (entry i: ray key_first + i; wl likewise).
    means (F, K) f64: what slot 8 is taken about, default the f64 quotient of the f64-rounded slots 2 and 0; centre (F, 2) f64:
    what the pupil's largest distance is taken about, default the f64 quotients of the f64-rounded band sums added in band order."""
    F = len(fields)
    val, mag, pupil = np.zeros((F, K, M), dtype=LD), np.zeros((F, K, M), dtype=LD), np.zeros((F, PUPIL_M), dtype=LD)
    for f, (first, count) in enumerate(fields):
        val[f, :, 8] = np.nan
        if not count:
            pupil[f, :2] = np.nan
            continue
        cells = counted(w_out, key, key_first, first, count, K)
        for b, idx in enumerate(cells):
            if not idx.shape[0]:
                continue
            wt, l = np.asarray(w_out)[idx].astype(LD), np.asarray(opl)[idx].astype(LD)
            val[f, b, 0] = mag[f, b, 0] = wt.sum()
            val[f, b, 1] = idx.shape[0]
            for s, a in ((2, l), (3, np.asarray(u)[idx].astype(LD)), (4, np.asarray(v)[idx].astype(LD)), (5, np.asarray(wl)[idx].astype(LD))):
                val[f, b, s], mag[f, b, s] = (wt * a).sum(), (wt * np.abs(a)).sum()
            val[f, b, 6], val[f, b, 7] = l.min(), l.max()
            mean = np.float64(val[f, b, 2]) / np.float64(val[f, b, 0]) if means is None else np.float64(means[f][b])
            t = wt * (l - LD(mean)) ** 2
            val[f, b, 8] = mag[f, b, 8] = t.sum()
        if centre is None:
            W = su = sv = np.float64(0)
            for b in range(K):
                W, su, sv = W + np.float64(val[f, b, 0]), su + np.float64(val[f, b, 3]), sv + np.float64(val[f, b, 4])
            with np.errstate(invalid="ignore", divide="ignore"):
                c = np.array([su / W, sv / W])
        else:
            c = np.asarray(centre[f], dtype=np.float64)
        pupil[f, :2] = c
        every = np.concatenate(cells)
        if every.shape[0]:
            pupil[f, 2] = ((np.asarray(u)[every].astype(LD) - LD(c[0])) ** 2 + (np.asarray(v)[every].astype(LD) - LD(c[1])) ** 2).max()
        pupil[f, 3] = np.sqrt(pupil[f, 2])
    return val, mag, pupil


def record_means(mom):
    """The mean path the device forms from its moments records (..., 9) f64: one IEEE quotient per cell."""
    mom = np.asarray(mom, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        return mom[..., 2] / mom[..., 0]


def check_moments(mom, pupil, val, mag, tpupil, what=""):
    """Device records (F, K, 9) and pupil (F, 4) against `moments` taken about the records' own means and centre: counts, minimum
    and maximum equal, sums within (n + 40) eps sum |terms|; a cell without an entry 0 in slots 0 - 7 and NaN in slot 8; the
    largest squared distance within 8 eps (two differences, two squares, a sum), its root the IEEE root of the device's own
    number.  -> largest share of a bound used."""
    mom, pupil = np.asarray(mom, dtype=np.float64).reshape(val.shape), np.asarray(pupil, dtype=np.float64).reshape(tpupil.shape)
    assert np.array_equal(mom[..., 1], val[..., 1].astype(np.float64)), f"{what}: counts {mom[..., 1]} against {val[..., 1]}"
    empty = val[..., 1] == 0
    assert np.all(mom[empty][:, :8] == 0) and np.all(np.isnan(mom[empty][:, 8])), f"{what}: the record of a cell without an entry"
    assert np.array_equal(mom[~empty][:, 6:8], val[~empty][:, 6:8].astype(np.float64)), f"{what}: minimum and maximum"
    n, worst = val[..., 1].astype(np.float64), 0.0
    for s in SUMS:
        err = np.abs(mom[~empty][:, s].astype(LD) - val[~empty][:, s]).astype(np.float64)
        bound = sum_bound(n[~empty], mag[~empty][:, s].astype(np.float64))
        assert np.all(err <= bound), f"{what}: slot {s}: error {err} above {bound}"
        with np.errstate(invalid="ignore", divide="ignore"):
            worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0), initial=0.0)))
    some = ~np.all(empty, axis=1)
    r2 = tpupil[some][:, 2].astype(np.float64)
    assert np.all(np.abs(pupil[some][:, 2] - r2) <= 8 * EPS * r2), f"{what}: largest squared distance {pupil[:, 2]} against {tpupil[:, 2]}"
    assert np.array_equal(pupil[:, 3], np.sqrt(pupil[:, 2])), f"{what}: the pupil radius is the root of the largest squared distance"
    assert np.all(pupil[~some][:, 2:] == 0), f"{what}: the pupil of a field without an entry"
    print(f"{what}: moments use at most {worst:.3g} of their bound")
    return worst


def centre_bound(val, mag):
    """How far the f64 centre (sum_b slot 3, sum_b slot 4) / sum_b slot 0 of sums within their bounds may lie from the true one, per
    field: to first order (d3 + |c| d0) / W, doubled for the higher orders, plus 4 eps |c| for the K additions' rounding being in
    the bounds already and the quotient.  -> (true centre (F, 2) longdouble, bound (F, 2))."""
    n = val[..., 1].astype(np.float64)
    W = val[..., 0].sum(axis=1)
    d0 = sum_bound(n, mag[..., 0].astype(np.float64)).sum(axis=1) + EPS * val.shape[1] * W.astype(np.float64)
    out, bound = np.full((val.shape[0], 2), np.nan, dtype=LD), np.zeros((val.shape[0], 2))
    for c, s in enumerate((3, 4)):
        with np.errstate(invalid="ignore", divide="ignore"):
            out[:, c] = val[..., s].sum(axis=1) / W
            ds = sum_bound(n, mag[..., s].astype(np.float64)).sum(axis=1) + EPS * val.shape[1] * mag[..., s].sum(axis=1).astype(np.float64)
            bound[:, c] = 2 * (ds + np.abs(out[:, c].astype(np.float64)) * d0) / W.astype(np.float64) + 4 * EPS * np.abs(out[:, c].astype(np.float64))
    return out, bound


def normal_equations(u, v, opl, w_out, fields, key, key_first, K, mom, pupil, pupil_radius, J):
    """Step 5 -> per cell (f, b) a tuple (G, |terms| of G, g, |terms| of g, entries in the sums) as
    `wavefront_cases.normal_equations` forms them, Z at ((u, v) - the field's centre) / pupil radius, opd against the cell's mean:
    the means, the centre and the radius are the device's own (mom (F, K, 9), pupil (F, 4))."""
    mom, pupil = np.asarray(mom, dtype=np.float64), np.asarray(pupil, dtype=np.float64)
    out = {}
    for f, (first, count) in enumerate(fields):
        if not count:
            continue
        for b, idx in enumerate(counted(w_out, key, key_first, first, count, K)):
            if not idx.shape[0]:
                continue
            rec = np.zeros(11)  # (a single-bundle record whose quotients are the cell's mean and the field's pupil)
            rec[0], rec[2], rec[3], rec[4], rec[10] = 1.0, record_means(mom[f, b]), pupil[f, 0], pupil[f, 1], pupil[f, 3]
            out[f, b] = wc.normal_equations(np.asarray(u)[idx], np.asarray(v)[idx], np.asarray(opl)[idx], np.asarray(w_out)[idx].astype(np.float64),
                                            rec, pupil_radius, J)
    return out


def unpack(packed, J):
    """out of `ot_wavefield_zernike` for one cell -> (G (J, J) symmetric, g (J,))."""
    tri = J * (J + 1) // 2
    G = np.zeros((J, J))
    G[np.triu_indices(J)] = packed[:tri]
    return G + np.triu(G, 1).T, np.array(packed[tri:tri + J])


def check_normal(normal, truth, F, K, J, what=""):
    """Device normal equations (F, K, T) against `normal_equations`: every entry within (n + 40) eps sum |terms|; a cell without an
    entry holds zeros.  -> largest share of a bound used."""
    normal = np.asarray(normal, dtype=np.float64).reshape(F, K, -1)
    worst = 0.0
    for f in range(F):
        for b in range(K):
            G, g = unpack(normal[f, b], J)
            if (f, b) not in truth:
                assert np.all(normal[f, b] == 0), f"{what}: cell ({f}, {b}) has no entry, but sums"
                continue
            tG, aG, tg, ag, n = truth[f, b]
            for got, want, mag, name in ((G, tG, aG, "G"), (g, tg, ag, "g")):
                err = np.abs(got.astype(LD) - want).astype(np.float64)
                bound = sum_bound(n, mag.astype(np.float64))
                assert np.all(err <= bound), f"{what}: {name} of cell ({f}, {b}): error {err.max()} above its bound"
                with np.errstate(invalid="ignore", divide="ignore"):
                    worst = max(worst, float(np.nanmax(np.where(bound > 0, err / bound, 0.0), initial=0.0)))
    print(f"{what}: normal equations use at most {worst:.3g} of their bound")
    return worst


def solve_ld(G, g):
    """G a = g by Gaussian elimination with partial pivoting in longdouble; None where a pivot vanishes."""
    A = np.concatenate([np.asarray(G, dtype=LD), np.asarray(g, dtype=LD)[:, None]], axis=1)
    J = A.shape[0]
    for i in range(J):
        piv = i + int(np.argmax(np.abs(A[i:, i])))
        if A[piv, i] == 0:
            return None
        A[[i, piv]] = A[[piv, i]]
        A[i] = A[i] / A[i, i]
        for r in range(J):
            if r != i:
                A[r] = A[r] - A[r, i] * A[i]
    return A[:, J]


def evaluate(p, n, w, wl, fields, k, key, key_first, K, spheres, J, pupil_radius=None):
    """The whole definition from the sphere table on, longdouble throughout (the paths in longdouble too: no float64 inputs): dict
    of band_N, band_power, n_missed, n_no_sphere, opl_mean, opd_rms, opd_min, opd_max, pupil_centre, pupil_radius, zernike (F, K, J;
    NaN where the cell has no entry or its system no solution)."""
    span = max([a + c for a, c in fields if c] + [key_first]) - key_first
    P = paths(p, n, w, fields, k, key, key_first, K, spheres, span)
    F = len(fields)
    wl_d = np.zeros(span)
    hi = min(key_first + span, len(wl))
    wl_d[:hi - key_first] = np.asarray(wl)[key_first:hi]
    means = np.full((F, K), np.nan, dtype=LD)
    out = dict(n_missed=P["n_missed"], n_no_sphere=P["n_no_sphere"], band_N=np.zeros((F, K), dtype=np.int64),
               band_power=np.zeros((F, K), dtype=LD), zernike=np.full((F, K, J), np.nan, dtype=LD),
               pupil_centre=np.full((F, 2), np.nan, dtype=LD), pupil_radius=np.full(F, np.nan, dtype=LD))
    for name in ("opl_mean", "opd_rms", "opd_min", "opd_max"):
        out[name] = np.full((F, K), np.nan, dtype=LD)
    for f, (first, count) in enumerate(fields):
        if not count:
            continue
        cells = counted(P["w"], key, key_first, first, count, K)
        every = np.concatenate(cells)
        if not every.shape[0]:
            continue
        we = P["w"][every]
        c = np.array([(we * P["u"][every]).sum(), (we * P["v"][every]).sum()]) / we.sum()
        r = np.sqrt(((P["u"][every] - c[0]) ** 2 + (P["v"][every] - c[1]) ** 2).max()) if pupil_radius is None else LD(pupil_radius)
        out["pupil_centre"][f], out["pupil_radius"][f] = c, r
        for b, idx in enumerate(cells):
            if not idx.shape[0]:
                continue
            wt, l = P["w"][idx], P["opl"][idx]
            W = wt.sum()
            mean = (wt * l).sum() / W
            out["band_N"][f, b], out["band_power"][f, b], out["opl_mean"][f, b] = idx.shape[0], W, mean
            out["opd_rms"][f, b] = np.sqrt((wt * (l - mean) ** 2).sum() / W)
            out["opd_min"][f, b], out["opd_max"][f, b] = l.min() - mean, l.max() - mean
            x, y = ((P["u"][idx] - c[0]) / r, (P["v"][idx] - c[1]) / r) if r > 0 else (np.zeros_like(l), np.zeros_like(l))
            sel = np.ones(idx.shape[0], dtype=bool) if pupil_radius is None else ~(x * x + y * y > 1)
            Z = np.array([wc.zernike_ld(j, x[sel], y[sel]) for j in range(1, J + 1)], dtype=LD).reshape(J, -1)
            a = solve_ld((Z * wt[sel]) @ Z.T, (Z * wt[sel]) @ (l[sel] - mean))
            if a is not None and np.all(np.isfinite(a.astype(np.float64))):
                out["zernike"][f, b] = a
    return out
