"""The definition of the MTF analysis (DESIGN.md "MTF analysis"; include/optrace_amd.h, ot_mtf_sums) in NumPy longdouble, written
from that text and using nothing of the package's MTF code.

Storage, used rays, bands and the ray lines (a, m) are those of the field analysis (tests/field_cases.py).  About the means of
the cell -- four f64 quotients of its `ot_field_sums` record, the device's own or the oracle's --, da = a - mean_a and
dm = m - mean_m, and with t of the field and s = (-t_y, t_x)

    al_t = t_x da_x + t_y da_y   mu_t = t_x dm_x + t_y dm_y   al_s = s_x da_x + s_y da_y   mu_s = s_x dm_x + s_y dm_y

are formed in float64 in this order (`line_terms`): per-ray values of the definition, which enter the sums as exact inputs.
e = al + zeta mu, tau = nu e, tau -= rint(tau) and the sine and cosine of 2 pi tau are formed in longdouble.  Beside every sum stands
its allowance

    (n + 40) eps sum w  +  sum_r min(2 w_r, w_r (2 pi 3 eps |nu| (|al_r| + |zeta mu_r|) + 4 eps)),      eps = 2^-52:

a sum of n terms of at most w_r each, added in any order; two roundings in e and one in tau, at the slope 2 pi of the sine and
cosine in tau; under 1 ulp each for the device's sine and cosine and for the product with w, doubled.  A term is never off by more
than 2 w_r, whatever its phase: the cap of a ray that lies far away."""
import numpy as np

import field_cases as fc
from field_cases import EPS, LD, NO_BAND  # noqa: F401  (shared with the tests)

MAX_FREQ, MAX_PLANES, PAIRS, BLOCKS, MIN_BLOCKS = 64, 65, 8, 1024, 16
PI = LD(4) * np.arctan(LD(1))


def workspace(counts, K, Z, Q):
    """Doubles `ot_mtf_workspace` asks for (include/optrace_amd.h), for fields of `counts` rays, each below 2^28."""
    KB = min(K, 4)
    tile = 3 if KB == 3 else PAIRS // KB
    groups, tiles = -(-K // KB), -(-Z * Q // tile)
    cap = max(MIN_BLOCKS, BLOCKS // (groups * tiles))
    longest = max(1, max(min(-(-n // 256), cap) for n in counts))
    return len(counts) * longest * groups * tiles * KB * 4 * tile


def line_terms(am, mean, t):
    """am (n, 4) f64: a_x, a_y, m_x, m_y of a cell's rays; mean (4,) f64; t (2,) -> (al_t, mu_t, al_s, mu_s) f64, each two products and
    one sum in that order."""
    am, mean = np.asarray(am, dtype=np.float64), np.asarray(mean, dtype=np.float64)
    tx, ty = np.float64(t[0]), np.float64(t[1])
    sx, sy = -ty, tx
    with np.errstate(all="ignore"):
        dax, day, dmx, dmy = am[:, 0] - mean[0], am[:, 1] - mean[1], am[:, 2] - mean[2], am[:, 3] - mean[3]
        return tx * dax + ty * day, tx * dmx + ty * dmy, sx * dax + sy * day, sx * dmx + sy * dmy


def cell_sums(wt, al, mu, zeta, freq):
    """One direction of one cell: wt (n,) longdouble, al, mu (n,) f64, zeta (Z,), freq (Q,) f64 -> (re, im (Z, Q) longdouble,
    allowance (Z, Q) f64): sum w cos 2 pi tau, -sum w sin 2 pi tau."""
    n = wt.shape[0]
    zeta, freq = np.asarray(zeta, dtype=np.float64), np.asarray(freq, dtype=np.float64)
    with np.errstate(all="ignore"):
        e = al.astype(LD)[:, None] + zeta.astype(LD)[None, :] * mu.astype(LD)[:, None]           # (n, Z)
        tau = freq.astype(LD)[None, None, :] * e[:, :, None]                                      # (n, Z, Q)
        tau = tau - np.rint(tau)
        tau = np.where(np.isfinite(tau), tau, 0)  # (a ray so far away that its phase is no number: its allowance is 2 w)
        re = (wt[:, None, None] * np.cos(2 * PI * tau)).sum(axis=0)
        im = -(wt[:, None, None] * np.sin(2 * PI * tau)).sum(axis=0)
        reach = np.abs(al)[:, None] + np.abs(zeta[None, :] * mu[:, None])                         # (n, Z) f64
        per_ray = 2 * np.pi * 3 * EPS * np.abs(freq)[None, None, :] * reach[:, :, None] + 4 * EPS
        per_ray = np.where(np.isfinite(per_ray), np.minimum(per_ray, 2.0), 2.0)
    w64 = wt.astype(np.float64)
    allow = (n + 40) * EPS * w64.sum() + (w64[:, None, None] * per_ray).sum(axis=0)
    return re, im, allow


def sums(p, w, fields, k, key, key_first, K, origin, means, t, zeta, freq):
    """fields: [(first, count), ...]; key[r - key_first]: the band of ray r; means (F, K, 4) f64: what the phases are taken about
    (`field_cases.record_means` of the records); t (F, 2); zeta (Z,); freq (Q,).  -> (val (F, K, Z, Q, 4) longdouble: re t, im t,
    re s, im s; allow (F, K, Z, Q, 2) f64: the allowance of the t and of the s sums; n (F, K): the rays in the sums)."""
    F, Z, Q = len(fields), len(zeta), len(freq)
    key = np.asarray(key)
    val, allow, n = np.zeros((F, K, Z, Q, 4), dtype=LD), np.zeros((F, K, Z, Q, 2)), np.zeros((F, K), dtype=np.int64)
    for f, (first, count) in enumerate(fields):
        if not count:
            continue
        _, inside, am = fc.lines(p, w, first, count, k, origin)
        kf = key[first - key_first:first - key_first + count]
        for b in range(K):
            m = inside & (kf == b)
            n[f, b] = np.count_nonzero(m)
            if not n[f, b]:
                continue
            wt = w[first:first + count, k][m].astype(LD)
            al_t, mu_t, al_s, mu_s = line_terms(am[m], means[f][b], t[f])
            val[f, b, :, :, 0], val[f, b, :, :, 1], allow[f, b, :, :, 0] = cell_sums(wt, al_t, mu_t, zeta, freq)
            val[f, b, :, :, 2], val[f, b, :, :, 3], allow[f, b, :, :, 1] = cell_sums(wt, al_s, mu_s, zeta, freq)
    return val, allow, n


def check_sums(got, val, allow, what=""):
    """Device sums (F, K, Z, Q, 4) against the truth of `sums`: every sum within its allowance.  -> largest share of one used."""
    got = np.asarray(got, dtype=np.float64).reshape(val.shape)
    err = np.abs(got.astype(LD) - val).astype(np.float64)
    bound = np.repeat(allow, 2, axis=-1)
    assert not np.any(np.isnan(got)), f"{what}: a sum is no number"
    over = err > bound
    assert not np.any(over), f"{what}: {np.count_nonzero(over)} sums off, first at {np.argwhere(over)[0]}: {err[over][0]} above {bound[over][0]}"
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.max(np.where(bound > 0, err / bound, 0.0), initial=0.0))
    print(f"{what}: sums use at most {worst:.3g} of their allowance")
    return worst


def direct_otf(x, wt, u, freq, centre=None):
    """sum w exp(-2 pi i nu u . (x - c)) / sum w over points x (n, 2) with weights wt, c their weighted mean unless given; all in
    longdouble.  -> (otf (Q,) complex as (re, im) longdouble arrays, c)."""
    x, wt = np.asarray(x).astype(LD), np.asarray(wt).astype(LD)
    W = wt.sum()
    c = (wt[:, None] * x).sum(axis=0) / W if centre is None else np.asarray(centre).astype(LD)
    d = (x - c) @ np.asarray(u).astype(LD)
    tau = np.asarray(freq).astype(LD)[None, :] * d[:, None]
    tau = tau - np.rint(tau)
    return (wt[:, None] * np.cos(2 * PI * tau)).sum(axis=0) / W, -(wt[:, None] * np.sin(2 * PI * tau)).sum(axis=0) / W, c
