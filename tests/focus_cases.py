"""Inputs and a host restatement for the focus-search kernels (csrc/ot_focus.hpp), shared by the fixture generator
tests/golden/generate_golden_focus_lines.py (run on the reference), tests/test_focus_host.py and
tests/test_gpu_focus_kernels.py.

`lines` draws "dyadic" hit lines ph(z) = pa + sb z: pa in multiples of 2^-12 inside [-1, 1), sb in multiples of 2^-8 inside
[-1/4, 1/4], to be evaluated at z in multiples of 2^-3 inside [0, 16], weights k / 1024 (k = 1..1024) as float32.  Then
  * x = pa + sb z is a multiple of 2^-12 below 5: exact in f64, with or without a fused multiply-add;
  * n_px / (x1 - x0) * (x - x0) rounds twice, the same way in the kernel and in NumPy: pixel indices are identical;
  * a pixel sum is a sum of multiples of 2^-10 below 2^43: exact in any order, the image is bit-equal.

`cost_terms` / `direct_solution` restate the reference's cost function and direct RMS solution with every sum in
np.longdouble and return, next to each sum, what the error bounds of the GPU tests need.
"""
from __future__ import annotations

import functools
import io
import zipfile

import numpy as np

LD = np.longdouble
U = 2.0 ** -53
METHODS = ("RMS Spot Size", "Irradiance Variance", "Image Sharpness", "Image Center Sharpness")
Z_SAMPLES = np.array([0.0, 3.125, 16.0])
BOUNDS = (0.0, 16.0)
ZERO_SHARE = 1 / 8   # rays with w = 0 (they stay in: pixel number and extent)
OUT_SHARE = 1 / 8    # rays left out, w = -1

# fixture cases: name -> arguments of `lines`
FIXTURE_CASES = {
    "n2": dict(n=2, seed=1, two=(512, 1024)),
    "n2_w0": dict(n=2, seed=2, two=(0, 768)),
    "n65": dict(n=65, seed=3),
    "n1025": dict(n=1025, seed=4),
    "n5000": dict(n=5000, seed=5),
    "fan1025": dict(n=1025, seed=6, fan=True),
}


def lines(n: int, seed: int, fan: bool = False, extremes_w0: bool = False, zero: float = ZERO_SHARE, out: float = OUT_SHARE,
          two: tuple | None = None, cross: float | None = None):
    """-> pa (n, 2) f64, sb (n, 2) f64, w (n,) f32 with w = -1 for the rays left out.
    fan: pa_y = sb_y = 0 (zero-height extent).  extremes_w0: four rays of weight 0 attain x-min, x-max, y-min, y-max at every
    z of [0, 16].  two: the weights k / 1024 of an n = 2 case (no shares).  cross: all lines meet in one point at this z."""
    rng = np.random.default_rng(seed)
    pa = rng.integers(-4096, 4096, (n, 2)) / 4096.0
    sb = rng.integers(-64, 65, (n, 2)) / 256.0
    w = (rng.integers(1, 1025, n) / 1024.0).astype(np.float32)
    if two is not None:
        assert n == 2
        w = (np.array(two) / 1024.0).astype(np.float32)
    else:
        kind = rng.random(n)
        w[kind < zero] = 0.0
        w[kind > 1.0 - out] = -1.0
    if cross is not None:
        point = np.array([0.25, -0.125])
        pa = point - sb * cross   # multiples of 2^-11: still exact
    if extremes_w0:
        assert n >= 8 and not fan
        j = [n // 5, 2 * n // 5, 3 * n // 5, 4 * n // 5]
        lo, hi = -1.0, 4095 / 4096.0
        pa[j[0]], sb[j[0]] = (lo, 0.0), (-0.25, 0.0)
        pa[j[1]], sb[j[1]] = (hi, 0.0), (0.25, 0.0)
        pa[j[2]], sb[j[2]] = (0.0, lo), (0.0, -0.25)
        pa[j[3]], sb[j[3]] = (0.0, hi), (0.0, 0.25)
        w[j] = 0.0
    if fan:
        pa[:, 1] = 0.0
        sb[:, 1] = 0.0
    return pa, sb, w


def kept(pa, sb, w):
    """The rays the reference's cost function is handed: those not left out."""
    m = w >= 0
    return pa[m], sb[m], w[m]


def n_px_for(n_kept: int) -> int:
    """Image side of the image methods: grows with sqrt(N), odd."""
    side = 100 * int(1 + np.sqrt(n_kept) / 1500)
    return side if side % 2 else side + 1


def hit_positions(pa, sb, z, fused=False):
    """x, y (f64) of the kept rays at z; fused: pa + sb z rounded once (as a fused multiply-add does)."""
    if not fused:
        return pa[:, 0] + sb[:, 0] * z, pa[:, 1] + sb[:, 1] * z
    # longdouble carries pa + sb z to 2^-63 relative; rounding that to f64 is the fused result unless it lies within that
    # distance of the middle between two f64 neighbours: those few are decided in exact rational arithmetic
    from fractions import Fraction
    ext = pa.astype(LD) + sb.astype(LD) * LD(z)
    ph = ext.astype(np.float64)
    half = np.spacing(np.abs(ph)).astype(LD) / 2
    near = np.abs(np.abs(ext - ph.astype(LD)) - half) <= np.abs(ext) * LD(2.0 ** -61)
    for i, c in zip(*np.nonzero(near)):
        exact = Fraction(float(pa[i, c])) + Fraction(float(sb[i, c])) * Fraction(float(z))
        ph[i, c] = float(exact)   # Fraction -> float rounds to nearest even
    return ph[:, 0], ph[:, 1]


def pixel_indices(x, y, n_px):
    """Flat pixel index per ray (-1: outside) and the extent, formed in f64 the way the reference forms them:
    floor(n_px / side * (x - x0)), the rays on the upper edge go to the last pixel, what is still outside is dropped."""
    ext = np.array([x.min(), x.max(), y.min(), y.max()])
    with np.errstate(all="ignore"):
        gx = np.floor(n_px / (ext[1] - ext[0]) * (x - ext[0]))
        gy = np.floor(n_px / (ext[3] - ext[2]) * (y - ext[2]))
    gy[y == ext[3]] = n_px - 1
    gx[x == ext[1]] = n_px - 1
    inside = (gx >= 0) & (gy >= 0) & (gx < n_px) & (gy < n_px)   # NaN compares false
    pix = np.full(x.shape[0], -1, dtype=np.int64)
    pix[inside] = gy[inside].astype(np.int64) * n_px + gx[inside].astype(np.int64)
    return pix, ext


@functools.lru_cache(maxsize=4)
def window(n_px):
    """Rotationally symmetric Hann window on the [-1, 1]^2 pixel grid, in f64 (read-only, shared)."""
    t = np.arange(n_px) * (2.0 / (n_px - 1)) + -1.0
    R = np.sqrt(t[None, :] ** 2 + t[:, None] ** 2)
    win = np.where(R > 1, 0.0, 1 + np.cos(R * np.pi))
    win.flags.writeable = False
    return win


def render(pix, w, n_px):
    """-> image (longdouble sums of the weights per pixel), rays per pixel."""
    img = np.zeros(n_px * n_px, dtype=LD)
    use = (pix >= 0) & (w > 0)
    np.add.at(img, pix[use], w[use].astype(LD))
    cnt = np.bincount(pix[use], minlength=n_px * n_px)
    return img.reshape(n_px, n_px), cnt.reshape(n_px, n_px)


def rms_terms(x, y, w):
    """RMS spot size sqrt(var_x + var_y) with the normalisation of a weighted covariance, W - sum w^2 / W.
    -> dict(cost, var, W, W2, Sx, Sy, Ax, Ay (sums of |w x|, |w y|), Vx, Vy, fact, n)."""
    wl, xl, yl = w.astype(LD), x.astype(LD), y.astype(LD)
    W, W2 = wl.sum(), (wl * wl).sum()
    Sx, Sy = (wl * xl).sum(), (wl * yl).sum()
    with np.errstate(all="ignore"):
        mx, my = Sx / W, Sy / W
        Vx, Vy = (wl * (xl - mx) ** 2).sum(), (wl * (yl - my) ** 2).sum()
        fact = W - W2 / W
        f = LD(1) / fact if fact > 0 else LD(np.inf)   # a weighted covariance without degrees of freedom divides by 0
        var = Vx * f + Vy * f
        cost = np.sqrt(var)
    return dict(cost=float(cost), var=var, W=W, W2=W2, Sx=Sx, Sy=Sy, Ax=np.abs(wl * xl).sum(), Ay=np.abs(wl * yl).sum(),
                Vx=Vx, Vy=Vy, fact=fact, mx=mx, my=my, n=int(w.shape[0]))


def image_terms(img, cnt, ext, n_px):
    """The three image costs of one image (longdouble) and the sums behind them.
    -> dict(irr=dict(cost, m, S, V, ...), sharp=dict(cost, T), center=dict(cost, s, g, T, win))."""
    out = {}
    with np.errstate(all="ignore"):
        # Irradiance Variance: -log(variance of the non-empty pixels / pixel area^2)
        lit = img > 0
        v = img[lit]
        m = int(v.size)
        S = v.sum()
        mean = S / LD(m) if m else LD(np.nan)
        V = ((v - mean) ** 2).sum()
        var = V / LD(m) if m else LD(np.nan)
        ap = (LD(ext[1]) - LD(ext[0])) * (LD(ext[3]) - LD(ext[2])) / LD(n_px) ** 2
        out["irr"] = dict(cost=float(-np.log(var / ap ** 2)), m=m, S=S, V=V, mean=mean, var=var, ap=ap, v=v, k=cnt[lit])
        # Image Sharpness: minus the sum of the squared forward differences in both directions
        T = 2 * n_px * (n_px - 1)
        g = ((img[1:] - img[:-1]) ** 2).sum() + ((img[:, 1:] - img[:, :-1]) ** 2).sum()
        out["sharp"] = dict(cost=float(-g), g=g, T=T)
        # Image Center Sharpness: the same of the windowed image, normalised to sum 1 where that sum is not 0
        win = window(n_px)
        im0 = img * win.astype(LD)
        s = im0.sum()
        g0 = ((im0[1:] - im0[:-1]) ** 2).sum() + ((im0[:, 1:] - im0[:, :-1]) ** 2).sum()
        out["center"] = dict(cost=float(-(g0 / (s * s)) if s != 0 else -g0), s=s, g=g0, T=T, win=win, im0=im0)
    return out


def cost_terms(pa, sb, w, z, n_px=None, xy=None):
    """All four costs at z of the lines pa, sb, w (rays with w < 0 are dropped first).
    -> dict(ext, n_px, pix, img (f64), img_ld, cnt, costs (4,), rms, irr, sharp, center)."""
    pa, sb, w = kept(pa, sb, w)
    n_px = n_px_for(w.shape[0]) if n_px is None else n_px
    x, y = hit_positions(pa, sb, z) if xy is None else xy
    pix, ext = pixel_indices(x, y, n_px)
    img, cnt = render(pix, w, n_px)
    out = dict(ext=ext, n_px=n_px, pix=pix, img=img.astype(np.float64), img_ld=img, cnt=cnt, rms=rms_terms(x, y, w))
    out.update(image_terms(img, cnt, ext, n_px))
    out["costs"] = np.array([out["rms"]["cost"], out["irr"]["cost"], out["sharp"]["cost"], out["center"]["cost"]])
    return out


def mean_line(pa, sb, w):
    """-> W, weighted means of pa_x, pa_y, sb_x, sb_y (longdouble), and sum |w pa_x| ... for the bounds."""
    wl = w.astype(LD)
    W = wl.sum()
    cols = [pa[:, 0], pa[:, 1], sb[:, 0], sb[:, 1]]
    sums = [(wl * c.astype(LD)).sum() for c in cols]
    mass = [np.abs(wl * c.astype(LD)).sum() for c in cols]
    return W, sums, mass


def moment_sums(pa, sb, w, b0, b1, means=None):
    """The fourteen sums of ot_focus_moments in longdouble, with sum |terms| beside each: -> (sums[14], mass[14], parts).
    means: (mpx, mpy, msx, msy) to centre on (f64 values of the device); default: the exact weighted means.
    parts: the per-sum first derivatives needed to propagate an error of the centring constants
    (dS5_dv, dS6_dv, dS6_dp, dS8_dm, dS9_dm per axis)."""
    pa, sb, w = kept(pa, sb, w)
    wl = w.astype(LD)
    pax, pay, sbx, sby = (c.astype(LD) for c in (pa[:, 0], pa[:, 1], sb[:, 0], sb[:, 1]))
    W, s14, m14 = mean_line(pa, sb, w)
    S, M = np.zeros(14, dtype=LD), np.zeros(14, dtype=LD)
    S[0], M[0] = W, W
    S[1:5], M[1:5] = s14, m14
    w2 = wl * wl
    S[7] = M[7] = w2.sum()
    mpx, mpy, msx, msy = [LD(v) for v in means] if means is not None else [v / W for v in s14]
    b0, b1 = LD(b0), LD(b1)
    pb0x, pb0y = mpx + msx * b0, mpy + msy * b0
    vxz, vyz = msx, msy   # ((mp + ms b1) - (mp + ms b0)) / (b1 - b0)
    z0 = (b0 + b1) / 2
    dx, dy, dtx, dty = pax - pb0x, pay - pb0y, sbx - vxz, sby - vyz
    t5 = w2 * dtx * dtx + w2 * dty * dty
    t6x, t6y = dtx * dx * w2, dty * dy * w2
    S[5], M[5] = t5.sum(), t5.sum()
    S[6], M[6] = (t6x + t6y).sum(), (np.abs(t6x) + np.abs(t6y)).sum()
    x0, y0 = (pax + sbx * z0) - (mpx + msx * z0), (pay + sby * z0) - (mpy + msy * z0)
    sx, sy = sbx - msx, sby - msy
    for k, t in zip((8, 9, 10, 11, 12, 13), (wl * x0 * x0, wl * x0 * sx, wl * sx * sx, wl * y0 * y0, wl * y0 * sy, wl * sy * sy)):
        S[k], M[k] = t.sum(), np.abs(t).sum()
    parts = dict(dS5_dv=2 * ((w2 * np.abs(dtx)).sum() + (w2 * np.abs(dty)).sum()),
                 dS6_dv=(w2 * np.abs(dx)).sum() + (w2 * np.abs(dy)).sum(),
                 dS6_dp=(w2 * np.abs(dtx)).sum() + (w2 * np.abs(dty)).sum(),
                 dS8_dm=2 * (wl * np.abs(x0)).sum(), dS11_dm=2 * (wl * np.abs(y0)).sum(),
                 dS9_dm=(wl * np.abs(sx)).sum(), dS12_dm=(wl * np.abs(sy)).sum(), W=W, W2=w2.sum(), n=int(w.shape[0]))
    return S, M, parts


def direct_solution(pa, sb, w, bounds):
    """Direct RMS solution: the z that minimises the w^2-weighted spread of the lines about the mean line through the
    bounds, clipped to the bounds; fun = RMS cost there.  -> dict(x, fun, S5, S6, unclipped)."""
    pk, sk, wk = kept(pa, sb, w)
    S, M, parts = moment_sums(pa, sb, w, bounds[0], bounds[1])
    d = -S[6] / S[5] if S[5] != 0 else LD(0.5) * (LD(bounds[0]) + LD(bounds[1]))
    x = float(min(max(d, LD(bounds[0])), LD(bounds[1])))
    fun = rms_terms(*hit_positions(pk, sk, x), wk)["cost"]
    return dict(x=x, fun=fun, S=S, M=M, parts=parts, unclipped=d)


def variance_at(pa, sb, w, z):
    """var_x + var_y of the hits at z with the weighted-covariance normalisation, longdouble."""
    pk, sk, wk = kept(pa, sb, w)
    xl = pk.astype(LD) + sk.astype(LD) * LD(z)
    return rms_terms(xl[:, 0], xl[:, 1], wk)["var"]


def same_kind(a: float, b: float) -> bool:
    """Non-finite values agree in kind and sign (and zeros in sign)."""
    if np.isnan(a) or np.isnan(b):
        return bool(np.isnan(a) and np.isnan(b))
    if np.isinf(a) or np.isinf(b) or a == 0 or b == 0:
        return bool(a == b and np.signbit(a) == np.signbit(b))
    return True


def write_npz(path, arrays: dict) -> None:
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())
