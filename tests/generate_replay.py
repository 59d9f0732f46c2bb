"""Host replay of the ray generator (optrace_amd/csrc/ot_generate.hpp), NumPy only.

Ray j of a range of n rays is a pure function of (seed, global index, range id, j, n, source record), so the whole stage
can be replayed without a device:

integer layer   bit-exact by construction (uint32 / uint64): Philox-4x32, the stream keys, the keyed permutations, the
                slicing of the Philox blocks into dither fields, the per-range constants, the range ids.
uniform layer   `k + bits * 2^-32` (2^-16 for image sources) is exact in the 64 mantissa bits of a longdouble, which is the
                single rounding of the device's fused form; the stratified samplers on top of it in longdouble.
formula layer   RaySource.create_rays (ray_source.py:204-437) and the helpers of random.py restated from their
                DEFINITIONS in longdouble: arcsin / arccos and sin / cos where the kernel forms (sin, cos) pairs
                algebraically, searchsorted where it walks from a guide bucket, divmod where it multiplies by a reciprocal
                and fixes up.  None of the device's guide / bucket tables exists here: they are hints.

`replay` returns, next to the rays, `near`: the number of rays whose replayed uniform variable lies so close to a table
node, a cell edge or a branch point that the discrete decision behind it could legitimately differ after rounding
(NEAR * eps, relative to the table's total).  The tests demand near == 0 before they consult the device.
"""
import numpy as np

LD = np.longdouble
EPS = 2.0 ** -52
NEAR = 8  # a discrete decision is left open within NEAR * eps of a node / edge / branch point
LD_PI = 4 * np.arctan(LD(1))
M32 = np.uint64(0xffffffff)

# enums of include/optrace_amd.h (test_generate_replay_host.py holds them against optrace_amd._capi)
SRC_POINT, SRC_LINE, SRC_CIRCLE, SRC_RING, SRC_RECT, SRC_IMAGE_RGB, SRC_IMAGE_GRAY = range(7)
DIV_NONE, DIV_LAMBERTIAN, DIV_ISOTROPIC, DIV_TABLE = range(4)
OR_CONSTANT, OR_CONVERGING, OR_ARRAY = range(3)
POL_CONSTANT, POL_UNIFORM, POL_LIST, POL_TABLE = range(4)
SPEC_MONO, SPEC_UNIFORM, SPEC_LINES, SPEC_GAUSSIAN, SPEC_TABLE = range(5)
(ST_POS, ST_PIX_JITTER, ST_DIV, ST_DIV_ALPHA, ST_WL, ST_POL, ST_RGB_CHOICE, ST_RGB_WL, ST_PIXEL) = range(1, 10)
PRIM_N, PRIM_M = 5000, 65536  # wavelengths(5000) of srgb.py:528; buckets of the device's inverse table
FR, FB = 0.885651229244, 0.775993481741  # srgb.py:24-26


# ---- integer layer ---------------------------------------------------------------------------------------------------
def _u64(x):
    return np.asarray(x).astype(np.uint64)


def philox4x32(counter, key, rounds=10):
    """Philox-4x32 (Salmon et al., SC'11).  counter (..., 4), key (..., 2), any integer arrays -> (..., 4) uint32."""
    c = [_u64(np.asarray(counter)[..., k]) & M32 for k in range(4)]
    k0, k1 = (_u64(np.asarray(key)[..., k]) & M32 for k in range(2))
    m0, m1, w0, w1 = (np.uint64(v) for v in (0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85))
    for _ in range(rounds):
        p0, p1 = m0 * c[0], m1 * c[2]  # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & M32, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & M32]
        k0, k1 = (k0 + w0) & M32, (k1 + w1) & M32
    return np.stack(np.broadcast_arrays(*c), axis=-1).astype(np.uint32)


def stream_key(seed, rng, stream):
    m = 0xffffffff
    h = (seed & m) ^ (((seed >> 32) * 0x9E3779B1) & m) ^ ((rng * 0x85EBCA77) & m) ^ ((stream * 0xC2B2AE3D) & m)
    h ^= h >> 16
    h = (h * 0x7feb352d) & m
    h ^= h >> 15
    h = (h * 0x846ca68b) & m
    h ^= h >> 16
    return h


def _mul(i, c):
    return (i * np.uint64(c)) & M32


def permute_hash(i, w, key):
    """Kensler's hash on [0, w], w = 2^k - 1 (Pixar TM 13-01)."""
    i, w = _u64(i), np.uint64(w)
    sh = lambda v, s: v >> np.uint64(s)
    i = i ^ np.uint64(key)
    i = _mul(i, 0xe170893d)
    i = i ^ np.uint64(key >> 16)
    i = i ^ sh(i & w, 4)
    i = i ^ np.uint64(key >> 8)
    i = _mul(i, 0x0929eb3f)
    i = i ^ np.uint64(key >> 23)
    i = i ^ sh(i & w, 1)
    i = _mul(i, 1 | (key >> 27))
    i = _mul(i, 0x6935fa69)
    i = i ^ sh(i & w, 11)
    i = _mul(i, 0x74dcb303)
    i = i ^ sh(i & w, 2)
    i = _mul(i, 0x9e501cc3)
    i = i ^ sh(i & w, 2)
    i = _mul(i, 0xc860a3df)
    i = i & w
    return i ^ sh(i, 5)


def permute_pow2_large(i, w, key):
    i, k = _u64(i), int(w).bit_length()
    sa, sb, wu = np.uint64((k + 1) >> 1), np.uint64((k + 2) // 3), np.uint64(w)
    m2 = ((0x0929eb3f ^ ((key >> 7) << 1)) | 1) & 0xffffffff
    i = i ^ np.uint64(key & w)
    i = _mul(i, 0xe170893d) & wu
    i = i ^ (i >> sa)
    i = _mul(i, m2) & wu
    i = i ^ (i >> sb)
    i = i ^ np.uint64((key >> 13) & w)
    i = _mul(i, 0x6935fa69) & wu
    i = i ^ (i >> sa)
    return (i + np.uint64((key >> 3) & w)) & wu


def permute_index(i, l, key):
    """Keyed bijection of [0, l): the stratum of sample i."""
    i = _u64(i)
    if l <= 1:
        return np.zeros_like(i)
    w = l - 1
    if l & w == 0:
        if l >= 1 << 20:
            return permute_pow2_large(i, w, key)
        return (permute_hash(i, w, key) + np.uint64(key & w)) & np.uint64(w)
    w = (1 << w.bit_length()) - 1
    i = permute_hash(i, w, key)
    out = i >= np.uint64(l)
    while out.any():  # cycle walking, only the lanes still outside
        i[out] = permute_hash(i[out], w, key)
        out = i >= np.uint64(l)
    rot = key & w
    return (i + np.uint64(rot - l if rot >= l else rot)) % np.uint64(l)


def range_constants(n):
    """(n2, inv_n, inv_n2): floor(sqrt(n)) and the float64 reciprocals the host hands to the kernels."""
    import math
    n2 = math.isqrt(int(n))
    return n2, (1.0 / n if n else 0.0), (1.0 / n2 if n2 else 0.0)


def range_ids(ranges):
    """ranges: [(source, first, count, ...)] in call order -> the same records in the order that numbers them on the device
    (stable sort by (first, count): an empty range comes before the non-empty one that shares its start)."""
    return sorted(ranges, key=lambda r: (r[1], r[2]))  # sorted() is stable


def dither_slot(stream):
    return {ST_DIV: 0, ST_WL: 2, ST_RGB_WL: 2, ST_POL: 3, ST_POS: 4, ST_DIV_ALPHA: 6, ST_PIXEL: 8, ST_PIX_JITTER: 9}.get(stream, 11)


def dither_field(slot, image):
    """(block, word, shift, bits) of dither slot `slot`: block 0 = A, 1 = B.  Image sources cut block A into eight 16-bit
    halves for the slots 0-3 and 8-11; the slots 4-7 are always the 32-bit words of block B."""
    if 4 <= slot < 8:
        return 1, slot - 4, 0, 32
    if image:
        j = slot if slot < 4 else slot - 4
        return 0, j >> 1, 16 * (j & 1), 16
    if slot >= 8:
        raise ValueError("the slots 8-11 exist for image sources only")
    return 0, slot, 0, 32


def needs_block_b(shape, divergence, div_2d):
    image = shape >= SRC_IMAGE_RGB
    return (shape != SRC_POINT and not image) or (divergence != DIV_NONE and bool(div_2d))


def streams_read(shape, divergence, div_2d, rgb_spectrum_free=True):
    """[(stream, number of consecutive slots)] that create_rays' device version draws for a source of this kind (every
    optional stream included: a polychromatic spectrum, a sampled polarisation)."""
    image = shape >= SRC_IMAGE_RGB
    out = [(ST_POL, 1)]
    if shape != SRC_IMAGE_RGB:
        out.append((ST_WL, 1))
    if image:
        out += [(ST_PIXEL, 1), (ST_PIX_JITTER, 2)] + ([(ST_RGB_CHOICE, 1)] if shape == SRC_IMAGE_RGB else [])
    elif shape != SRC_POINT:
        out.append((ST_POS, 1 if shape == SRC_LINE else 2))
    if divergence != DIV_NONE:
        out += [(ST_DIV, 1), (ST_DIV_ALPHA, 1)] if div_2d else [(ST_DIV, 2)]
    return out


class Ctx:
    """One range: seed, range id, the indices j of its n rays, their global indices, the Philox blocks."""

    def __init__(self, seed, rid, first, n, need_b, image, identity=False):
        self.seed, self.rid, self.n, self.image = int(seed), int(rid), int(n), bool(image)
        self.j = np.arange(n, dtype=np.uint64)
        g = self.j + np.uint64(first)
        cnt = lambda c2, c3: np.stack([g & M32, g >> np.uint64(32), np.full_like(g, c2), np.full_like(g, c3)], axis=-1)
        key = (self.seed & 0xffffffff, self.seed >> 32)
        self.blocks = [philox4x32(cnt(0x67656e31, 0), key, 7), philox4x32(cnt(0x67656e32, 1), key, 7) if need_b else None]
        self.n2 = range_constants(n)[0]
        self.near = 0
        self.identity = identity  # shuffle=False of ot.random: stratum j for sample j

    def stratum(self, stream):
        if self.identity:
            return self.j.copy()
        return permute_index(self.j, self.n, stream_key(self.seed, self.rid, stream))

    def bits(self, slot):
        block, word, shift, nb = dither_field(slot, self.image)
        if self.blocks[block] is None:
            raise RuntimeError(f"slot {slot} reads block B, which this source does not draw")
        return (self.blocks[block][:, word].astype(np.uint64) >> np.uint64(shift)) & np.uint64((1 << nb) - 1), nb

    def plus(self, slot, k):
        """k + u, u = bits * 2^-nb in [0, 1): exact in a longdouble"""
        b, nb = self.bits(slot)
        return k.astype(LD) + b.astype(LD) * LD(2.0 ** -nb)

    def centred(self, slot):
        """(bits + 0.5) * 2^-nb: the dither where no stratum index is added"""
        b, nb = self.bits(slot)
        return (b.astype(LD) + LD(0.5)) * LD(2.0 ** -nb)

    def mark(self, mask):
        self.near += int(np.count_nonzero(mask))


# ---- uniform layer (random.py) -----------------------------------------------------------------------------------------
def strat_interval(c, stream, a, b, k=None):
    """random.stratified_interval_sampling random.py:48-67: a + (k + u) * (b - a) / N"""
    k = c.stratum(stream) if k is None else k
    return LD(a) + c.plus(dither_slot(stream), k) * ((LD(b) - LD(a)) / c.n)


def strat_rect(c, stream, a, b, cc, d):
    """random.stratified_rectangle_sampling random.py:8-45 -> x, y, (ix, iy, nx, ny) (cell -1: one of the n - N2^2 uniform samples).
    A power-of-two count of at least 4 fills a 2^ceil(m/2) x 2^floor(m/2) grid instead."""
    k, slot, n = c.stratum(stream), dither_slot(stream), c.n
    a, b, cc, d = LD(a), LD(b), LD(cc), LD(d)
    if n & (n - 1) == 0 and n >= 4:
        m = n.bit_length() - 1
        nx, ny = 1 << ((m + 1) >> 1), 1 << (m >> 1)
        iy, ix = np.divmod(k, np.uint64(nx))
        ux, uy = c.plus(slot, ix), c.plus(slot + 1, iy)
        for u, i in ((ux, ix), (uy, iy)):  # a sample on its cell's edge
            c.mark(u - i.astype(LD) < NEAR * EPS)
        return a + ux * ((b - a) / nx), cc + uy * ((d - cc) / ny), (ix.astype(np.int64), iy.astype(np.int64), nx, ny)
    u0, u1, n2 = c.centred(slot), c.centred(slot + 1), c.n2
    grid = k < np.uint64(n2 * n2)
    iy, ix = np.divmod(k, np.uint64(n2))
    x = np.where(grid, a + (ix.astype(LD) + u0) * ((b - a) / n2), a + u0 * (b - a))
    y = np.where(grid, cc + (iy.astype(LD) + u1) * ((d - cc) / n2), cc + u1 * (d - cc))
    return x, y, (np.where(grid, ix.astype(np.int64), -1), np.where(grid, iy.astype(np.int64), -1), n2, n2)


def strat_ring(c, stream, ri, r, polar):
    """random.stratified_ring_sampling random.py:70-110 -> (x, y) or (|r|, theta)"""
    x, y, _ = strat_rect(c, stream, -r, r, -r, r)
    x2, y2 = x * x, y * y
    c.mark(np.abs(np.abs(x) - np.abs(y)) < NEAR * EPS * r)  # which branch of Shirley's map
    m = x2 > y2
    safe = lambda v: np.where(v == 0, LD(1), v)
    r_ = np.where(m, x, np.where(y2 > 0, y, LD(0)))
    theta = np.where(m, LD_PI / 4 * y / safe(x), np.where(y2 > 0, LD_PI / 2 - LD_PI / 4 * x / safe(y), LD(0)))
    if ri:
        r_ = np.where(r_ < 0, LD(-1), LD(1)) * np.sqrt(LD(ri) ** 2 + r_ ** 2 * (1 - (LD(ri) / LD(r)) ** 2))
    if not polar:
        return r_ * np.cos(theta), r_ * np.sin(theta)
    return np.abs(r_), np.where(r_ < 0, theta - LD_PI, theta)


def inverse_discrete(c, values, F, X):
    """random.inverse_transform_sampling kind="discrete" (interp1d kind="next"): the first entry whose cumulative weight
    reaches X -> (value, index)"""
    F = np.asarray(F, dtype=np.float64)
    near_nodes(c, F, X)
    idx = np.minimum(np.searchsorted(F, X.astype(np.float64), side="left"), len(F) - 1)
    # (searchsorted in float64 can only err for X within an ulp of a node, and those are marked `near`)
    return np.asarray(values)[idx], idx


def inverse_linear(c, x, F, X):
    """kind="continuous": linear interpolation of the inverse of the cumulative trapezoid F over x -> (value, bound on what
    NEAR / 2 eps * F[-1] of error in X move the value by)"""
    x, F = np.asarray(x, dtype=np.float64), np.asarray(F, dtype=np.float64)
    near_nodes(c, F, X)
    lo = np.clip(np.searchsorted(F, X.astype(np.float64), side="right") - 1, 0, len(F) - 2)
    F0, F1, x0, x1 = F[lo].astype(LD), F[lo + 1].astype(LD), x[lo].astype(LD), x[lo + 1].astype(LD)
    dF = F1 - F0
    ok = dF > 0
    val = np.where(ok, x0 + (X - F0) / np.where(ok, dF, 1) * (x1 - x0), x0)
    slope = np.where(ok, np.abs(x1 - x0) / np.where(ok, dF, 1), 0) * np.abs(LD(F[-1]))
    return val, (slope * EPS).astype(np.float64)


def near_nodes(c, F, X):
    Xd = X.astype(np.float64)
    i = np.clip(np.searchsorted(F, Xd), 1, len(F) - 1) if len(F) > 1 else np.zeros(len(Xd), dtype=int)
    dist = np.minimum(np.abs(X - F[i].astype(LD)), np.abs(X - F[i - 1].astype(LD))) if len(F) > 1 else np.abs(X - LD(F[0]))
    c.mark(dist < NEAR * EPS * abs(F[-1]))


# ---- formula layer -------------------------------------------------------------------------------------------------------
def erf_ld(x):
    """erf in longdouble: 2 / sqrt(pi) * exp(-x^2) * sum_n 2^n x^(2n+1) / (2n+1)!! (all terms of one sign: no cancellation)"""
    x = np.asarray(x, dtype=LD)
    term, total = x.copy(), x.copy()
    for n in range(1, 400):
        term = term * (2 * x * x / (2 * n + 1))
        total = total + term
    return 2 / np.sqrt(LD_PI) * np.exp(-x * x) * total


def erfinv_ld(t):
    """erfinv by Newton's iteration on erf_ld, from Winitzki's closed form"""
    t = np.asarray(t, dtype=LD)
    a, lg = LD(0.147), np.log(1 - t * t)
    h = 2 / (LD_PI * a) + lg / 2
    y = np.sign(t) * np.sqrt(np.sqrt(h * h - lg / a) - h)
    for _ in range(6):
        y = y - (erf_ld(y) - t) / (2 / np.sqrt(LD_PI) * np.exp(-y * y))
    return y


def srgb_to_linear(v):  # srgb.py:30-47
    v = np.asarray(v, dtype=np.float64)
    a = 0.055
    return np.where(np.abs(v) <= 0.04045, 1 / 12.92 * v, np.sign(v) * (1 / (1 + a) * (np.abs(v) + a)) ** 2.4)


def primary_inverse(primaries, wl_grid):
    """-> x_def(prim, t): the inverse of the cumulative trapezoid of primary `prim` over `wl_grid` at t in [0, 1] (srgb.py:549-551
    with random.py:150-157)"""
    tabs = []
    for f in primaries:
        v = np.asarray(f(wl_grid), dtype=np.float64)
        tabs.append(np.concatenate(([0.], np.cumsum((v[1:] + v[:-1]) / 2))))

    def x_def(prim, t):
        out = np.zeros(t.shape, dtype=LD)
        for q in range(3):
            sel = prim == q
            if sel.any():
                F = tabs[q]
                X = F[0] + t[sel] * (LD(F[-1]) - F[0])
                lo = np.clip(np.searchsorted(F, X.astype(np.float64), side="right") - 1, 0, len(F) - 2)
                dF = (F[lo + 1] - F[lo]).astype(LD)
                out[sel] = np.where(dF > 0, wl_grid[lo] + (X - F[lo]) / np.where(dF > 0, dF, 1) * (wl_grid[lo + 1] - wl_grid[lo]),
                                    wl_grid[lo])
        return out
    return x_def


def _wavelength(c, f):
    """LightSpectrum.random_wavelengths light_spectrum.py:81-138 -> (wl, float64 bound on the chain behind the uniform variable)"""
    kind, n = f["spectrum"], c.n
    if kind == SPEC_MONO:
        return np.full(n, LD(np.float32(f["wl"]))), np.zeros(n)
    if kind == SPEC_UNIFORM:
        wl = strat_interval(c, ST_WL, f["wl0"], f["wl1"])
        return wl, 4 * EPS * np.abs(wl).astype(np.float64)  # 1 / n, (b - a) / n, the product, the sum
    if kind == SPEC_LINES:
        tab, m = np.asarray(f["spec_tab"]), int(f["n_spec"])
        wl, _ = inverse_discrete(c, tab[:m], tab[m:], strat_interval(c, ST_WL, 0.0, tab[-1]))
        return wl.astype(LD), np.zeros(n)
    if kind == SPEC_GAUSSIAN:
        mu, sig, s2 = LD(f["mu"]), LD(f["sig"]), np.sqrt(LD(2))
        xl, xr = ((1 + erf_ld((LD(b) - mu) / (s2 * sig))) / 2 for b in (f["wl0"], f["wl1"]))
        X = strat_interval(c, ST_WL, xl, xr)
        y = erfinv_ld(2 * X - 1)
        # d wl / d X = sqrt(2) sig * sqrt(pi) exp(y^2): X carries 6 roundings (erf of the bounds, the four of the interval
        # sampler, 2 X - 1), then mu + c * erfinv: 3 more on the scale of wl
        cond = s2 * sig * np.sqrt(LD_PI) * np.exp(y * y)
        return mu + s2 * sig * y, (6 * EPS * cond + 3 * EPS * 780.).astype(np.float64)
    tab, m = np.asarray(f["spec_tab"]), int(f["n_spec"])
    wl, b = inverse_linear(c, tab[:m], tab[m:], strat_interval(c, ST_WL, tab[m], tab[-1]))
    return wl, 6 * b + 4 * EPS * 780.  # X: 4 roundings, X - F0 and the quotient: 2; the interpolation: 4 on the scale of wl


def replay_source(c, f, no_pol, s_or=None, x_def=None):
    """The n rays of range `c` of the source with `_source_fields()` f (plus "power" where no ray power is given).
    -> dict of longdouble arrays p, s, pol (n, 3), wl (n,), float64 bounds wl_bound / s_extra / pol_cond, and facts."""
    n, shape, out = c.n, f["shape"], {}
    image = shape >= SRC_IMAGE_RGB
    pos = [LD(v) for v in f["pos"]]
    p = np.empty((n, 3), dtype=LD)
    p[:] = pos

    # ---- wavelength ----
    if shape != SRC_IMAGE_RGB:
        out["wl"], out["wl_bound"] = _wavelength(c, f)

    # ---- start position (ray_source.py:229-255, Surface.random_positions) ----
    if shape == SRC_LINE:
        t = strat_interval(c, ST_POS, -f["r"], f["r"])
        ang = LD(f.get("angle", 0.0))
        p[:, 0] += np.cos(ang) * t
        p[:, 1] += np.sin(ang) * t
        out["stratum"] = c.stratum(ST_POS).astype(np.int64)
    elif shape in (SRC_CIRCLE, SRC_RING):
        x, y = strat_ring(c, ST_POS, f["ri"] if shape == SRC_RING else 0.0, f["r"], False)
        p[:, 0] += x
        p[:, 1] += y
    elif shape == SRC_RECT:
        d0, d1, ang = LD(f["dim"][0]), LD(f["dim"][1]), LD(f.get("angle", 0.0))
        x, y, out["cell"] = strat_rect(c, ST_POS, -d0 / 2, d0 / 2, -d1 / 2, d1 / 2)
        out["rect_xy"] = (x, y)
        p[:, 0] += x * np.cos(ang) - y * np.sin(ang)
        p[:, 1] += x * np.sin(ang) + y * np.cos(ang)
    elif image:
        W, H = int(f["img_w"]), int(f["img_h"])
        pdf = np.asarray(f["img_pdf"], dtype=np.float64)
        k_pixel = c.stratum(ST_PIXEL)
        if W * H > 1:  # ray_source.py:239-245
            F = np.cumsum(pdf)
            _, P = inverse_discrete(c, np.arange(W * H), F, strat_interval(c, ST_PIXEL, 0.0, F[-1], k=k_pixel))
        else:
            P = np.zeros(n, dtype=np.int64)
        PY, PX = np.divmod(P, W)
        rx, ry = c.centred(dither_slot(ST_PIX_JITTER)), c.centred(dither_slot(ST_PIX_JITTER) + 1)
        d0, d1 = LD(f["dim"][0]), LD(f["dim"][1])
        p[:, 0] = d0 / W * (PX + rx) + (pos[0] - d0 / 2)
        p[:, 1] = d1 / H * (PY + ry) + (pos[1] - d1 / 2)
        out["pixel"] = P
        if shape == SRC_IMAGE_RGB:  # color.random_wavelengths_from_srgb srgb.py:513-553
            if n & (n - 1) == 0 and n >= 2:  # the choice variable's stratum: a rank-1 lattice on the pixel stratum
                m = n.bit_length() - 1
                mult = (0x9E3779B1 >> (32 - m)) | 1
                kc = (k_pixel * np.uint64(mult) + np.uint64(stream_key(c.seed, c.rid, ST_RGB_CHOICE))) & np.uint64(n - 1)
            else:
                kc = c.stratum(ST_RGB_CHOICE)
            choice = strat_interval(c, ST_RGB_CHOICE, 0.0, 1.0, k=kc)
            rgbl = srgb_to_linear(np.asarray(f["img_rgb"]).reshape(-1, 3)[P]) * [FR, 1.0, FB]
            cs = np.cumsum(rgbl, axis=1)
            cs = cs / np.where(cs[:, 2:3], cs[:, 2:3], 1)
            c_r, c_rg = cs[:, 0], cs[:, 1]
            # the float64 c_r, c_rg come out of pow(): a few ulps either way
            c.mark((np.abs(choice - c_r) < NEAR * EPS) | (np.abs(choice - c_rg) < NEAR * EPS))
            prim = np.where(choice < c_r, 0, np.where(choice > c_rg, 2, 1))
            lo = np.where(prim == 0, 0.0, np.where(prim == 1, c_r, c_rg)).astype(LD)
            hi = np.where(prim == 0, c_r, np.where(prim == 1, c_rg, 1.0)).astype(LD)
            t = np.where(hi > lo, (choice - lo) / np.where(hi > lo, hi - lo, 1), LD(0.5))
            m = np.clip(np.floor(t * PRIM_M), 0, PRIM_M - 1)
            out["wl"] = x_def(prim, t)
            out["wl_bucket"] = (x_def(prim, m / PRIM_M), x_def(prim, (m + 1) / PRIM_M))
            out["primary"], out["wl_bound"] = prim, np.zeros(n)

    # ---- orientation (ray_source.py:264-277) ----
    if f["orientation"] == OR_CONVERGING:
        d = np.array([LD(v) for v in f["conv_pos"]]) - p
        so = d / np.sqrt((d * d).sum(axis=1))[:, None]
    elif f["orientation"] == OR_ARRAY and s_or is not None:
        so = np.asarray(s_or, dtype=LD)
    else:
        so = np.broadcast_to(np.array([LD(v) for v in f["s"]]), (n, 3))

    # ---- divergence (ray_source.py:290-351) ----
    s, s_extra = so, np.zeros(n)
    if f["divergence"] != DIV_NONE:
        div_rad = LD(np.radians(f["div_angle"]))
        div_sin = np.sin(div_rad)
        if f["div_2d"]:
            X = strat_interval(c, ST_DIV_ALPHA, 0.0, 2.0)  # inverse transform of two equal weights, F = [1, 2]
            c.mark(np.abs(X - 1) < NEAR * EPS * 2)
            alpha = LD(np.radians(f["div_axis_angle"])) + np.where(X <= 1, LD(0), LD_PI)
            out["branch"] = (X <= 1)
            if f["divergence"] == DIV_LAMBERTIAN:
                theta = np.arcsin(strat_interval(c, ST_DIV, 0.0, div_sin))
            elif f["divergence"] == DIV_ISOTROPIC:
                theta = strat_interval(c, ST_DIV, 0.0, div_rad)
            else:
                tab, m = np.asarray(f["div_tab"]), int(f["n_div"])
                theta, b = inverse_linear(c, tab[:m], tab[m:], strat_interval(c, ST_DIV, tab[m], tab[-1]))
                s_extra = 6 * b
        else:
            r, alpha = strat_ring(c, ST_DIV, 0.0, div_sin, True)
            if f["divergence"] == DIV_LAMBERTIAN:
                theta = np.arcsin(r)
            elif f["divergence"] == DIV_ISOTROPIC:
                theta = np.arccos(1 - r ** 2)
            else:
                tab, m = np.asarray(f["div_tab"]), int(f["n_div"])
                X0 = r ** 2 / div_sin ** 2
                theta, b = inverse_linear(c, tab[:m], tab[m:], tab[m] + X0 * (LD(tab[-1]) - tab[m]))
                s_extra = 12 * b  # r^2 / div_sin^2 and the rescaling: X carries about twice the roundings of a sampler's
        fa = 1 / np.sqrt(1 - so[:, 0] ** 2)
        sy = np.stack([np.zeros(n, dtype=LD), -so[:, 2] * fa, so[:, 1] * fa], axis=1)
        sx = np.cross(so, sy)
        th, al = theta[:, None], alpha[:, None]
        s = np.cos(th) * so + np.sin(th) * (np.cos(al) * sx + np.sin(al) * sy)

    # ---- polarisation (ray_source.py:359-433) ----
    pol = np.zeros((n, 3), dtype=LD)
    out["pol_cond"] = np.zeros(n)
    if not no_pol:
        kind = f["polarization"]
        if kind == POL_CONSTANT:
            ang = np.full(n, LD(f["pol_angle"]))
        elif kind == POL_UNIFORM:
            ang = strat_interval(c, ST_POL, 0.0, 2.0) * LD_PI
        elif kind == POL_LIST:
            tab, m = np.asarray(f["pol_tab"]), int(f["n_pol"])
            ang, out["pol_index"] = inverse_discrete(c, tab[:m], tab[m:], strat_interval(c, ST_POL, 0.0, tab[-1]))
            ang = ang.astype(LD)
        else:
            tab, m = np.asarray(f["pol_tab"]), int(f["n_pol"])
            ang, b = inverse_linear(c, tab[:m], tab[m:], strat_interval(c, ST_POL, tab[m], tab[-1]))
            out["pol_cond"] = out["pol_cond"] + 6 * b
        pol[:, 0], pol[:, 1] = np.cos(ang), np.sin(ang)
        mask = s[:, 2] != 1
        q2 = 1 - s[:, 2] ** 2
        fa = 1 / (np.sqrt(np.where(mask, q2, 1)) + LD(1e-16))
        ps = np.stack([s[:, 1] * fa, -s[:, 0] * fa, np.zeros(n, dtype=LD)], axis=1)
        A_ts = ps[:, 0] * pol[:, 0] + ps[:, 1] * pol[:, 1]
        A_tp = ps[:, 1] * pol[:, 0] - ps[:, 0] * pol[:, 1]
        pp = np.cross(ps, s)
        pol = np.where(mask[:, None], ps * A_ts[:, None] + pp * A_tp[:, None], pol)
        out["pol_q2"] = np.where(mask, q2, 1).astype(np.float64)
    out.update(p=p, s=s, pol=pol, s_extra=np.asarray(s_extra, dtype=np.float64) * np.ones(n))
    return out


def replay(sources, ranges, seed, no_pol, s_or=None, x_def=None):
    """sources: list of `_source_fields()` dicts with "power"; ranges: [(source, first, count, ray_power)] in call order;
    s_or: {source index: (count, 3) base orientations} for OR_ARRAY sources.
    -> dict of arrays over all rays (index = global ray index): p, s, pol, wl longdouble, w float32, bounds, `near`,
    `rid` (range id of every ray), `facts`: [(first, count, per-range dict)]."""
    N = max((r[1] + r[2] for r in ranges), default=0)
    res = dict(p=np.zeros((N, 3), LD), s=np.zeros((N, 3), LD), pol=np.zeros((N, 3), LD), wl=np.zeros(N, LD),
               w=np.zeros(N, np.float32), wl_bound=np.zeros(N), s_extra=np.zeros(N), pol_cond=np.zeros(N), pol_q2=np.ones(N),
               rid=np.full(N, -1), near=0, facts=[])
    for rid, (src, first, count, ray_power) in enumerate(range_ids(ranges)):
        if not count:
            continue
        f = sources[src]
        image = f["shape"] >= SRC_IMAGE_RGB
        c = Ctx(seed, rid, first, count, needs_block_b(f["shape"], f["divergence"], f["div_2d"]), image)
        o = replay_source(c, f, no_pol, None if s_or is None else s_or.get(src), x_def)
        sl = slice(first, first + count)
        for k in ("p", "s", "pol", "wl", "wl_bound", "s_extra", "pol_cond"):
            res[k][sl] = o[k]
        if "pol_q2" in o:
            res["pol_q2"][sl] = o["pol_q2"]
        res["w"][sl] = np.float32(ray_power if ray_power > 0 else f["power"] / count)
        res["rid"][sl] = rid
        res["near"] += c.near
        res["facts"].append((first, count, src, o))
    return res
