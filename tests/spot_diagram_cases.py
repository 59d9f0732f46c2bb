"""The definition of the spot diagram (DESIGN.md "Spot diagrams"; include/optrace_amd.h, ot_spotdiag_*) in NumPy, written from that
text and using nothing of the package's spot diagram code.

Storage, used rays, bands and the ray lines (a, m) are those of the field analysis (tests/field_cases.py); a used ray with d_z == 0
enters nothing.  For a ray of field f and band b on plane j, in float64, one operation per component and line:

    x = a + zeta_j m        e = x - centre[f][b][j]
    scale = n_px / size     half = 0.5 n_px
    column = floor(e_x scale + half)        row = floor(e_y scale + half)

binned when both lie in [0, n_px), else outside (a value that is no number included).  These are exact integers: a ray belongs to
one cell and no other.  Per cell the weights are summed in longdouble, and the allowance of a cell is (n_cell + 2) eps sum_cell w:
n positive terms added in any order, plus the flush from LDS.  |e|^2 = e_x e_x + e_y e_y in float64; its maximum has the device's
bits; sum w |e|^2 takes |e|^2 as an exact per-ray input and is within (n + 40) eps of the sum of its terms."""
import numpy as np

import field_cases as fc
from field_cases import EPS, LD, NO_BAND  # noqa: F401  (shared with the tests)

MAX_PX, MAX_CELLS, MAX_PLANES, PAIRS, BLOCKS, MIN_BLOCKS, LDS_BYTES, TILE_AUX = 1024, 1 << 28, 65, 8, 1024, 16, 159 * 1024, 40
SIZE_FACTOR = 2.0 * (1.0 + 2.0 ** -32)  # the default side of a tile over the largest distance from a centre (spot_diagram.py)


def workspace(counts, K, Z):
    """Doubles `ot_spotdiag_workspace` asks for (include/optrace_amd.h), for fields of `counts` rays, each below 2^28."""
    KB = min(K, 4)
    tile = 3 if KB == 3 else PAIRS // KB
    groups, tiles = -(-K // KB), -(-Z // tile)
    cap = max(MIN_BLOCKS, BLOCKS // (groups * tiles))
    longest = max(1, max(min(-(-n // 256), cap) for n in counts))
    return len(counts) * longest * groups * tiles * KB * 2 * tile


def chunks(K, Z, n_px):
    """-> (chunks `ot_spotdiag_chunks` states, whether the cells are held in LDS)."""
    T = min(LDS_BYTES // (8 * n_px * n_px + TILE_AUX), K * Z)
    return (-(-K * Z // T), True) if T else (1, False)


def offsets(am, centre, zeta):
    """am (n, 4) f64: a_x, a_y, m_x, m_y; centre (2,); zeta -> e (n, 2) f64: a product, a sum and a difference per component."""
    am = np.asarray(am, dtype=np.float64)
    with np.errstate(all="ignore"):
        x = am[:, :2] + np.float64(zeta) * am[:, 2:]
        return x - np.asarray(centre, dtype=np.float64)


def cells_of(e, n_px, size):
    """e (n, 2) f64 -> (inside (n,) bool, column (n,), row (n,) int64, 0 where outside)."""
    scale, half = np.float64(n_px) / np.float64(size), np.float64(0.5 * n_px)
    with np.errstate(all="ignore"):
        q = np.floor(np.asarray(e, dtype=np.float64) * scale + half)
        inside = np.all((q >= 0) & (q < n_px), axis=1)  # (no number: False)
    q = np.where(inside[:, None], q, 0.0).astype(np.int64)
    return inside, q[:, 0], q[:, 1]


def tile(e, wt, n_px, size):
    """One tile: e (n, 2) f64, wt (n,) f32 or f64 -> dict of power (n_px, n_px) longdouble [row][column], n_cell (n_px, n_px),
    N, outside_N, outside_power (longdouble), r2max (f64), wr2, wr2_mag (longdouble)."""
    inside, col, row = cells_of(e, n_px, size)
    wl_ = np.asarray(wt).astype(LD)
    power, n_cell = np.zeros((n_px, n_px), dtype=LD), np.zeros((n_px, n_px), dtype=np.int64)
    np.add.at(power, (row[inside], col[inside]), wl_[inside])
    np.add.at(n_cell, (row[inside], col[inside]), 1)
    with np.errstate(all="ignore"):
        r2 = e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]
        terms = wl_ * r2.astype(LD)
    return dict(power=power, n_cell=n_cell, N=int(np.count_nonzero(inside)), outside_N=int(np.count_nonzero(~inside)),
                outside_power=wl_[~inside].sum(), r2max=np.float64(np.fmax.reduce(r2, initial=0.0)), wr2=terms.sum(),
                wr2_mag=np.abs(terms).sum())


def diagram(p, w, fields, k, key, key_first, K, origin, centre, zeta, n_px, size):
    """fields: [(first, count), ...]; key[r - key_first]: the band of ray r; centre (F, K, Z, 2) f64, relative to origin_xy; zeta (Z,).
    -> dict of power (F, K, Z, n_px, n_px) longdouble, n_cell, N, outside_N (F, K, Z), outside_power (longdouble), r2max (f64), wr2,
    wr2_mag (longdouble), n (F, K): the rays of a cell."""
    F, Z = len(fields), len(zeta)
    key = np.asarray(key)
    out = dict(power=np.zeros((F, K, Z, n_px, n_px), dtype=LD), n_cell=np.zeros((F, K, Z, n_px, n_px), dtype=np.int64),
               N=np.zeros((F, K, Z), dtype=np.int64), outside_N=np.zeros((F, K, Z), dtype=np.int64),
               outside_power=np.zeros((F, K, Z), dtype=LD), r2max=np.zeros((F, K, Z)), wr2=np.zeros((F, K, Z), dtype=LD),
               wr2_mag=np.zeros((F, K, Z), dtype=LD), n=np.zeros((F, K), dtype=np.int64))
    for f, (first, count) in enumerate(fields):
        if not count:
            continue
        _, inside, am = fc.lines(p, w, first, count, k, origin)
        kf = key[first - key_first:first - key_first + count]
        for b in range(K):
            m = inside & (kf == b)
            out["n"][f, b] = np.count_nonzero(m)
            if not out["n"][f, b]:
                continue
            wt = w[first:first + count, k][m]
            for j in range(Z):
                one = tile(offsets(am[m], centre[f, b, j], zeta[j]), wt, n_px, size)
                for name, v in one.items():
                    out[name][f, b, j] = v
    return out


def check_maps(power, counts, outside_power, want, what=""):
    """Device maps (F, K, Z, n_px, n_px) f64, counts (F, K, Z, 2) and outside power against `diagram`: counts equal, every cell within
    (n_cell + 2) eps sum_cell w -- a cell without a ray exactly 0 --, the power outside within (n_outside + 2) eps of it."""
    power = np.asarray(power, dtype=np.float64).reshape(want["power"].shape)
    counts = np.asarray(counts).astype(np.int64).reshape(want["N"].shape + (2,))
    assert np.array_equal(counts[..., 0], want["N"]), f"{what}: rays binned {counts[..., 0].ravel()[:12]} against {want['N'].ravel()[:12]}"
    assert np.array_equal(counts[..., 1], want["outside_N"]), f"{what}: rays outside"
    assert not np.any(np.isnan(power)), f"{what}: a cell is no number"
    err = np.abs(power.astype(LD) - want["power"]).astype(np.float64)
    allow = (want["n_cell"] + 2) * EPS * want["power"].astype(np.float64)
    over = err > allow
    assert not np.any(over), f"{what}: {np.count_nonzero(over)} cells off, first at {np.argwhere(over)[0]}: {err[over][0]} above {allow[over][0]}"
    out = np.asarray(outside_power, dtype=np.float64).reshape(want["N"].shape)
    err_o = np.abs(out.astype(LD) - want["outside_power"]).astype(np.float64)
    assert np.all(err_o <= (want["outside_N"] + 2) * EPS * want["outside_power"].astype(np.float64)), f"{what}: the power outside"
    with np.errstate(invalid="ignore", divide="ignore"):
        worst = float(np.max(np.where(allow > 0, err / allow, 0.0), initial=0.0))
    print(f"{what}: cells use at most {worst:.3g} of their allowance")
    return worst


def check_extents(ext, want, what=""):
    """Device extents (F, K, Z, 2) against `diagram`: max |e|^2 the same bits, sum w |e|^2 within (n + 40) eps of the sum of its terms."""
    ext = np.asarray(ext, dtype=np.float64).reshape(want["N"].shape + (2,))
    assert np.array_equal(ext[..., 0].view(np.uint64), np.ascontiguousarray(want["r2max"]).view(np.uint64)), f"{what}: max |e|^2 differs in bits"
    n = want["n"][:, :, None].astype(np.float64)
    fin = np.isfinite(want["wr2_mag"].astype(np.float64))
    err = np.abs(ext[..., 1].astype(LD) - want["wr2"]).astype(np.float64)
    bound = (n + 40) * EPS * want["wr2_mag"].astype(np.float64)
    assert np.all(err[fin] <= bound[fin]), f"{what}: sum w |e|^2 off by {err[fin].max()} at the most"
    assert not np.any(np.isfinite(ext[..., 1][~fin])), f"{what}: a sum beyond every number came out finite"
