"""Inputs and NumPy references for the stage that turns hits into results: RenderImage.render (binning_indices_2d misc.py:59-91,
render_image.py:396-418) and LightSpectrum.render (light_spectrum.py:41-79).  No device code: tests/test_binning_host.py checks
the references against the CPU oracle, tests/test_gpu_binning.py holds every device route to them.

Pixel membership  `pixel_index`: the reference's rule in float64, operation by operation -- fx = Nx / (x1 - x0),
                  floor(fx * (x - x0)), the `== x1` / `== y1` rule, then the range test.  The range test is made on the floored
                  float64 (NaN, +-inf and indices beyond int32 are outside: the reference's int32 conversion gives INT_MIN there).
Observer lookup   `observer_terms`: np.interp's definition on the 471-node CIE table in np.longdouble (NaN for a NaN wavelength).
Image             `reference_image`: per pixel the hit count k, the sums in np.longdouble and the derived bounds.
Spectrum          `spectrum_counts`: np.histogram's own integer counts for float32 data and float32 range.

Every list carries the class of each entry (`Hits.cls`), so that a test can show that a generator produced what it was asked for.
"""
from __future__ import annotations

import functools
import pathlib

import numpy as np

ROOT = pathlib.Path(__file__).resolve().parent.parent
EPS = 2.0 ** -53

SHAPES = [(1, 1), (3, 5), (64, 64), (63, 65), (129, 1), (1, 130), (200, 70), (945, 315)]
EXTENTS = {
    "unit": [-1.0, 1.0, -1.0, 1.0],
    "asym": [-0.37, 1.93, 2.1, 2.8],                           # non-dyadic, asymmetric
    "far": [1000.0, 1000.001, -1000.0005, -999.9995],          # offset 1e3, width 1e-3
    "tiny": [0.25, 0.25 + 1e-9, -3e-10, 7e-10],                # width 1e-9
    "zero_edge": [0.0, 1.5, -0.75, 0.0],                       # edges at 0: -0.0 is a position on them
}

HIT_CLASSES = ["interior", "boundary_x", "boundary_y", "boundary_xy", "extent_edge", "corner", "neg_zero", "nonfinite",
               "huge_index"]
WEIGHT_CLASSES = ["w_zero", "w_neg_zero", "w_nan", "w_negative", "w_subnormal", "w_ordinary"]
WL_CLASSES = ["wl_node", "wl_table_end_ulp", "wl_outside", "wl_nan", "wl_between"]
COUNT_CLASSES = ["n1", "n63", "n64", "n65", "n1023", "n1024", "n1025", "several_workgroups", "two_slabs", "empty_tiles_between",
                 "last_partial_tile"]
WAVE_CLASSES = ["one_pixel", "share7", "share8", "share9", "four_keys", "eight_by_eight", "lane63_singleton", "lane63_first_key",
                "invalid_interleaved", "last_wave_1", "last_wave_63", "hash_collisions", "hash_overflow"]
SPECTRUM_CLASSES = ["edge", "edge_below", "edge_above", "first_last", "just_outside", "nan", "between"]


class Hits:
    """A hit list: x, y (f64), w, wl (f32) and the class names of every entry (position, weight, wavelength)."""

    def __init__(self):
        self.x, self.y, self.w, self.wl, self.cls = [], [], [], [], []

    def add(self, cls, x, y, w=1.0, wl=555.0):
        x, y = np.atleast_1d(np.asarray(x, dtype=np.float64)), np.atleast_1d(np.asarray(y, dtype=np.float64))
        n = max(x.shape[0], y.shape[0])
        self.x.append(np.broadcast_to(x, n))
        self.y.append(np.broadcast_to(y, n))
        self.w.append(np.broadcast_to(np.asarray(w, dtype=np.float32), n))
        self.wl.append(np.broadcast_to(np.asarray(wl, dtype=np.float32), n))
        self.cls.append(np.full(n, cls, dtype=object))
        return self

    def done(self):
        self.x, self.y = np.ascontiguousarray(np.concatenate(self.x)), np.ascontiguousarray(np.concatenate(self.y))
        self.w, self.wl = np.ascontiguousarray(np.concatenate(self.w)), np.ascontiguousarray(np.concatenate(self.wl))
        self.cls = np.concatenate(self.cls)
        self.wcls = np.full(self.n, "", dtype=object)
        self.wlcls = np.full(self.n, "", dtype=object)
        return self

    @property
    def n(self):
        return self.x.shape[0]

    def classes(self) -> dict:
        out = {}
        for arr in (self.cls, self.wcls, self.wlcls):
            names, counts = np.unique(arr[arr != ""].astype(str), return_counts=True)
            out.update(dict(zip(names.tolist(), counts.tolist())))
        return out


class Case:
    def __init__(self, name, Nx, Ny, extent, hits: Hits, mode, expects):
        self.name, self.Nx, self.Ny, self.extent, self.hits, self.mode = name, Nx, Ny, [float(v) for v in extent], hits, mode
        self.expects = list(expects)  # classes this case must contain

    def __repr__(self):
        return self.name


# ---- references -------------------------------------------------------------------------------------------------------------
def pixel_index(x, y, Nx, Ny, extent) -> np.ndarray:
    """Pixel iy * Nx + ix of every position by the reference's rule, -1 where the reference sets the weight to zero."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    x0, x1, y0, y1 = (np.float64(v) for v in extent)
    with np.errstate(all="ignore"):
        fx = np.float64(Nx) / (x1 - x0)
        fy = np.float64(Ny) / (y1 - y0)
        gx = np.floor(fx * (x - x0))
        gy = np.floor(fy * (y - y0))
        gy = np.where(y == y1, np.float64(Ny - 1), gy)
        gx = np.where(x == x1, np.float64(Nx - 1), gx)
        inside = (gx >= 0) & (gy >= 0) & (gy < Ny) & (gx < Nx)  # (false for NaN)
    pix = np.full(x.shape[0], -1, dtype=np.int64)
    pix[inside] = gy[inside].astype(np.int64) * Nx + gx[inside].astype(np.int64)
    return pix


@functools.lru_cache(maxsize=None)
def observer_table() -> np.ndarray:
    """(471, 4) wl, x, y, z: the oracle's table (tests/test_oracle_golden.py pins it to the reference)."""
    tab = np.ascontiguousarray(np.load(ROOT / "optrace_amd" / "data" / "cie_tables.npz")["observers"], dtype=np.float64)
    assert tab.shape == (471, 4) and tab[0, 0] == 360.0 and tab[-1, 0] == 830.0
    return tab


def observer_terms(wl):
    """np.interp(wl, table wl, table c, left=0, right=0) for c = x, y, z, written out in np.longdouble.
    -> (value (n, 3) longdouble, NaN for a NaN wavelength; magnitude (n, 3) longdouble: |d t| + |v| of the interpolation
    v + d t between the nodes (|v| at and beyond the last node, 0 outside the table and for NaN))."""
    LD = np.longdouble
    tab = observer_table()
    xp, fp = tab[:, 0].astype(LD), tab[:, 1:].astype(LD)
    l = np.asarray(wl, dtype=np.float32).astype(LD)
    n = l.shape[0]
    val, mag = np.zeros((n, 3), dtype=LD), np.zeros((n, 3), dtype=LD)
    nan = np.isnan(l)
    with np.errstate(invalid="ignore"):
        inside = ~nan & (l >= xp[0]) & (l <= xp[-1])
    li = l[inside]
    j = np.minimum(np.floor(li - xp[0]).astype(np.int64), xp.shape[0] - 1)  # largest j with xp[j] <= l (1 nm grid)
    last = j == xp.shape[0] - 1
    jj = np.where(last, j - 1, j)
    slope = (fp[jj + 1] - fp[jj]) / (xp[jj + 1] - xp[jj])[:, None]
    t = (li - xp[jj])[:, None]
    v = np.where(last[:, None], fp[j], slope * t + fp[jj])
    m = np.where(last[:, None], np.abs(fp[j]), np.abs(slope * t) + np.abs(fp[jj]))
    val[inside], mag[inside] = v, m
    val[nan] = np.nan
    return val, mag


def reference_image(x, y, w, wl, Nx, Ny, extent, sparse=False) -> dict:
    """The image the reference forms from these hits, per pixel (flat, iy * Nx + ix; `sparse`: per pixel with a hit that adds,
    `ids` their sorted pixel numbers -- every other pixel of the image is exactly zero):
    k        hits that add (inside by the pixel rule, weight neither 0 nor NaN; negative weights add)
    w3       channel 3: sum of the weights, longdouble (exact for dyadic weights)
    absw     sum |w|
    xyz      (npx, 3) channels 0..2: sum of observer value times weight, longdouble; NaN where a hit with a NaN wavelength adds
    mag      (npx, 3) sum (|d t| + |v|) |w| of the same terms, for the bound (k + 3) eps mag
    pix      pixel of every hit, -1 for one that adds nothing"""
    LD = np.longdouble
    w = np.asarray(w, dtype=np.float32)
    pix = pixel_index(x, y, Nx, Ny, extent)
    with np.errstate(invalid="ignore"):
        adds = (pix >= 0) & (w != 0) & ~np.isnan(w)
    pix = np.where(adds, pix, -1)
    npx = Nx * Ny
    p, wv = pix[adds], w[adds].astype(LD)
    ids = None
    if sparse:
        ids, p = np.unique(p, return_inverse=True)
        npx = ids.shape[0]
    val, mag = observer_terms(np.asarray(wl, dtype=np.float32)[adds])
    k = np.bincount(p, minlength=npx)
    w3, absw = np.zeros(npx, dtype=LD), np.zeros(npx, dtype=LD)
    xyz, mg = np.zeros((npx, 3), dtype=LD), np.zeros((npx, 3), dtype=LD)
    np.add.at(w3, p, wv)
    np.add.at(absw, p, np.abs(wv))
    with np.errstate(invalid="ignore"):
        np.add.at(xyz, p, val * wv[:, None])
    np.add.at(mg, p, mag * np.abs(wv)[:, None])
    return dict(k=k, w3=w3, absw=absw, xyz=xyz, mag=mg, pix=pix, ids=ids)


def check_image(got, ref, mode, what="") -> float:
    """`got` (Ny, Nx, 4) f64 against `reference_image`.  mode "unit" / "dyadic": channel 3 equal bit for bit (every partial sum
    of multiples of 2^-10 below 2^40 is exact in any order); "ordinary": lit mask equal and |got - ref| <= (k - 1) eps sum |w|.
    XYZ: |got - ref| <= (k + 3) eps sum (|d t| + |v|) |w| per pixel and channel, NaN exactly where the reference has NaN.
    -> worst observed ratio of an XYZ error to its bound."""
    got = np.asarray(got, dtype=np.float64).reshape(-1, 4)
    if ref.get("ids") is not None:  # a sparse reference: nothing anywhere else, then the pixels with hits
        rest = np.ones(got.shape[0], dtype=bool)
        rest[ref["ids"]] = False
        bad = np.flatnonzero((got[rest] != 0).any(axis=1))
        assert bad.size == 0, f"{what}: {bad.size} pixels without a hit are not zero, first {np.flatnonzero(rest)[bad[:5]]}"
        got = got[ref["ids"]]
    k = ref["k"]
    w3 = ref["w3"].astype(np.float64)
    assert got.shape[0] == k.shape[0], what
    if mode in ("unit", "dyadic"):
        bad = np.flatnonzero(got[:, 3] != w3)
        assert bad.size == 0, f"{what}: channel 3 differs in {bad.size} pixels, first {bad[:5]}: got {got[bad[:5], 3]} want {w3[bad[:5]]}"
    else:
        bad = np.flatnonzero((got[:, 3] != 0) != (ref["w3"] != 0))
        assert bad.size == 0, f"{what}: lit mask differs in {bad.size} pixels, first {bad[:5]}"
        err = np.abs(got[:, 3].astype(np.longdouble) - ref["w3"])
        bound = np.maximum(k - 1, 0) * EPS * ref["absw"]
        bad = np.flatnonzero(~(err <= bound))
        assert bad.size == 0, f"{what}: channel 3 beyond (k - 1) eps sum |w| in {bad.size} pixels, first {bad[:5]}"
    want_nan = np.isnan(ref["xyz"])
    got_nan = np.isnan(got[:, :3])
    assert np.array_equal(got_nan, want_nan), f"{what}: NaN in XYZ at pixels {np.flatnonzero((got_nan != want_nan).any(axis=1))[:5]}"
    fin = ~want_nan
    err = np.abs(got[:, :3].astype(np.longdouble) - ref["xyz"])
    bound = (k + 3)[:, None] * EPS * ref["mag"]
    bad = np.flatnonzero((fin & ~(err <= bound)).any(axis=1))
    assert bad.size == 0, (f"{what}: XYZ beyond (k + 3) eps sum (|d t| + |v|) |w| in {bad.size} pixels, first {bad[:5]}: "
                           f"got {got[bad[:3], :3]} want {ref['xyz'][bad[:3]]} k {k[bad[:3]]}")
    sel = fin & (bound > 0)
    return float(np.max(err[sel] / bound[sel])) if sel.any() else 0.0


def spectrum_counts(wl, first, last, nbins) -> np.ndarray:
    """NumPy's own integer counts: np.histogram of float32 data over a float32 range, unit weights."""
    wl = np.asarray(wl, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        counts, edges = np.histogram(wl, bins=int(nbins), range=(np.float32(first), np.float32(last)))
    assert edges.dtype == np.float32
    assert np.array_equal(edges, np.linspace(np.float32(first), np.float32(last), int(nbins) + 1, dtype=np.float32))
    return counts.astype(np.int64)


# ---- hit lists --------------------------------------------------------------------------------------------------------------
def _around(v):
    v = np.float64(v)
    return np.array([np.nextafter(v, -np.inf), v, np.nextafter(v, np.inf)])


def _inside(rng, a, b, n):
    """n positions strictly inside (a, b)"""
    return a + (b - a) * (0.02 + 0.96 * rng.random(n))


def edge_hits(Nx, Ny, extent, rng, n_interior=400) -> Hits:
    """Random interior hits and every decision point of the pixel rule for this grid, each with weight 1 (`assign_weights` and
    `assign_wavelengths` replace weights and wavelengths afterwards)."""
    x0, x1, y0, y1 = (np.float64(v) for v in extent)
    ix = lambda n: _inside(rng, x0, x1, n)
    iy = lambda n: _inside(rng, y0, y1, n)
    h = Hits()
    h.add("interior", ix(n_interior), iy(n_interior))
    # every pixel boundary as float64 forms it, with its neighbours on both sides
    bx = np.array([x0 + k * (x1 - x0) / Nx for k in range(Nx + 1)])
    by = np.array([y0 + k * (y1 - y0) / Ny for k in range(Ny + 1)])
    X = np.concatenate([_around(b) for b in bx])
    Y = np.concatenate([_around(b) for b in by])
    h.add("boundary_x", X, iy(X.shape[0]))
    h.add("boundary_y", ix(Y.shape[0]), Y)
    m = max(Nx, Ny) + 1
    for q in range(m):  # both at once: boundary q of x with boundary q of y (cyclic), all nine neighbour pairs
        ax, ay = _around(bx[q % (Nx + 1)]), _around(by[(q * 7 + 3) % (Ny + 1)])
        h.add("boundary_xy", np.repeat(ax, 3), np.tile(ay, 3))
    # the extent itself: one ulp inside, on, one ulp outside
    for v in (x0, x1):
        h.add("extent_edge", _around(v), iy(3))
    for v in (y0, y1):
        h.add("extent_edge", ix(3), _around(v))
    for cx in (x0, x1):
        for cy in (y0, y1):
            h.add("corner", np.repeat(_around(cx), 3), np.tile(_around(cy), 3))
    if x0 == 0 or x1 == 0:
        h.add("neg_zero", [-0.0, -0.0], [y0, iy(1)[0]])
    if y0 == 0 or y1 == 0:
        h.add("neg_zero", [x1, ix(1)[0]], [-0.0, -0.0])
    if (x0 == 0 or x1 == 0) and (y0 == 0 or y1 == 0):
        h.add("neg_zero", [-0.0], [-0.0])
    bad = np.array([np.inf, -np.inf, np.nan, 1e300, -1e300])
    h.add("nonfinite", bad, iy(5))
    h.add("nonfinite", ix(5), bad)
    h.add("nonfinite", bad, bad[::-1])
    # finite positions whose scaled index lies beyond int32 in either sign
    for mlt in (2.0 ** 31 + 4096, 2.0 ** 32 + 4096, 2.0 ** 33, 1e12):  # (4096: well beyond the rounding of x itself)
        for sg in (1.0, -1.0):
            h.add("huge_index", [x0 + sg * mlt * (x1 - x0) / Nx], iy(1))
            h.add("huge_index", ix(1), [y0 + sg * mlt * (y1 - y0) / Ny])
    return h.done()


def subset_with_weight(h: Hits, cls, w, every=7) -> Hits:
    """copies of every `every`-th hit of h with the weight `w`: positions of every kind under a weight that adds nothing (or little)"""
    sel = np.arange(0, h.n, every)
    out = Hits().add("copy", h.x[sel], h.y[sel], w=w).done()
    out.cls = h.cls[sel].copy()
    out.wcls[:] = cls
    return out


def concat(parts) -> Hits:
    out = Hits()
    out.x, out.y = np.concatenate([p.x for p in parts]), np.concatenate([p.y for p in parts])
    out.w, out.wl = np.concatenate([p.w for p in parts]), np.concatenate([p.wl for p in parts])
    out.cls = np.concatenate([p.cls for p in parts])
    out.wcls = np.concatenate([p.wcls for p in parts])
    out.wlcls = np.concatenate([p.wlcls for p in parts])
    return out


def assign_weights(h: Hits, mode, rng, Nx, Ny, extent) -> Hits:
    """Non-zero weights for every hit of h, then copies under the weights that add nothing.
    unit:     1
    dyadic:   multiples of 2^-10 up to 4, a quarter of them negative (sums exact in any order)
    ordinary: random float32 and the smallest float32 subnormal; all hits of a pixel carry one sign (every fifth pixel the
              negative one), so that no sum cancels and the lit mask is the mask of pixels with a hit"""
    n = h.n
    if mode == "unit":
        h.w = np.ones(n, dtype=np.float32)
        h.wcls[:] = "w_ordinary"
    elif mode == "dyadic":
        h.w = (rng.integers(1, 4097, n) / 1024.0).astype(np.float32)
        neg = rng.random(n) < 0.25
        h.w[neg] = -h.w[neg]
        h.wcls[:] = np.where(neg, "w_negative", "w_ordinary")
    else:
        h.w = (0.01 + 2 * rng.random(n)).astype(np.float32)
        sub = np.arange(n) % 13 == 5
        h.w[sub] = np.float32(1e-45)
        pix = pixel_index(h.x, h.y, Nx, Ny, extent)
        neg = (pix % 5 == 0) & (pix >= 0)
        h.w[neg] = -h.w[neg]
        h.wcls[:] = np.where(neg, "w_negative", np.where(sub, "w_subnormal", "w_ordinary"))
        assert np.float32(1e-45) > 0 and np.float32(1e-45) == np.finfo(np.float32).smallest_subnormal
    parts = [h, subset_with_weight(h, "w_zero", 0.0), subset_with_weight(h, "w_neg_zero", -0.0, every=11),
             subset_with_weight(h, "w_nan", np.nan, every=5)]
    return concat(parts)


def wavelength_pool(rng) -> tuple:
    f32 = np.float32
    nodes = np.arange(360, 831).astype(f32)
    ends = np.array([np.nextafter(f32(360), f32(0)), np.nextafter(f32(360), f32(1e3)), np.nextafter(f32(830), f32(0)),
                     np.nextafter(f32(830), f32(1e4))], dtype=f32)
    outside = np.array([100.0, 359.5, 830.5, 2000.0, -10.0, 0.0, np.inf, -np.inf], dtype=f32)
    between = (360 + 470 * rng.random(240)).astype(f32)
    pool = np.concatenate([nodes, ends, outside, between])
    names = np.concatenate([np.full(471, "wl_node", dtype=object), np.full(4, "wl_table_end_ulp", dtype=object),
                            np.full(8, "wl_outside", dtype=object), np.full(240, "wl_between", dtype=object)])
    return pool, names


def assign_wavelengths(h: Hits, rng, n_nan=3) -> Hits:
    """Every table node, one float32 ulp on both sides of 360 and 830, values outside the table and values between the nodes,
    dealt out over the hits in a random order; NaN on `n_nan` of the interior hits."""
    pool, names = wavelength_pool(rng)
    order = rng.permutation(pool.shape[0])
    idx = order[np.arange(h.n) % pool.shape[0]]
    h.wl = pool[idx].copy()
    h.wlcls = names[idx].copy()
    first = np.flatnonzero((h.cls == "interior") & (h.wcls != "w_zero") & (h.wcls != "w_neg_zero") & (h.wcls != "w_nan"))[:n_nan]
    h.wl[first] = np.nan
    h.wlcls[first] = "wl_nan"
    return h


@functools.lru_cache(maxsize=None)
def edge_cases() -> list:
    """Every shape with every extent: unit weights for the small shapes (exact counts), dyadic and ordinary weights in turn."""
    cases = []
    modes = ["unit", "dyadic", "ordinary"]
    q = 0
    for si, (Nx, Ny) in enumerate(SHAPES):
        for ei, (ename, ext) in enumerate(EXTENTS.items()):
            rng = np.random.default_rng(1000 + 31 * si + ei)
            mode = modes[q % 3]
            q += 1
            h = edge_hits(Nx, Ny, ext, rng)
            h = assign_weights(h, mode, rng, Nx, Ny, ext)
            h = assign_wavelengths(h, rng)
            expects = [c for c in HIT_CLASSES if c != "neg_zero" or ename == "zero_edge"]
            expects += ["w_zero", "w_neg_zero", "w_nan", "w_ordinary"] + WL_CLASSES
            if mode != "unit":
                expects += ["w_negative"]
            if mode == "ordinary":
                expects += ["w_subnormal"]
            cases.append(Case(f"{Nx}x{Ny}-{ename}-{mode}", Nx, Ny, ext, h, mode, expects))
    return cases


# ---- counts -----------------------------------------------------------------------------------------------------------------
def _pixel_centres(pix, Nx, Ny, extent):
    x0, x1, y0, y1 = extent
    pix = np.asarray(pix, dtype=np.int64)
    return x0 + (pix % Nx + 0.5) * (x1 - x0) / Nx, y0 + (pix // Nx + 0.5) * (y1 - y0) / Ny


def _finish(h: Hits, rng, cls, n_nan=0) -> Hits:
    h = h.done()
    h.w = (rng.integers(1, 4097, h.n) / 1024.0).astype(np.float32) * np.where(h.w == 0, 0, 1).astype(np.float32)
    h.wcls[:] = "w_ordinary"
    h = assign_wavelengths(h, rng, n_nan=n_nan)
    h.cls[:] = cls
    return h


@functools.lru_cache(maxsize=None)
def count_cases() -> list:
    """List lengths at the steps of the kernels (wave, workgroup, chunk of the tile accumulation) and tile occupancies."""
    cases = []
    Nx, Ny, ext = 63, 65, EXTENTS["asym"]
    for n in (1, 63, 64, 65, 1023, 1024, 1025):
        rng = np.random.default_rng(2000 + n)
        h = Hits().add("c", _inside(rng, ext[0] - 0.1, ext[1] + 0.1, n), _inside(rng, ext[2] - 0.05, ext[3] + 0.05, n))
        cases.append(Case(f"n{n}", Nx, Ny, ext, _finish(h, rng, f"n{n}"), "dyadic", [f"n{n}"]))
    # several workgroups of the direct kernel (one per 1024 hits)
    rng = np.random.default_rng(2100)
    n = 5 * 1024 + 77
    h = Hits().add("c", _inside(rng, ext[0] - 0.1, ext[1] + 0.1, n), _inside(rng, ext[2] - 0.05, ext[3] + 0.05, n))
    cases.append(Case("several_workgroups", Nx, Ny, ext, _finish(h, rng, "several_workgroups"), "dyadic", ["several_workgroups"]))
    # 200 x 70: 4 x 2 tiles of 64 x 64, the last column 8 wide and the last row 6 high
    Nx, Ny, ext = 200, 70, EXTENTS["unit"]
    tile_pixels = lambda tx, ty: np.array([iy * Nx + ix for iy in range(64 * ty, min(64 * ty + 64, Ny))
                                           for ix in range(64 * tx, min(64 * tx + 64, Nx))])
    rng = np.random.default_rng(2200)
    px = rng.choice(tile_pixels(1, 0), 40_000)  # more than 16384 hits in one tile: two slabs of tile 1
    x, y = _pixel_centres(np.concatenate([px, rng.choice(tile_pixels(3, 1), 50)]), Nx, Ny, ext)
    cases.append(Case("two_slabs", Nx, Ny, ext, _finish(Hits().add("c", x, y), rng, "two_slabs"), "dyadic", ["two_slabs"]))
    rng = np.random.default_rng(2300)
    px = np.concatenate([rng.choice(tile_pixels(0, 0), 700), rng.choice(tile_pixels(3, 0), 300), rng.choice(tile_pixels(2, 1), 500)])
    x, y = _pixel_centres(rng.permutation(px), Nx, Ny, ext)
    cases.append(Case("empty_tiles_between", Nx, Ny, ext, _finish(Hits().add("c", x, y), rng, "empty_tiles_between"), "dyadic",
                      ["empty_tiles_between"]))
    rng = np.random.default_rng(2400)
    x, y = _pixel_centres(rng.choice(tile_pixels(3, 1), 900), Nx, Ny, ext)
    cases.append(Case("last_partial_tile", Nx, Ny, ext, _finish(Hits().add("c", x, y), rng, "last_partial_tile"), "dyadic",
                      ["last_partial_tile"]))
    return cases


# ---- waves composed on purpose ----------------------------------------------------------------------------------------------
HASH_BITS = 11  # OT_HASH_N = 2^11 entries in the LDS table of render_kernel, OT_HASH_PROBES = 4 probes


def hash_slot(pix) -> np.ndarray:
    """render_kernel's slot of a pixel id: (pix * 2654435761 mod 2^32) >> 21"""
    return ((np.asarray(pix, dtype=np.uint64) * np.uint64(2654435761)) & np.uint64(0xFFFFFFFF)) >> np.uint64(32 - HASH_BITS)


def colliding_pixels(npx, want=9) -> np.ndarray:
    """`want` pixel ids below npx with one common slot"""
    slots = hash_slot(np.arange(npx))
    order = np.argsort(slots, kind="stable")
    s = slots[order]
    start = np.flatnonzero(np.r_[True, s[1:] != s[:-1]])
    length = np.diff(np.r_[start, s.shape[0]])
    g = int(np.argmax(length >= want))
    assert length[g] >= want
    out = order[start[g]:start[g] + want]
    assert np.unique(hash_slot(out)).size == 1 and np.unique(out).size == want
    return out


def wave_groups(rng, npx) -> list:
    """-> [(class, pixel id per lane (64), -1 = a lane that adds nothing)]: compositions of one wave of the direct kernels.
    wave_add4_by_key sums the lanes of up to three keys with at least eight lanes each (lane 63 delivers each sum); every
    other lane adds for itself."""
    fresh = iter(rng.permutation(npx))
    new = lambda n=1: np.array([next(fresh) for _ in range(n)], dtype=np.int64)
    groups = []
    groups.append(("one_pixel", np.full(64, new()[0])))
    for share in (7, 8, 9):
        lanes = new(64)
        at = rng.choice(64, share, replace=False)
        lanes[at] = lanes[at[0]]
        groups.append((f"share{share}", lanes))
        lanes = new(64)  # the same with the shared lanes in front: the first leader's key
        lanes[:share] = lanes[0]
        groups.append((f"share{share}", lanes))
    keys = new(4)
    groups.append(("four_keys", np.repeat(keys, 16)))                      # A x16, B x16, C x16, D x16: D lane by lane
    groups.append(("four_keys", np.tile(keys, 16)))                        # interleaved: leaders in lanes 0, 1, 2
    lanes = np.concatenate([np.repeat(keys[:3], 8), np.repeat(keys[3:], 40)])  # the fourth key holds most lanes and lane 63
    groups.append(("four_keys", lanes))
    groups.append(("eight_by_eight", np.repeat(new(8), 8)))
    groups.append(("eight_by_eight", np.tile(new(8), 8)))
    lanes = new(64)  # lane 63 a singleton while it delivers the sums of two other keys
    lanes[0:16] = lanes[0]
    lanes[20:30] = lanes[20]
    groups.append(("lane63_singleton", lanes))
    lanes = new(64)  # lane 63 belongs to the first key (with lane 0), a second key in between
    lanes[[0, 5, 9, 17, 33, 40, 62, 63]] = lanes[0]
    lanes[20:32] = lanes[20]
    groups.append(("lane63_first_key", lanes))
    lanes = np.repeat(new(4), 16)  # lanes that add nothing in between, the leaders among them
    lanes[::3] = -1
    groups.append(("invalid_interleaved", lanes))
    lanes = np.full(64, new()[0])
    lanes[[0, 1, 2, 62, 63]] = -1
    groups.append(("invalid_interleaved", lanes))
    return groups


def _wave_list(groups, Nx, Ny, extent, rng, tail=None):
    """Hit list of whole 64-lane groups (and a shorter `tail` group).  A lane that adds nothing has weight 0 or lies outside."""
    h = Hits()
    for gi, (cls, lanes) in enumerate(list(groups) + ([tail] if tail is not None else [])):
        valid = lanes >= 0
        x, y = _pixel_centres(np.where(valid, lanes, 0), Nx, Ny, extent)
        w = np.ones(lanes.shape[0], dtype=np.float32)
        off = np.flatnonzero(~valid)
        w[off[::2]] = 0.0                          # w = 0 ...
        x = x.copy()
        x[off[1::2]] = extent[1] + (extent[1] - extent[0])  # ... or outside the extent
        h.add(cls, x, y, w=w)
    return h


@functools.lru_cache(maxsize=None)
def wave_cases() -> list:
    cases = []
    Nx, Ny, ext = 200, 70, EXTENTS["asym"]
    for k, (tail_n, tail_cls) in enumerate([(0, None), (1, "last_wave_1"), (63, "last_wave_63")]):
        rng = np.random.default_rng(3000 + k)
        groups = wave_groups(rng, Nx * Ny)
        tail = (tail_cls, np.full(tail_n, 17 * 200 + 31)) if tail_n else None
        h = _wave_list(groups, Nx, Ny, ext, rng, tail).done()
        cls = h.cls.copy()
        zero = h.w == 0
        h.w = (rng.integers(1, 4097, h.n) / 1024.0).astype(np.float32)
        h.w[zero] = 0
        h.wcls[:] = "w_ordinary"
        h = assign_wavelengths(h, rng, n_nan=0)
        h.cls = cls
        expects = [c for c in WAVE_CLASSES if not c.startswith(("last_wave", "hash"))] + ([tail_cls] if tail_cls else [])
        cases.append(Case(f"waves-tail{tail_n}", Nx, Ny, ext, h, "dyadic", expects))
    # more than four pixel ids with one slot of the LDS hash, all from one workgroup: the fifth and later go to global atomics
    Nx, Ny, ext = 945, 315, EXTENTS["unit"]
    rng = np.random.default_rng(3100)
    ids = colliding_pixels(Nx * Ny, 9)
    px = np.concatenate([np.repeat(ids, 5), rng.permutation(np.repeat(ids, 40)), np.tile(ids, 7)])[:1024]
    x, y = _pixel_centres(px, Nx, Ny, ext)
    cases.append(Case("hash_collisions", Nx, Ny, ext, _finish(Hits().add("c", x, y), rng, "hash_collisions"), "dyadic",
                      ["hash_collisions"]))
    return cases


def hash_overflow_case(workgroups: int) -> Case:
    """More than 2048 distinct pixels from every workgroup of the direct kernel: 3072 hits per workgroup of a grid of `workgroups`
    (one per compute unit), each list position its own pixel as far as the image has pixels."""
    Nx, Ny, ext = 945, 315, EXTENTS["unit"]
    rng = np.random.default_rng(3200)
    n = workgroups * 3072
    px = (np.arange(n, dtype=np.int64) * 7919) % (Nx * Ny)
    x, y = _pixel_centres(px, Nx, Ny, ext)
    h = Hits().add("hash_overflow", x, y).done()
    h.wcls[:] = "w_ordinary"
    h.wlcls[:] = "wl_between"
    h.wl = (400 + 300 * rng.random(n)).astype(np.float32)
    return Case("hash_overflow", Nx, Ny, ext, h, "unit", ["hash_overflow"])


# ---- compact lists ----------------------------------------------------------------------------------------------------------
PIECES = 1024


def compact_layout(n, piece_len, rng) -> tuple:
    """Where the n hits of a dense list go in a compact list of 1024 pieces of `piece_len` entries: piece 0 full (if the list is
    long enough), piece 1 empty, piece 2 with one entry, every third piece after it empty, the last piece used, the rest of the
    hits dealt out at random, in list order.  -> (fill (1024,) uint32, position of every hit)"""
    fill = np.zeros(PIECES, dtype=np.int64)
    left = n
    if left >= piece_len + 2:
        fill[0] = piece_len
        left -= piece_len
    if left >= 1:
        fill[2] = 1
        left -= 1
    if left >= 1:
        fill[PIECES - 1] = min(left, 3)
        left -= fill[PIECES - 1]
    usable = np.array([p for p in range(3, PIECES - 1) if p % 3 != 0])
    assert left <= 0.9 * usable.shape[0] * piece_len, "list too long for this layout"
    most = 200 if n < 100_000 else piece_len
    while left > 0:
        p = usable[rng.integers(0, usable.shape[0])]
        take = min(left, int(rng.integers(1, most)), piece_len - fill[p])
        fill[p] += take
        left -= take
    assert fill.sum() == n and fill.max() <= piece_len
    pos = np.concatenate([p * piece_len + np.arange(fill[p]) for p in range(PIECES) if fill[p]]) if n else np.zeros(0, dtype=np.int64)
    return fill.astype(np.uint32), pos.astype(np.int64)


# ---- spectra ----------------------------------------------------------------------------------------------------------------
class SpectrumCase:
    def __init__(self, name, first, last, nbins, wl, cls):
        self.name, self.first, self.last, self.nbins = name, np.float32(first), np.float32(last), int(nbins)
        self.wl, self.cls = np.ascontiguousarray(wl, dtype=np.float32), cls
        self.edges = np.linspace(self.first, self.last, self.nbins + 1, endpoint=True, dtype=np.float32)

    def classes(self) -> dict:
        names, counts = np.unique(self.cls.astype(str), return_counts=True)
        return dict(zip(names.tolist(), counts.tolist()))

    def __repr__(self):
        return self.name


# hist_shape (optrace_amd/csrc/ot_host.hpp:76-79, `lds_wanted <= 64 * 1024`): sums (f64) and edges (f32) in LDS up to this many
# bytes.  A copy of that constant: if the source's limit moves, the 6001-bin case still pins the result but no longer the form.
HIST_LDS_LIMIT = 64 * 1024


def hist_lds_bytes(nbins: int) -> int:
    """what spectrum_histogram asks hist_shape for: nbins f64 sums and nbins + 2 f32 edges"""
    return nbins * 8 + (nbins + 2) * 4


SPECTRUM_BINS = [1, 2, 51, 1001, 6001]  # 6001 bins: 72 KB, beyond the LDS limit -- global atomics
SPECTRUM_RANGES = [(380.0, 780.0), (401.3, 698.7)]


@functools.lru_cache(maxsize=None)
def spectrum_cases() -> list:
    """A wavelength on every float32 edge of np.linspace(first, last, nbins + 1) and one float32 ulp on both sides of it, on
    `first` and `last` and just outside them, NaN, and values between the edges."""
    f32 = np.float32
    cases = []
    for nbins in SPECTRUM_BINS:
        for ri, (first, last) in enumerate(SPECTRUM_RANGES):
            rng = np.random.default_rng(4000 + 7 * nbins + ri)
            first, last = f32(first), f32(last)
            e = np.linspace(first, last, nbins + 1, endpoint=True, dtype=np.float32)
            below, above = np.nextafter(e, f32(-np.inf)), np.nextafter(e, f32(np.inf))
            outside = np.array([below[0], above[-1], first - f32(1), last + f32(1), -np.inf, np.inf, 0.0], dtype=f32)
            between = (first + (last - first) * rng.random(500).astype(f32)).astype(f32)
            parts = [("edge", e), ("edge_below", below[1:]), ("edge_above", above[:-1]), ("first_last", np.array([first, last] * 3, dtype=f32)),
                     ("just_outside", outside), ("nan", np.full(3, np.nan, dtype=f32)), ("between", between)]
            wl = np.concatenate([p[1] for p in parts])
            cls = np.concatenate([np.full(p[1].shape[0], p[0], dtype=object) for p in parts])
            order = rng.permutation(wl.shape[0])
            cases.append(SpectrumCase(f"bins{nbins}-range{ri}", first, last, nbins, wl[order], cls[order]))
    return cases
