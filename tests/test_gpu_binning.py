"""Image and spectrum binning hit by hit, at its edges: `ot_render_accumulate` and `ot_render_accumulate_compact` on every route
(direct kernel, tile path, the library's own choice), the fused routes of `ot_detector_images` (`fuse_direct`, both tile kernels,
the multi-detector pass), automatic extents through compact hit lists and the one-pass form, `ot_spectrum_range`,
`ot_spectrum_histogram`, their compact forms and `LightSpectrum.render`, against the NumPy references of tests/binning_cases.py (the reference's rules operation by operation: misc.py:75-89,
np.interp on the CIE table, np.histogram's own counts).

Bounds (binning_cases.check_image): pixel and bin membership has no tolerance -- with unit or dyadic weights channel 3 and every
spectrum bin are equal bit for bit on every route; ordinary float32 weights: the lit masks are equal and channel 3 lies within
(k - 1) eps sum |w|; XYZ channels within (k + 3) eps sum (|d t| + |v|) |w| per pixel and channel, k the hits of the pixel and
v + d t the interpolation between two nodes of the observer table.  No hit is excluded: the generators place hits on the decision
points on purpose."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd._device import ptr, stream_ptr

import binning_cases as bc
from oracle import spectrum as ospec

pytestmark = pytest.mark.gpu

ROUTES = ["direct", "tiles", None]  # OT_RENDER_PATH; None: unset, the library decides


class render_path:
    def __init__(self, path):
        self.path = path

    def __enter__(self):
        self.old = os.environ.pop("OT_RENDER_PATH", None)
        if self.path:
            os.environ["OT_RENDER_PATH"] = self.path

    def __exit__(self, *a):
        os.environ.pop("OT_RENDER_PATH", None)
        if self.old is not None:
            os.environ["OT_RENDER_PATH"] = self.old


def dev(a, dtype):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to("cuda")


def accumulate_dense(h, Nx, Ny, extent, path):
    lib = _capi.load_library()
    hist = torch.zeros(Ny * Nx * 4, dtype=torch.float64, device="cuda")
    x, y, w, wl = dev(h.x, np.float64), dev(h.y, np.float64), dev(h.w, np.float32), dev(h.wl, np.float32)
    with render_path(path):
        _capi.check(lib.ot_render_accumulate(h.n, ptr(x), ptr(y), ptr(w), ptr(wl), (C.c_double * 4)(*extent), Nx, Ny, ptr(hist),
                                             stream_ptr()))
        torch.cuda.synchronize()
    return hist.cpu().numpy().reshape(Ny, Nx, 4)


def compact_lists(n, arrays, sentinels, seed):
    """The dense lists `arrays` as compact lists the way the detector stage hands them over: 1024 pieces of ot_hit_piece_len(n)
    entries, piece k filled at its front up to fill[k]; behind every fill count lies `sentinel` garbage that must not be read.
    -> (capacity, fill, device lists)"""
    lib = _capi.load_library()
    plen = int(lib.ot_hit_piece_len(n))
    assert plen >= 1024 and plen * bc.PIECES >= n
    fill, pos = bc.compact_layout(n, plen, np.random.default_rng(seed))
    cap = bc.PIECES * plen
    pos_d = dev(pos, np.int64)
    out = []
    for a, s in zip(arrays, sentinels):
        t = torch.full((cap,), s, dtype=torch.from_numpy(a[:0]).dtype, device="cuda")
        t[pos_d] = dev(a, a.dtype)
        out.append(t)
    return cap, dev(fill.astype(np.int32), np.int32), out


def accumulate_compact(h, Nx, Ny, extent, path):
    lib = _capi.load_library()
    # garbage behind the fill counts: a position in the middle of the image, weight 3, 555 nm -- it would be counted if read
    mid = (0.5 * (extent[0] + extent[1]), 0.5 * (extent[2] + extent[3]))
    cap, fill, (x, y, w, wl) = compact_lists(h.n, (h.x, h.y, h.w, h.wl), (mid[0], mid[1], 3.0, 555.0), seed=h.n)
    hist = torch.zeros(Ny * Nx * 4, dtype=torch.float64, device="cuda")
    with render_path(path):
        _capi.check(lib.ot_render_accumulate_compact(cap, ptr(fill), ptr(x), ptr(y), ptr(w), ptr(wl), (C.c_double * 4)(*extent),
                                                     Nx, Ny, ptr(hist), stream_ptr()))
        torch.cuda.synchronize()
    return hist.cpu().numpy().reshape(Ny, Nx, 4)


@functools.lru_cache(maxsize=8)
def reference_of(case):
    h = case.hits
    return bc.reference_image(h.x, h.y, h.w, h.wl, case.Nx, case.Ny, case.extent)


WORST = {}  # worst observed ratio of an XYZ error to its bound, per route (printed by the last test of this file)


def note(route, ratio):
    WORST[route] = max(WORST.get(route, 0.0), ratio)


def run_hit_list_case(case, routes=ROUTES, layouts=("dense", "compact")):
    ref = reference_of(case)
    for path in routes:
        for layout in layouts:
            fn = accumulate_dense if layout == "dense" else accumulate_compact
            got = fn(case.hits, case.Nx, case.Ny, case.extent, path)
            note(f"{layout} {path}", bc.check_image(got, ref, case.mode, what=f"{case.name} {layout} list, OT_RENDER_PATH={path}"))


# ---- 2. hit-list entries ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.edge_cases(), ids=repr)
def test_hit_list_edges(case):
    """Every decision point of the pixel rule (pixel boundaries and the extent's edges with their one-ulp neighbours, corners,
    -0.0, NaN, +-inf, +-1e300, scaled indices beyond int32), weights 0, -0.0, NaN, negative, subnormal and ordinary, every node of
    the observer table, its ends with their float32 neighbours, wavelengths outside and NaN: dense and compact lists through the
    direct kernel, the tile path and the library's own choice.  A NaN position adds nothing; a NaN wavelength makes X, Y, Z of its
    pixel NaN as np.interp does and leaves channel 3 alone."""
    run_hit_list_case(case)


@pytest.mark.parametrize("case", bc.count_cases(), ids=repr)
def test_hit_list_counts(case):
    """List lengths around a wave and a workgroup, several workgroups of the direct kernel, more than 16384 hits in one tile (two
    slabs of the tile accumulation), empty tiles between lit ones, hits in the last, partial tile only."""
    run_hit_list_case(case)


def test_accumulates_into_existing_image():
    """The entry ADDS to the image it is given: a second call on an image that holds 0.25 times the first result gives 1.25
    times it, bit for bit (dyadic weights), on both paths."""
    case = bc.count_cases()[7]  # several workgroups
    h = case.hits
    lib = _capi.load_library()
    want = reference_of(case)["w3"].astype(np.float64)
    for path in ("direct", "tiles"):
        first = accumulate_dense(h, case.Nx, case.Ny, case.extent, path)
        hist = dev(0.25 * first.reshape(-1), np.float64)
        x, y, w, wl = dev(h.x, np.float64), dev(h.y, np.float64), dev(h.w, np.float32), dev(h.wl, np.float32)
        with render_path(path):
            _capi.check(lib.ot_render_accumulate(h.n, ptr(x), ptr(y), ptr(w), ptr(wl), (C.c_double * 4)(*case.extent), case.Nx,
                                                 case.Ny, ptr(hist), stream_ptr()))
            torch.cuda.synchronize()
        assert np.array_equal(hist.cpu().numpy().reshape(-1, 4)[:, 3], 1.25 * want), path


def test_long_list_takes_the_probe():
    """Lists of 2^21 hits and more go through `tile_probe`: a spread list is binned by the tile path, a point-like one by the
    direct kernel -- the same counts either way, with the decision points of a 945 x 315 image dealt out over the list.
    Which route the probe chose cannot be observed through the entry: the lists are made for the rule as the source states it
    (more than 1024 distinct pixels among 4096 sampled hits: tiles); if that rule changes, the counts are still pinned, the
    branch named here possibly no longer."""
    case = next(c for c in bc.edge_cases() if c.name.startswith("945x315-asym"))
    n = (1 << 21) + 333
    rng = np.random.default_rng(77)
    e = case.extent
    for spread in (True, False):
        h = bc.Hits()
        take = rng.integers(0, case.hits.n, n)
        x, y = case.hits.x[take].copy(), case.hits.y[take].copy()
        some = rng.random(n) < (0.9 if spread else 0.0)   # spread: most hits anywhere in the image; point-like: edge hits of a few pixels
        x[some] = e[0] + (e[1] - e[0]) * (1.2 * rng.random(int(some.sum())) - 0.1)
        y[some] = e[2] + (e[3] - e[2]) * (1.2 * rng.random(int(some.sum())) - 0.1)
        if not spread:
            x, y = case.hits.x[take % 64].copy(), case.hits.y[take % 64].copy()
        h.add("probe", x, y).done()
        h.w = np.where(rng.random(n) < 0.1, 0, rng.integers(1, 9, n) / 8.0).astype(np.float32)
        pix = bc.pixel_index(h.x, h.y, case.Nx, case.Ny, case.extent)
        ok = (pix >= 0) & (h.w != 0)
        want = np.bincount(pix[ok], weights=h.w[ok].astype(np.float64), minlength=case.Nx * case.Ny)
        assert ok.sum() > n // 4 and (np.unique(pix[ok]).size > 4096) == spread
        got = accumulate_dense(h, case.Nx, case.Ny, case.extent, None)
        assert np.array_equal(got[..., 3].reshape(-1), want), f"spread={spread}"


# ---- 3. waves composed on purpose -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", bc.wave_cases(), ids=repr)
def test_composed_waves(case):
    """wave_add4_by_key on waves made for it (groups of 64 consecutive list entries from a multiple of 1024 are the waves of the
    direct kernel): one pixel for all lanes; 7, 8 and 9 lanes sharing a pixel among singletons; four keys of at least eight lanes
    (the fourth is added lane by lane); eight pixels of eight lanes; lane 63 a singleton while it delivers other keys' sums; lane
    63 in the first key; lanes that add nothing in between; a last wave of 1 and of 63 lanes.  And the LDS hash of render_kernel:
    nine pixel ids with one slot from one workgroup (the fifth and later go to global atomics)."""
    run_hit_list_case(case)


def test_hash_table_overflow():
    """More than 2048 distinct pixels from every workgroup of the direct kernel: what finds no place in the LDS table of 2048
    entries goes to global atomics.  The grid of the direct kernel (one workgroup per compute unit, here 3072 consecutive
    hits each) is the source's rule, not something the entry reports: with another grid the counts stay pinned, the overflow
    possibly not exercised."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    case = bc.hash_overflow_case(cus)
    h = case.hits
    pix = bc.pixel_index(h.x, h.y, case.Nx, case.Ny, case.extent)
    assert np.all(pix >= 0)
    want = np.bincount(pix, minlength=case.Nx * case.Ny).astype(np.float64)
    # the list is cut into one contiguous piece of 3072 hits per workgroup
    assert all(np.unique(row).size > 2048 for row in pix.reshape(cus, 3072)[[0, cus // 2, cus - 1]])
    for path in ("direct", "tiles"):
        got = accumulate_dense(h, case.Nx, case.Ny, case.extent, path)
        assert np.array_equal(got[..., 3].reshape(-1), want), path


# ---- 5. spectrum ------------------------------------------------------------------------------------------------------------
def spectrum_range(wl, w, fill=None, n=None):
    lib = _capi.load_library()
    rng = torch.full((2,), 123.0, dtype=torch.float64, device="cuda")
    cnt = torch.full((1,), -5, dtype=torch.int64, device="cuda")
    n = int(wl.shape[0]) if n is None else n
    if fill is None:
        _capi.check(lib.ot_spectrum_range(n, ptr(wl), ptr(w), ptr(rng), ptr(cnt), stream_ptr()))
    else:
        _capi.check(lib.ot_spectrum_range_compact(n, ptr(fill), ptr(wl), ptr(w), ptr(rng), ptr(cnt), stream_ptr()))
    torch.cuda.synchronize()
    return rng.cpu().numpy(), int(cnt.item())


def range_grid_cap():
    """rays one launch of spectrum_stats_kernel covers without a second round: cu_count * 8 workgroups of 256"""
    return torch.cuda.get_device_properties(0).multi_processor_count * 8 * 256


@pytest.mark.parametrize("n", [1, 255, 256, 257, "cap"])
def test_spectrum_range(n):
    """Range and count of the selected rays: rays of weight 0 hold the extreme wavelengths and are ignored; with all weights zero
    the count is 0 and the +-inf presets stay; the count is exact around a workgroup and above the grid cap."""
    n = range_grid_cap() + 77 if n == "cap" else n
    rng = np.random.default_rng(n)
    wl = (400 + 300 * rng.random(n)).astype(np.float32)
    w = np.ones(n, dtype=np.float32)
    off = rng.random(n) < 0.3
    off[rng.integers(0, n)] = False
    w[off] = 0
    wl[off] = np.where(rng.random(int(off.sum())) < 0.5, 200.0, 900.0)  # the extremes belong to rays that are not selected
    if n > 2:
        w[0], wl[0], w[n - 1], wl[n - 1] = 0, 100.0, 0, 1000.0
    sel = w > 0
    for layout in ("dense", "compact"):
        if layout == "dense":
            got, cnt = spectrum_range(dev(wl, np.float32), dev(w, np.float32))
        else:
            cap, fill, (wl_c, w_c) = compact_lists(n, (wl, w), (50.0, 2.0), seed=n)  # garbage: 50 nm with weight 2
            got, cnt = spectrum_range(wl_c, w_c, fill, cap)
        assert cnt == int(sel.sum()), layout
        assert got[0] == float(wl[sel].min()) and got[1] == float(wl[sel].max()), layout
        # nothing selected
        zero = torch.zeros(n, dtype=torch.float32, device="cuda")
        if layout == "dense":
            got, cnt = spectrum_range(dev(wl, np.float32), zero)
        else:
            got, cnt = spectrum_range(wl_c, torch.zeros_like(w_c), fill, cap)
        assert cnt == 0 and got[0] == np.inf and got[1] == -np.inf, layout


def spectrum_histogram(case, layout):
    lib = _capi.load_library()
    n = case.wl.shape[0]
    w = np.ones(n, dtype=np.float32)
    edges = dev(case.edges, np.float32)
    hist = torch.zeros(case.nbins, dtype=torch.float64, device="cuda")
    if layout == "dense":
        wl_d, w_d = dev(case.wl, np.float32), dev(w, np.float32)
        _capi.check(lib.ot_spectrum_histogram(n, ptr(wl_d), ptr(w_d), ptr(edges), case.nbins, ptr(hist), stream_ptr()))
    else:
        mid = float(case.edges[case.nbins // 2])
        cap, fill, (wl_d, w_d) = compact_lists(n, (case.wl, w), (mid, 2.0), seed=n)
        _capi.check(lib.ot_spectrum_histogram_compact(cap, ptr(fill), ptr(wl_d), ptr(w_d), ptr(edges), case.nbins, ptr(hist),
                                                      stream_ptr()))
    torch.cuda.synchronize()
    return hist.cpu().numpy()


@pytest.mark.parametrize("layout", ["dense", "compact"])
@pytest.mark.parametrize("case", bc.spectrum_cases(), ids=repr)
def test_spectrum_histogram_on_every_edge(case, layout):
    """A wavelength on every float32 edge and one float32 ulp on both sides of it, on `first` and `last` and just outside, NaN:
    the bins hold NumPy's own counts.  1, 2, 51 and 1001 bins are privatised in LDS; 6001 bins need 72 KB, more than `hist_shape`
    (csrc/ot_host.hpp:76-79) grants, and take the kernel's global-atomics form by that rule.  Which form a call took cannot be
    observed through the C interface: the 6001-bin case pins the RESULT at that size, not the form (binning_cases.HIST_LDS_LIMIT
    is a copy of the source's constant)."""
    want = bc.spectrum_counts(case.wl, case.first, case.last, case.nbins)
    got = spectrum_histogram(case, layout)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bins differ, first {bad[:5]}: got {got[bad[:5]]} want {want[bad[:5]]}"


def test_spectrum_histogram_accumulates_and_drops_unselected():
    """Rays of weight 0, -0.0 and NaN are not selected whatever their wavelength; dyadic weights sum exactly per bin."""
    case = bc.spectrum_cases()[4]  # 51 bins
    n = case.wl.shape[0]
    rng = np.random.default_rng(9)
    w = (rng.integers(1, 4097, n) / 1024.0).astype(np.float32)
    w[::5], w[1::7], w[2::11] = 0.0, -0.0, np.nan
    lib = _capi.load_library()
    hist = torch.zeros(case.nbins, dtype=torch.float64, device="cuda")
    wl_d, w_d, edges = dev(case.wl, np.float32), dev(w, np.float32), dev(case.edges, np.float32)
    _capi.check(lib.ot_spectrum_histogram(n, ptr(wl_d), ptr(w_d), ptr(edges), case.nbins, ptr(hist), stream_ptr()))
    torch.cuda.synchronize()
    sel = w > 0
    with np.errstate(invalid="ignore"):
        want, _ = np.histogram(case.wl[sel], bins=case.nbins, range=(case.first, case.last), weights=w[sel].astype(np.float64))
    assert np.array_equal(hist.cpu().numpy(), want)


@pytest.mark.parametrize("wl0,want", [(550.0, (549.0, 551.0)), (380.25, (380.0, 381.25)), (779.5, (778.5, 780.0))])
def test_spectrum_render_equal_wavelengths(wl0, want):
    """All wavelengths equal: the range is widened by +-1 nm and clipped at the visible range on both ends."""
    n = 300
    wl = np.full(n, wl0, dtype=np.float32)
    w = np.ones(n, dtype=np.float32)
    w[::9] = 0
    spec = ot.LightSpectrum.render(wl, w)
    edges, vals = ospec.render(wl[w > 0], w[w > 0])
    assert spec._wls[0] == np.float32(want[0]) and spec._wls[-1] == np.float32(want[1])
    assert spec._wls.shape[0] == 52 and np.array_equal(spec._wls.astype(np.float64), edges)
    counts = bc.spectrum_counts(wl[w > 0], want[0], want[1], 51)
    assert counts.sum() == int((w > 0).sum())
    width = np.float64(spec._wls[1]) - np.float64(spec._wls[0])
    assert np.array_equal(np.rint(spec._vals * width), counts)
    np.testing.assert_allclose(spec._vals, vals, rtol=1e-6, atol=0)


@pytest.mark.parametrize("nz,bins", [(2, 51), (10404, 51), (10815, 51), (10816, 53), (11235, 53), (11664, 55), (12100, 55)])
def test_spectrum_render_bin_count_rule(nz, bins):
    """At least 51 bins, sqrt(N) / 2 above that, made odd -- N the rays with a weight, not the length of the list."""
    rng = np.random.default_rng(nz)
    n = nz + 500
    wl = (420 + 250 * rng.random(n)).astype(np.float32)
    w = np.ones(n, dtype=np.float32)
    w[rng.permutation(n)[:500]] = 0
    spec = ot.LightSpectrum.render(wl, w)
    assert spec._vals.shape[0] == bins and spec._wls.shape[0] == bins + 1
    sel = w > 0
    first, last = wl[sel].min(), wl[sel].max()
    assert last - first >= 1  # (no widening of the range here)
    assert spec._wls[0] == first and spec._wls[-1] == last
    counts = bc.spectrum_counts(wl[sel], first, last, bins)
    width = np.float64(spec._wls[1]) - np.float64(spec._wls[0])
    assert np.array_equal(np.rint(spec._vals * width), counts)


# ---- 4. fused routes and automatic extents ----------------------------------------------------------------------------------
# Rays that reach a flat detector unchanged: direction (0, 0, 1), weight exactly 1.0f, no surface in between, so a hit's x and y
# are the ray's.  The truth of every route is the NumPy pixel rule applied to the positions, weights and wavelengths that the
# hit-list route (`ot_detector_hits`, pinned by tests/test_gpu_detectors.py) returns for the same rays.
from test_gpu_parity_paths import forced, spy_one_pass  # noqa: E402

HALF = 1100.0  # the detector reaches +-HALF: every extent of binning_cases.EXTENTS lies on it
FUSED_EXTENTS = dict(bc.EXTENTS, tall=[-2.0, -1.3, -1.0, 1.3])  # 945 x 945, 2835 x 945 and (tall) 945 x 2835 pixels


def flat_scene():
    RT = ot.Raytracer(outline=[-HALF - 100, HALF + 100, -HALF - 100, HALF + 100, -1, 12], no_pol=True)
    RT.add(ot.RaySource(ot.RectangularSurface(dim=[8, 8]), divergence="None", s=[0, 0, 1], pos=[0, 0, 0]))
    RT.add(ot.Detector(ot.RectangularSurface(dim=[2 * HALF, 2 * HALF]), pos=[0, 0, 6]))
    return RT


def image_grid(extent):
    """(image extent, Nx, Ny) of a detector image with this extent: RenderImage's own rule"""
    img, Nx, Ny = ot.RenderImage.on_grid(np.array(extent, dtype=np.float64), None, "", None)
    return [float(v) for v in img.extent], Nx, Ny


def fused_rays(extents, seed, inside_only=False, n_nan_wl=0):
    """Ray positions for images of `extents`: for the grid of the first extent the wave compositions of section 3 (whole groups of
    64 from the start of the list, lanes that add nothing lie outside the extent) with its corners in front of them, then for
    every extent the finite decision points of its grid (binning_cases.edge_hits) that lie on the detector.
    `inside_only`: only positions inside the first extent, so that the hits' own extent is that extent.  -> (x, y, wl)"""
    rng = np.random.default_rng(seed)
    xs, ys = [], []
    e, Nx, Ny = image_grid(extents[0])
    cx, cy = np.meshgrid([e[0], e[1]], [e[2], e[3]])
    lanes = np.full(64, -1, dtype=np.int64)
    lanes[4:] = rng.integers(0, Nx * Ny, 60)
    x, y = bc._pixel_centres(np.maximum(lanes, 0), Nx, Ny, e)
    x[:4], y[:4] = cx.ravel(), cy.ravel()  # the first wave: the four corners and 60 singletons
    xs.append(x)
    ys.append(y)
    for _, lanes in bc.wave_groups(rng, Nx * Ny):
        x, y = bc._pixel_centres(np.maximum(lanes, 0), Nx, Ny, e)
        off = lanes < 0
        if inside_only:  # (no lane may lie outside: it shares the pixel of its neighbour instead)
            x[off], y[off] = x[~off][0], y[~off][0]
        else:
            x[off] = e[1] + (e[1] - e[0])
        xs.append(x)
        ys.append(y)
    for ext in extents:
        e, Nx, Ny = image_grid(ext)
        h = bc.edge_hits(Nx, Ny, e, rng, n_interior=300)
        keep = np.isfinite(h.x) & np.isfinite(h.y) & (np.abs(h.x) < HALF - 1) & (np.abs(h.y) < HALF - 1)
        xs.append(h.x[keep])
        ys.append(h.y[keep])
    x, y = np.concatenate(xs), np.concatenate(ys)
    if inside_only:
        e = image_grid(extents[0])[0]
        keep = (x >= e[0]) & (x <= e[1]) & (y >= e[2]) & (y <= e[3])
        x, y = x[keep], y[keep]
    pool, _ = bc.wavelength_pool(rng)
    pool = pool[np.isfinite(pool) & (pool > 50)]
    wl = pool[rng.permutation(x.shape[0]) % pool.shape[0]].astype(np.float32)
    if n_nan_wl:
        wl[rng.choice(np.arange(64, x.shape[0]), n_nan_wl, replace=False)] = np.nan
    return x, y, wl


@functools.lru_cache(maxsize=2)
def traced(key, inside_only=False, n_nan_wl=0):
    """(RT with the rays traced, truth lists x, y, w, wl from the hit-list route); key: names of FUSED_EXTENTS"""
    x, y, wl = fused_rays([FUSED_EXTENTS[k] for k in key], seed=len(key) + 11 * len(key[0]), inside_only=inside_only,
                          n_nan_wl=n_nan_wl)
    n = x.shape[0]
    p0 = np.stack([x, y, np.zeros(n)], axis=1)
    s0 = np.tile([0.0, 0.0, 1.0], (n, 1))
    RT = flat_scene()
    with ot.global_options.no_warnings():
        RT.trace(n, _initial_rays=(p0, s0, None, np.ones(n, dtype=np.float32), wl), _N_list=np.array([n]))
        hits = RT._hit_detectors([dict(detector_index=0, source_index=None, extent=None, projection_method=None)])[0]
    assert not RT.geometry_error
    ph = hits.xy.cpu().numpy()
    hx, hy, hw, hwl = ph[:n], ph[n:2 * n], hits.w.cpu().numpy(), hits.wl.cpu().numpy()
    assert np.array_equal(hx, x) and np.array_equal(hy, y), "the rays reach the detector unchanged"
    assert np.all(hw == 1.0) and np.array_equal(hwl, wl, equal_nan=True)
    return RT, (hx, hy, hw, hwl)


def check_fused(img, truth, extent, route, user_extent=True):
    """`user_extent`: the hits outside the extent asked for are dropped first, as the reference does (raytracer.py:1036-1040),
    then the rest is binned on the image's extent -- the two differ for the 1e-9 wide extent, which RenderImage widens by 1e-9
    on every side as a point-like image (render_image.py:224-255)."""
    e, Nx, Ny = image_grid(extent)
    assert img._data.shape == (Ny, Nx, 4) and np.array_equal(np.asarray(img.extent, dtype=np.float64), e), route
    if user_extent:
        x, y, w, wl = truth
        inside = (extent[0] <= x) & (x <= extent[1]) & (extent[2] <= y) & (y <= extent[3])
        truth = (x, y, np.where(inside, w, 0).astype(np.float32), wl)
    ref = bc.reference_image(*truth, Nx, Ny, e, sparse=True)
    assert ref["k"].sum() > 1000
    note(route, bc.check_image(img._data, ref, "unit", what=f"{route}, extent {extent}"))


FUSED_ROUTES = [("direct", "1"), ("tiles", "1"), ("tiles", "0")]


@pytest.mark.parametrize("path,linebuf", FUSED_ROUTES, ids=["fuse_direct", "fuse_tiles_lb", "fuse_tiles"])
@pytest.mark.parametrize("name", list(FUSED_EXTENTS))
def test_fused_user_extent(name, path, linebuf):
    """`ot_detector_images` with a user extent: hit search and binning in one pass by the LDS-hash kernel (the composed waves of
    section 3 in its first waves), the line-buffer tile kernel and the plain tile kernel, rays on every pixel boundary, edge and
    corner of the image's grid with their one-ulp neighbours."""
    RT, truth = traced((name,))
    with forced(render_path=path, linebuf=linebuf), ot.global_options.no_warnings():
        img = RT.detector_image(extent=FUSED_EXTENTS[name], projection_method=None)
    check_fused(img, truth, FUSED_EXTENTS[name], f"fused {path} linebuf={linebuf}")


@pytest.mark.parametrize("path,linebuf", FUSED_ROUTES, ids=["fuse_direct", "fuse_tiles_lb", "fuse_tiles"])
def test_fused_nan_wavelength(path, linebuf):
    """Rays with a NaN wavelength reach the fused kernels: X, Y, Z of their pixels are NaN, channel 3 counts them."""
    RT, truth = traced(("asym",), n_nan_wl=5)
    assert np.isnan(truth[3]).sum() == 5
    with forced(render_path=path, linebuf=linebuf), ot.global_options.no_warnings():
        img = RT.detector_image(extent=FUSED_EXTENTS["asym"], projection_method=None)
    assert np.isnan(img._data[..., :3]).any(axis=2).sum() >= 1
    check_fused(img, truth, FUSED_EXTENTS["asym"], f"fused {path} linebuf={linebuf} NaN wavelength")


@pytest.mark.parametrize("path", ["tiles", "direct"])
@pytest.mark.parametrize("K", [2, 3, 6])
def test_fused_multi_detector(K, path):
    """K images of different extents and shapes in one call: the multi-detector tile pass `fuse_tiles_kernel<2 | 4 | 8, 1>` with
    its `*_multi_kernel` second pass, and `fuse_direct_kernel<2 | 4 | 8>`; every image against the rule on the same hits."""
    names = ("unit", "asym", "tall", "zero_edge", "tiny", "far")[:K]
    RT, truth = traced(names)
    specs = [dict(detector_index=0, source_index=None, extent=FUSED_EXTENTS[k], projection_method=None) for k in names]
    with forced(render_path=path), ot.global_options.no_warnings():
        imgs = RT._render_detectors(specs, [None] * K)
    assert len(imgs) == K
    for k, img in zip(names, imgs):
        check_fused(img, truth, FUSED_EXTENTS[k], f"multi {path} K={K}")


@pytest.mark.parametrize("path", ["direct", "tiles"])
@pytest.mark.parametrize("name", ["unit", "asym", "tall"])
def test_auto_extent_compact_hit_lists(name, path):
    """Automatic extent through compact hit lists (`ot_detector_req.fill`) binned by the direct kernel and the tile path: the rays
    lie inside the extent with its corners among them, so the hits' own extent is that extent and its grid the one they sit on."""
    RT, truth = traced((name,), inside_only=True)
    with forced(one_pass=1 << 60, compact=1, render_path=path), ot.global_options.no_warnings():
        img = RT.detector_image(projection_method=None)
    check_fused(img, truth, FUSED_EXTENTS[name], f"auto compact {path}", user_extent=False)


@pytest.mark.parametrize("linebuf", ["1", "0"], ids=["line buffers", "plain tile kernel"])
def test_auto_extent_one_pass(linebuf):
    """`_auto_image_one_pass` (`spec_*`): sample extent, provisional tile grid, records, exact binning.  The sample is every 128th
    wave of the list; the first wave holds the four corners, so the sample's extent is the final one.  Where the form declines,
    it must have said so (the image is then the chain's) -- and it applies to at least one of the extents."""
    applied = []
    for name in ("unit", "asym", "tall"):
        RT, truth = traced((name,), inside_only=True)
        calls = spy_one_pass(RT)
        try:
            with forced(one_pass=1, linebuf=linebuf), ot.global_options.no_warnings():
                img = RT.detector_image(projection_method=None)
        finally:
            del RT._auto_image_one_pass
        assert len(calls) == 1
        applied.append(calls[0])
        check_fused(img, truth, FUSED_EXTENTS[name], f"one pass linebuf={linebuf} applied={calls[0]}", user_extent=False)
    print("one-pass form applied:", dict(zip(("unit", "asym", "tall"), applied)))
    assert any(applied)


def test_worst_xyz_ratio_report():
    """(last in the file) the worst observed ratio of an XYZ error to its bound on every route that ran, for DESIGN.md"""
    for route, ratio in sorted(WORST.items()):
        print(f"worst XYZ error / bound, {route}: {ratio:.3f}")
    assert all(r <= 1.0 for r in WORST.values())
