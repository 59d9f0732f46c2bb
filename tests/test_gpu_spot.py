"""Raytracer.spot_analysis and the `ot_spot_*` entry points on the GPU.

Truth is NumPy in float64 following the definitions of `ot.SpotAnalysis`: on the reference's recorded detector hits
(tests/golden/trace_*.npz) for rays injected into the device trace, on the device's own hit list, and on synthetic lists.
"""
import functools

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd._device import ptr, stream_ptr

import scenes
from helpers import load, assert_close

pytestmark = pytest.mark.gpu

FIXTURES = ["c1_single_lens", "double_gauss", "hurb_ring_ideal", "prism"]
EPS_W = 2e-7  # what test_trace_matches_reference grants the float32 weights of these scenes
EPS = np.finfo(np.float64).eps


@functools.lru_cache(maxsize=None)
def traced(name):
    """(fixture, Raytracer with the fixture's rays traced on the device, as test_gpu_parity.py::gpu_trace injects them), once per
    scene: the analyses change nothing."""
    g = load(f"trace_{name}.npz")
    with ot.global_options.no_warnings():
        RT = {**scenes.SCENES, **scenes.SCENES2}[name][0](ot)
        hn = g["hurb_normals"] if "hurb_normals" in g else None
        RT.trace(int(g["N"]), _initial_rays=(g["p0"], g["s0"], g["pol0"], g["w0"], g["wl"]), _hurb_normals=hn, _N_list=g["N_list"])
    assert not RT.geometry_error
    return g, RT


def numpy_spot(x, y, w, freq):
    """The definitions in float64.  -> dict of the figures, the per-hit radii and weights, and sums of |terms|."""
    sel = w > 0
    x, y, w = x[sel].astype(np.float64), y[sel].astype(np.float64), w[sel].astype(np.float64)
    t = dict(N=int(w.shape[0]), power=w.sum())
    W = t["power"]
    if not W > 0:
        return t
    t["centroid"] = np.array([(w * x).sum() / W, (w * y).sum() / W])
    dx, dy = x - t["centroid"][0], y - t["centroid"][1]
    t["rms_x"], t["rms_y"] = np.sqrt((w * dx * dx).sum() / W), np.sqrt((w * dy * dy).sum() / W)
    t["rms_radius"] = np.sqrt(t["rms_x"] ** 2 + t["rms_y"] ** 2)
    t["cov_xy"] = (w * dx * dy).sum() / W
    t["r"], t["w"] = np.sqrt(dx * dx + dy * dy), w
    t["max_radius"] = t["r"].max()
    freq = np.asarray(freq, dtype=np.float64)
    t["otf_x"] = (w * np.exp(-2j * np.pi * freq[:, None] * dx)).sum(axis=1) / W
    t["otf_y"] = (w * np.exp(-2j * np.pi * freq[:, None] * dy)).sum(axis=1) / W
    # sums of |terms| over W: what the rounding of a sum is measured against
    t["abs_c"] = np.array([(w * np.abs(x)).sum() / W, (w * np.abs(y)).sum() / W])
    t["abs_cov"] = (w * np.abs(dx * dy)).sum() / W
    return t


def ee_by_bin_rule(t, n_radii):
    r, rmax = t["r"], t["max_radius"]
    idx = np.zeros(r.shape, dtype=np.int64) if rmax == 0 else np.minimum(np.floor(r / rmax * n_radii).astype(np.int64), n_radii - 1)
    cum = np.concatenate(([0.0], np.cumsum(np.bincount(idx, weights=t["w"], minlength=n_radii))))
    return cum / cum[-1]


def ee_bounds(t, n_radii, tau):
    """Per interior edge the power fraction strictly inside by more than tau and the one inside or within tau: a hit within tau of
    an edge may fall on either side."""
    W, r, w = t["power"], t["r"], t["w"]
    edges = np.linspace(0, t["max_radius"], n_radii + 1)[1:-1]
    order = np.argsort(r)
    rs, cw = r[order], np.concatenate(([0.0], np.cumsum(w[order])))
    lo = cw[np.searchsorted(rs, edges - tau, side="left")] / W
    hi = cw[np.searchsorted(rs, edges + tau, side="right")] / W
    return lo, hi


def check_empty(sa, n_radii, K):
    assert sa.N == 0 and sa.power == 0
    for v in (sa.centroid, sa.rms_x, sa.rms_y, sa.rms_radius, sa.cov_xy, sa.max_radius, sa.otf_x, sa.otf_y, sa.mtf_x, sa.mtf_y):
        assert np.all(np.isnan(v))
    assert sa.otf_x.shape == sa.otf_y.shape == sa.mtf_x.shape == (K,)
    assert np.array_equal(sa.ee, np.zeros(n_radii + 1))


def check_result_shape(sa, n_radii, freq):
    assert isinstance(sa, ot.SpotAnalysis)
    assert isinstance(sa.N, int) and isinstance(sa.power, float) and isinstance(sa.rms_radius, float)
    assert sa.centroid.shape == (2,) and sa.extent.shape == (4,)
    assert sa.ee.shape == sa.ee_radii.shape == (n_radii + 1,)
    assert np.array_equal(sa.frequencies, freq)
    assert sa.otf_x.dtype == sa.otf_y.dtype == np.complex128 and sa.otf_x.shape == sa.otf_y.shape == (len(freq),)
    assert np.array_equal(sa.mtf_x, np.abs(sa.otf_x)) and np.array_equal(sa.mtf_y, np.abs(sa.otf_y))
    for arr in (sa.centroid, sa.ee, sa.ee_radii, sa.otf_x, sa.mtf_y, sa.frequencies, sa.extent):
        assert not arr.flags.writeable
    with pytest.raises(RuntimeError):
        sa.N = 1


def against_reference(name, crop):
    """Cases 1 and 2: the reference's hits (restricted to `crop` with closed bounds, the rule of `_hit_detectors`) against
    the device's analysis of the same injected rays.  Tolerances from what the parity tests grant the inputs."""
    g, RT = traced(name)
    ph, w = g["det0/None/ph"], g["det0/None/w"]
    x, y = ph[:, 0], ph[:, 1]
    dp = 1e-11 * (1 + np.abs(ph[:, :2]).max())
    if crop is not None:
        # (a hit within rounding of the crop may be kept on one side and dropped on the other: none is, so N is exact)
        assert min(np.abs(x - crop[0]).min(), np.abs(x - crop[1]).min(), np.abs(y - crop[2]).min(), np.abs(y - crop[3]).min()) > 1e-9
        keep = (x >= crop[0]) & (x <= crop[1]) & (y >= crop[2]) & (y <= crop[3])
        x, y, w = x[keep], y[keep], w[keep]
    pre = numpy_spot(x, y, w, [0.0])
    n_radii = 32
    freq = np.linspace(0, 1 / pre["rms_radius"], 17) if pre["N"] else np.linspace(0, 1, 17)
    t = numpy_spot(x, y, w, freq)
    with ot.global_options.no_warnings():
        sa = RT.spot_analysis(0, None, None if crop is None else list(crop), n_radii=n_radii, frequencies=freq)
    print(name, "N", sa.N, "power", sa.power, "centroid", sa.centroid, "rms", sa.rms_x, sa.rms_y, sa.rms_radius, "max", sa.max_radius)
    if not t["N"]:
        check_empty(sa, n_radii, 17)
        return
    check_result_shape(sa, n_radii, freq)
    rmax = t["max_radius"]
    assert sa.N == t["N"]
    assert_close(sa.power, t["power"], rtol=2 * EPS_W, what="power")
    assert_close(sa.centroid, t["centroid"], rtol=0, atol=dp + 2 * EPS_W * rmax, what="centroid")
    for key in ("rms_x", "rms_y", "rms_radius", "max_radius"):
        assert_close(getattr(sa, key), t[key], rtol=0, atol=2 * dp + 2 * EPS_W * rmax, what=key)
    tol = 4 * EPS_W + 4 * np.pi * freq.max() * dp
    for key in ("otf_x", "otf_y"):
        got = getattr(sa, key)
        print(key, "max error", np.abs(got - t[key]).max(), "tol", tol)
        assert_close(got.real, t[key].real, rtol=0, atol=tol, what=key + " real")
        assert_close(got.imag, t[key].imag, rtol=0, atol=tol, what=key + " imag")
    if crop is None:
        assert_close(sa.extent, g["det0/None/extent"], rtol=1e-9, atol=1e-11, what="extent")
    else:
        assert np.array_equal(sa.extent, crop)
    assert sa.ee[0] == 0 and sa.ee[-1] == 1 and np.all(np.diff(sa.ee) >= 0)
    assert_close(sa.ee_radii, np.linspace(0, sa.max_radius, n_radii + 1), rtol=0, what="ee_radii")
    lo, hi = ee_bounds(t, n_radii, 4 * dp)
    assert np.all(lo - 2 * EPS_W <= sa.ee[1:-1]) and np.all(sa.ee[1:-1] <= hi + 2 * EPS_W), (lo, sa.ee, hi)
    return t


@pytest.mark.parametrize("name", FIXTURES)
def test_matches_reference_hits(name):
    t = against_reference(name, None)
    # the prototype's figures for these fixtures
    proto = {"c1_single_lens": (2000, 1.0377), "double_gauss": (1083, 12.043), "hurb_ring_ideal": (1868, 0.06741), "prism": (2000, 0.15536)}
    assert t["N"] == proto[name][0] and abs(t["rms_radius"] / proto[name][1] - 1) < 1e-4
    # no reference hit within 1e-9 max(1, rmax) of an interior edge: both bounds of the encircled energy coincide
    lo, hi = ee_bounds(t, 32, 1e-9 * max(1.0, t["max_radius"]))
    assert np.array_equal(lo, hi)


@pytest.mark.parametrize("name", FIXTURES)
def test_user_extent(name):
    against_reference(name, traced(name)[0]["det0/user/uext"])


def against_own_hits(RT, n_radii=32, **kwargs):
    """Case 3's yardstick: NumPy on the hit list `_hit_detector` leaves (pinned by tests/test_gpu_detectors.py).  A sum of n
    terms t folded as a tree is off by at most log2(n) eps sum|t| (2e-15 sum|t| for these sizes); 1e-13 sum|t| grants 50 times that.
    Quotients of two such sums get both shares.  The truth's centroid differs from the device's by up to the tolerance dc of
    the centroid: that shifts every radius by |dc| and every phase by 2 pi nu dc; second moments feel it in second order only."""
    with ot.global_options.no_warnings():
        ph, hw, _, ext, _, _ = RT._hit_detector("x", kwargs.get("detector_index", 0), kwargs.get("source_index"),
                                                kwargs.get("extent"), kwargs.get("projection_method", "Equidistant"))
        n = hw.shape[0]
        ph_h, w_h = ph.cpu().numpy().reshape(3, n), hw.cpu().numpy()
        pre = numpy_spot(ph_h[0], ph_h[1], w_h, [0.0])
        freq = np.linspace(0, 1 / pre["rms_radius"], 17)
        sa = RT.spot_analysis(n_radii=n_radii, frequencies=freq, **kwargs)
    t = numpy_spot(ph_h[0], ph_h[1], w_h, freq)
    check_result_shape(sa, n_radii, freq)
    assert sa.N == t["N"] and t["N"] > 1
    assert_close(sa.power, t["power"], rtol=1e-13, what="power")
    dc = 2e-13 * t["abs_c"]
    for k in range(2):
        assert_close(sa.centroid[k], t["centroid"][k], rtol=0, atol=dc[k], what="centroid")
    for key in ("rms_x", "rms_y", "rms_radius"):  # (a root halves the relative error of its two sums)
        assert_close(getattr(sa, key), t[key], rtol=1e-13, what=key)
    assert_close(sa.cov_xy, t["cov_xy"], rtol=0, atol=2e-13 * t["abs_cov"], what="cov_xy")
    assert_close(sa.max_radius, t["max_radius"], rtol=4 * EPS, atol=dc.sum(), what="max_radius")
    for key, d in (("otf_x", dc[0]), ("otf_y", dc[1])):  # |terms| sum to W at most: 1e-13 for the sum, 1e-13 for W
        tol = 2e-13 + 2 * np.pi * freq.max() * d
        got = getattr(sa, key)
        assert_close(got.real, t[key].real, rtol=0, atol=tol, what=key + " real")
        assert_close(got.imag, t[key].imag, rtol=0, atol=tol, what=key + " imag")
    assert_close(sa.ee, ee_by_bin_rule(t, n_radii), rtol=0, atol=1e-12, what="ee")
    assert np.array_equal(sa.extent, ext)
    return sa


@pytest.mark.parametrize("name", FIXTURES)
def test_arithmetic_against_own_hit_list(name):
    g, RT = traced(name)
    against_own_hits(RT)
    if name != "prism":  # (its user extent holds no hit)
        against_own_hits(RT, extent=list(g["det0/user/uext"]))


def test_source_selection():
    g, RT = traced("double_gauss")
    assert len(g["N_list"]) == 5
    with ot.global_options.no_warnings():
        whole = RT.spot_analysis(frequencies=[])
    parts = [against_own_hits(RT, source_index=k) for k in range(5)]
    assert sum(p.N for p in parts) == whole.N
    assert_close(sum(p.power for p in parts), whole.power, rtol=1e-13, what="power of the five sources")
    assert all("RS%d" % k in p.long_desc for k, p in enumerate(parts))


def test_compact_list(monkeypatch):
    """The list of the valid hits alone (long bundles) against the dense one: the same hits in another order.  1e-13 relative to
    each field's own scale (|OTF| <= 1, positions: the spot's radius and the centroid's distance from the origin)."""
    g, RT = traced("double_gauss")
    freq = np.linspace(0, 0.2, 17)
    with ot.global_options.no_warnings():
        monkeypatch.setattr(ot.Raytracer, "COMPACT_HITS_FROM", 1 << 60)
        dense = RT.spot_analysis(n_radii=32, frequencies=freq)
        monkeypatch.setattr(ot.Raytracer, "COMPACT_HITS_FROM", 1)
        compact = RT.spot_analysis(n_radii=32, frequencies=freq)
        part = RT.spot_analysis(n_radii=32, frequencies=freq, source_index=3)
        monkeypatch.setattr(ot.Raytracer, "COMPACT_HITS_FROM", 1 << 60)
        part_dense = RT.spot_analysis(n_radii=32, frequencies=freq, source_index=3)
    for a, b in ((compact, dense), (part, part_dense)):
        assert a.N == b.N > 0
        scale = b.max_radius + np.abs(b.centroid).max()
        for key in ("power", "rms_x", "rms_y", "rms_radius", "max_radius", "centroid", "extent", "ee_radii"):
            assert_close(getattr(a, key), getattr(b, key), rtol=1e-13, atol=1e-13 * scale, what=key)
        assert_close(a.cov_xy, b.cov_xy, rtol=1e-13, atol=1e-13 * scale ** 2, what="cov_xy")
        for key in ("ee", "mtf_x", "mtf_y"):
            assert_close(getattr(a, key), getattr(b, key), rtol=1e-13, atol=1e-13, what=key)
        for key in ("otf_x", "otf_y"):
            assert np.abs(getattr(a, key) - getattr(b, key)).max() <= 1e-13, key


def test_reproducible():
    _, RT = traced("double_gauss")
    with ot.global_options.no_warnings():
        a, b = RT.spot_analysis(), RT.spot_analysis()
    assert a.frequencies.shape == (65,) and a.frequencies[-1] == 1 / a.rms_radius
    for key in ("power", "centroid", "rms_x", "rms_y", "rms_radius", "cov_xy", "max_radius", "otf_x", "otf_y"):
        va, vb = np.asarray(getattr(a, key)), np.asarray(getattr(b, key))
        assert va.tobytes() == vb.tobytes(), key


def test_projected_spherical_detector():
    with ot.global_options.no_warnings():
        RT = ot.Raytracer(outline=[-10, 10, -10, 10, -1, 40], seed=5)
        RT.add(ot.RaySource(ot.Point(), divergence="Isotropic", div_angle=12, pos=[0.2, -0.1, 0],
                            spectrum=ot.LightSpectrum("Monochromatic", wl=550.)))
        RT.add(ot.Detector(ot.SphericalSurface(r=6, R=-9), pos=[0, 0, 20]))
        RT.trace(1000)
    sa = against_own_hits(RT, projection_method="Equal-Area")
    assert sa.N == 1000
    with ot.global_options.no_warnings():  # another projection, other positions
        other = RT.spot_analysis(projection_method="Orthographic", frequencies=[])
    assert other.N == 1000 and abs(other.rms_radius - sa.rms_radius) > 1e-6 * sa.rms_radius


def test_degenerate_bundles():
    g, RT = traced("c1_single_lens")
    with ot.global_options.no_warnings():
        none = RT.spot_analysis(extent=[5, 6, 5, 6], n_radii=7, frequencies=[0.0, 1.0, 2.0])
        check_empty(none, 7, 3)
        assert np.array_equal(none.extent, [5, 6, 5, 6])
        assert none.encircled_energy(1.0) == 0 and np.isnan(none.radius_of(0.5))
        none = RT.spot_analysis(extent=[5, 6, 5, 6], n_radii=7)
        check_empty(none, 7, 65)
        assert np.array_equal(none.frequencies, np.linspace(0, 1, 65))

        no_otf = RT.spot_analysis(frequencies=[])
        assert no_otf.N == 2000 and no_otf.rms_radius > 0 and no_otf.ee.shape == (257,)
        for key in ("frequencies", "otf_x", "otf_y", "mtf_x", "mtf_y"):
            assert getattr(no_otf, key).shape == (0,)

        # one ray along the axis
        RT1 = scenes.c1_single_lens(ot)
        init = (np.array([[0., 0., -20.]]), np.array([[0., 0., 1.]]), np.array([[1., 0., 0.]]), g["w0"][:1], g["wl"][:1])
        RT1.trace(1, _initial_rays=init, _N_list=np.array([1]))
        one = RT1.spot_analysis(n_radii=5)
    assert one.N == 1 and 0 < one.power <= float(g["w0"][0])
    assert np.array_equal(one.centroid, [0, 0])
    assert one.rms_x == one.rms_y == one.rms_radius == one.cov_xy == one.max_radius == 0
    assert np.array_equal(one.ee, [0, 1, 1, 1, 1, 1]) and np.array_equal(one.ee_radii, np.zeros(6))
    assert np.array_equal(one.frequencies, np.linspace(0, 1, 65))
    assert np.array_equal(one.otf_x, np.ones(65)) and np.array_equal(one.mtf_y, np.ones(65))
    assert one.radius_of(1.0) == 0 and one.encircled_energy(0.0) == 1


# ---- the entry points on synthetic lists ---------------------------------------------------------------------------
LDS_BINS = 64 * 1024 // 8  # most radial bins the histogram keeps in LDS


def synthetic(n):
    """n entries about (3, -15), sigma 0.01; a third of them with weight 0 and NaN positions."""
    rng = np.random.default_rng(1000 + n)
    x, y = 3 + 0.01 * rng.standard_normal(n), -15 + 0.01 * rng.standard_normal(n)
    w = rng.uniform(0.1, 1, n).astype(np.float32)
    dead = np.arange(n) % 3 == 1
    w[dead] = 0
    x[dead] = y[dead] = np.nan
    return x, y, w


def as_compact(x, y, w, rng):
    """The same entries as a compact list of a bundle of n rays: uneven fill counts, empty pieces among them; what lies behind a
    piece's fill would be seen if it were read (weight 1, far away)."""
    n = x.shape[0]
    plen = int(_capi.load_library().ot_hit_piece_len(n))
    assert plen == 1024
    fill = np.zeros(1024, dtype=np.uint32)
    left = n
    for k in rng.permutation(1024)[:max(1, min(1024, n // 90 + 3))]:
        fill[k] = min(left, int(rng.integers(0, min(plen, max(1, n // 3)) + 1)))
        left -= int(fill[k])
    k = 0
    while left:  # whatever is left over goes where there is room
        room = min(left, plen - int(fill[k]))
        fill[k] += room
        left -= room
        k += 1
    assert fill.sum() == n and (fill == 0).any()
    cx, cy, cw = np.full(1024 * plen, 1e6), np.full(1024 * plen, -1e6), np.ones(1024 * plen, dtype=np.float32)
    at = np.concatenate([k * plen + np.arange(fill[k]) for k in range(1024)]).astype(np.int64)
    cx[at], cy[at], cw[at] = x, y, w
    return cx, cy, cw, fill


def run_entry_points(x, y, w, fill, n, n_radii_list, freqs):
    lib, dev = _capi.load_library(), torch.device("cuda")
    dx, dy, dw = (torch.from_numpy(a).to(dev) for a in (x, y, w))
    dfill = None if fill is None else torch.from_numpy(fill.astype(np.int32)).to(dev)
    st = stream_ptr()
    ws = torch.empty(_capi.spot_ws(max(len(f) for f in freqs)), dtype=torch.float64, device=dev)
    mom = torch.full((8,), np.nan, dtype=torch.float64, device=dev)
    _capi.check(lib.ot_spot_moments(n, ptr(dfill), ptr(dx), ptr(dy), ptr(dw), ptr(ws), ptr(mom), st))
    hists, otfs = [], []
    for n_radii in n_radii_list:
        hist = torch.zeros(n_radii, dtype=torch.float64, device=dev)
        _capi.check(lib.ot_spot_radial(n, ptr(dfill), ptr(dx), ptr(dy), ptr(dw), ptr(mom), n_radii, ptr(hist), st))
        hists.append(hist.cpu().numpy())
    for f in freqs:
        out = torch.full((4 * len(f),), np.nan, dtype=torch.float64, device=dev)
        df = torch.from_numpy(f).to(dev)
        _capi.check(lib.ot_spot_otf(n, ptr(dfill), ptr(dx), ptr(dy), ptr(dw), ptr(mom), ptr(df), len(f), ptr(ws), ptr(out), st))
        otfs.append(out.cpu().numpy().reshape(4, len(f)))
    return mom.cpu().numpy(), hists, otfs


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1025, 70000, 2048 * 256 + 257])
def test_entry_points_on_synthetic_lists(n):
    """Sizes around a wave, a workgroup and the grid caps (the last one the first at which the cap of 2048 workgroups binds for
    the moments, and every walker takes more than one step); frequency counts around the chunk of 8; radial bins in LDS and, above
    its budget, in global memory; dense and compact.  Tolerances as in `against_own_hits`."""
    x, y, w = synthetic(n)
    n_radii_list = [1, 32, LDS_BINS + 1808]
    t0 = numpy_spot(x, y, w, [0.0])
    sigma = max(t0["rms_radius"], 0.01)
    freqs = [np.linspace(0, 2 / sigma, K) if K > 1 else np.array([0.7 / sigma]) for K in (1, 8, 9, 17)]
    truths = [numpy_spot(x, y, w, f) for f in freqs]
    t = truths[0]
    W, r, rmax = t["power"], t["r"], t["max_radius"]
    dc = 2e-13 * t["abs_c"]
    # hits near an edge of the radial bins take no part in the comparison: at most 1 % of the entries, from NumPy alone
    tau = 1e-12
    for n_radii in n_radii_list:
        if rmax > 0:
            pos = r / rmax * n_radii  # edge k lies at k
            near = (np.abs(pos - np.rint(pos)) * rmax / n_radii <= tau) & (np.rint(pos) >= 1) & (np.rint(pos) <= n_radii - 1)
            assert np.count_nonzero(near) <= 0.01 * n
    for lay in ("dense", "compact"):
        if lay == "dense":
            mom, hists, otfs = run_entry_points(x, y, w, None, n, n_radii_list, freqs)
        else:
            cx, cy, cw, fill = as_compact(x, y, w, np.random.default_rng(7 + n))
            mom, hists, otfs = run_entry_points(cx, cy, cw, fill, n, n_radii_list, freqs)
        assert mom[3] == t["N"] == np.count_nonzero(w)
        assert_close(mom[0], W, rtol=1e-13, what="sum w")
        for k in range(2):
            assert_close(mom[1 + k] / mom[0], t["centroid"][k], rtol=0, atol=dc[k], what="centroid")
        assert_close(np.sqrt(mom[4] / mom[0]), t["rms_x"], rtol=1e-13, atol=1e-300, what="rms_x")
        assert_close(np.sqrt(mom[5] / mom[0]), t["rms_y"], rtol=1e-13, atol=1e-300, what="rms_y")
        assert_close(mom[6] / mom[0], t["cov_xy"], rtol=0, atol=2e-13 * t["abs_cov"], what="cov_xy")
        assert_close(np.sqrt(mom[7]), rmax, rtol=4 * EPS, atol=dc.sum() if n > 1 else 0, what="max_radius")
        for n_radii, hist in zip(n_radii_list, hists):
            assert_close(hist.sum(), W, rtol=1e-13, what="histogram sum")
            if n == 1:  # (w x / w need not return x: a radius of one rounding then fills the last bin, in NumPy as here)
                assert hist[0 if rmax == 0 else n_radii - 1] == W
                continue
            ee = np.cumsum(hist)[:-1] / hist.sum()
            lo, hi = ee_bounds(t, n_radii, tau)
            assert np.all(lo - 1e-12 <= ee) and np.all(ee <= hi + 1e-12), (lay, n_radii)
        for f, tk, got in zip(freqs, truths, otfs):
            for q, (key, d) in enumerate((("otf_x", dc[0]), ("otf_y", dc[1]))):
                tol = 2e-13 + 2 * np.pi * np.abs(f).max() * d
                assert_close(got[2 * q] / mom[0], tk[key].real, rtol=0, atol=tol, what=f"{lay} {key} real K={len(f)}")
                assert_close(got[2 * q + 1] / mom[0], tk[key].imag, rtol=0, atol=tol, what=f"{lay} {key} imag K={len(f)}")
