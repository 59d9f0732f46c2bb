"""Raytracer.ray_fans and the `ot_fans_*` entry points on the GPU.

Truth is NumPy longdouble following the definition (tests/fans_cases.py).  Each pass is judged on the planes and records that the
device's earlier passes left: the transverse step on the stored positions and the weights of `ot_wavefront_paths`, the band
records on the device's own ex, ey and cleared weights about the means of the device's own first pass, the bins on those planes
about the mean path of the device's records and the pupil of the device's moments record.

Bounds: counts, cleared weights and the extremes of opl equal the truth; ex and ey per ray within `fans_cases.transverse`'s bound;
the largest squared distance within 4 eps relative; every sum within (n + 40) eps sum |terms| (`wavefront_cases.sum_bound`), n the
rays of the band or of the bin; the records the same bits over two calls."""
import ctypes as C

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd._device import ptr, stream_ptr, to_dev
from optrace_amd.ray_storage import RayStorage

import chromatic_cases as cc
import fans_cases as fc
import wavefront_cases as wc
from test_gpu_chromatic import EDGES, FAR_END, Storage, dev, same_bits, traced
from test_gpu_wavefront import call_moments, call_paths, lens_tracer

pytestmark = pytest.mark.gpu

EPS, LD, M, BM, NONE = fc.EPS, fc.LD, fc.M, fc.BIN_M, fc.NO_BAND
F64 = lambda a: np.asarray(a).astype(np.float64)
d3 = C.c_double * 3
FOCUS = (0.25, -0.5, 9.0)


# ---- the entry points, device tensors in and host arrays out -----------------------------------------------------------------------
def call_transverse(R, first, count, k, focus, w):
    """w: device tensor (count,) f32, cleared in place -> (ex, ey device tensors, n_parallel)"""
    lib = _capi.load_library()
    ex, ey = (torch.full((count,), -7.0, dtype=torch.float64, device=dev()) for _ in range(2))
    par = torch.full((1,), 99, dtype=torch.int64, device=dev())
    _capi.check(lib.ot_fans_transverse(C.byref(R), first, count, k, d3(*(float(c) for c in focus)), ptr(w), ptr(ex), ptr(ey), ptr(par),
                                       stream_ptr()))
    return ex, ey, int(par.cpu()[0])


def call_bands(opl, ex, ey, w, wl, key, K):
    lib = _capi.load_library()
    count = opl.shape[0]
    n_ws = lib.ot_fans_workspace(count, K)
    assert n_ws == 8 * K * min(-(-count // 256), 1024)
    ws = torch.full((n_ws,), np.nan, dtype=torch.float64, device=dev())  # (a partial read before it is written shows)
    rec = torch.full((K * M,), -7.0, dtype=torch.float64, device=dev())
    _capi.check(lib.ot_fans_bands(count, ptr(opl), ptr(ex), ptr(ey), ptr(w), ptr(wl), ptr(key), K, ptr(ws), ptr(rec), stream_ptr()))
    return rec


def call_bins(u, v, opl, ex, ey, w, key, mom, pupil_radius, rec, K, n_bins, slab):
    lib = _capi.load_library()
    out = torch.zeros(K * 2 * n_bins * BM, dtype=torch.float64, device=dev())
    pr = np.nan if pupil_radius is None else pupil_radius
    _capi.check(lib.ot_fans_bins(u.shape[0], ptr(u), ptr(v), ptr(opl), ptr(ex), ptr(ey), ptr(w), ptr(key), ptr(mom), pr, ptr(rec), K,
                                 n_bins, slab, ptr(out), stream_ptr()))
    return out.cpu().numpy().reshape(K, 2, n_bins, BM)


# ---- synthetic storages and planes ----------------------------------------------------------------------------------------------------
def build(count, nt, k, first, K, seed, behind=37, keys=None, far=True):
    """-> (Storage, planes): the storage builder of test_gpu_chromatic.build, and host planes of `count` entries as the sphere stage
    leaves them: u, v, opl (f64, NaN where w = 0), w (f32), wl (f32), key (uint8).  Four rays in five have a weight; of those, one in
    twenty runs within a plane z = const.  Keys are drawn from 0 .. K - 1 and 255 unless `keys` gives them.  far: one ray with a
    weight in no band, and for K > 1 one of band K - 1, lies 1e30 away with a weight and a path of 1e30: any leak between bands
    shows.  The slots outside the range -- `first` in front, `behind` after it -- hold positions and weights of 1e30 too, which any
    read beyond the range would bring in."""
    rng = np.random.default_rng(seed)
    N = first + count + behind
    p = np.full((N, nt, 3), 1e30)
    p[:, 1::2] = FAR_END
    w = np.full((N, nt), 1e30, dtype=np.float32)
    wl = np.full(N, 1e30, dtype=np.float32)
    alive = rng.uniform(size=count) < 0.8
    q = rng.normal(size=(count, nt, 3)) * [3.0, 2.0, 1.0] + [0.5, -0.25, 10.0]
    q[:, k + 1, 2] += 4.0
    flat = rng.uniform(size=count) < 0.05
    q[flat, k + 1, 2] = q[flat, k, 2]                  # d_z == 0
    q[~alive] = np.nan
    wo = np.where(alive, rng.uniform(0.1, 1.0, size=count), 0.0)
    u, v = rng.normal(size=(2, count)) * 0.3 + [[0.05], [-0.02]]
    opl = 50 + rng.normal(size=count) * 1e-3
    key = rng.choice(np.arange(K + 1), size=count) if keys is None else np.array(keys)
    key = np.where(key >= K, NONE, key).astype(np.uint8)
    if far and count >= 8:
        at = [count // 3] + ([2 * count // 3] if K > 1 else [])
        q[at], wo[at], opl[at] = 1e30, 1e30, 1e30
        q[at, k + 1] = FAR_END
        u[at], v[at] = 0.05, -0.02  # (near the pupil centre: in both cuts)
        key[at[0]] = NONE
        if K > 1:
            key[at[1]] = K - 1
    u[wo == 0], v[wo == 0], opl[wo == 0] = np.nan, np.nan, np.nan
    p[first:first + count] = q
    w[first:first + count, k] = wo.astype(np.float32)
    wl[first:first + count] = rng.uniform(400, 700, size=count).astype(np.float32)
    return Storage(p, w, wl), dict(u=u, v=v, opl=opl, w=wo.astype(np.float32), wl=wl[first:first + count].copy(), key=key)


def check_entry_points(S, P, first, count, k, K, what, n_bins=32, slab=0.25, pupil_radius=None, focus=FOCUS):
    """The three passes on the storage S and the planes P -> (records, bins) of the device, checked against the truth."""
    u, v, opl = (to_dev(P[a], np.float64) for a in ("u", "v", "opl"))
    w, wl, key = to_dev(P["w"], np.float32), to_dev(P["wl"], np.float32), to_dev(P["key"], np.uint8)
    mom = call_moments(u, v, opl, w, wl)  # (as the sphere stage has them: before the parallel rays lose their weight)
    t = fc.transverse(S.p, P["w"], first, count, k, focus)
    ex, ey, par = call_transverse(S.rays, first, count, k, focus, w)
    hex_, hey, hw = ex.cpu().numpy(), ey.cpu().numpy(), w.cpu().numpy()
    worst_t = fc.check_transverse(hex_, hey, hw, par, t, what)

    rec_d = call_bands(opl, ex, ey, w, wl, key, K)
    rec = rec_d.cpu().numpy().reshape(K, M)
    assert same_bits(rec, call_bands(opl, ex, ey, w, wl, key, K).cpu().numpy().reshape(K, M)), f"{what}: records, two calls, different bits"
    val, mag = fc.band_records(P["opl"], hex_, hey, hw, P["wl"], P["key"], K, means=fc.record_means(rec))
    worst_r = fc.check_records(rec, val, mag, what)

    out = call_bins(u, v, opl, ex, ey, w, key, mom, pupil_radius, rec_d, K, n_bins, slab)
    bval, bmag, passed = fc.fan_bins(P["u"], P["v"], P["opl"], hex_, hey, hw, P["key"], K, mom.cpu().numpy(), pupil_radius, rec, n_bins, slab)
    worst_b = fc.check_bins(out, bval, bmag, what)
    assert np.array_equal(out[..., 1].sum(axis=(0, 2)), passed), f"{what}: {out[..., 1].sum(axis=(0, 2))} rays in the cuts, {passed} pass"
    print(f"{what}: of their bounds ex, ey use at most {worst_t:.3g}, the records {worst_r:.3g}, the bins {worst_b:.3g}; "
          f"{par} parallel, {passed} in the cuts")
    return rec, out


@pytest.mark.parametrize("count,nt,k,first,K", [
    (1, 2, 0, 5, 1), (63, 5, 3, 5, 2), (64, 5, 0, 33, 3), (65, 2, 0, 5, 32),   # around one wave; `first` off the 128-byte lines
    (255, 5, 3, 7, 3), (256, 2, 0, 33, 2), (257, 5, 0, 5, 32),                  # around one workgroup
    (3000, 5, 3, 64, 1),
])
def test_entry_points_on_synthetic_planes(count, nt, k, first, K):
    seed = count + 7 * nt + K
    S, P = build(count, nt, k, first, K, seed)
    what = f"{count} rays, nt {nt}, section {k}, {K} bands"
    rec, out = check_entry_points(S, P, first, count, k, K, what)
    if count >= 255:
        assert np.any(P["w"] == 0) and np.any(P["key"] == NONE) and rec[:, 1].sum() > 0 and out[..., 1].sum() > 0
    # the same planes with the storage ending at the range's end, and a pupil radius given
    S, P = build(count, nt, k, first, K, seed + 1, behind=0)
    assert first + count == S.N
    check_entry_points(S, P, first, count, k, K, what + ", first + count == N", n_bins=7, slab=0.1, pupil_radius=0.8)


def test_parallel_rays_are_cleared_and_counted():
    S, P = build(3000, 3, 1, 9, 2, 77)
    t = fc.transverse(S.p, P["w"], 9, 3000, 1, FOCUS)
    assert 50 < t["n_parallel"] < 250 and np.count_nonzero(t["w"]) == np.count_nonzero(P["w"]) - t["n_parallel"]


# ---- bins at their edges ----------------------------------------------------------------------------------------------------------------
def unit_moments(W=1.0):
    """A moments record whose pupil is the unit disc about (0, 0): x = u and y = v exactly."""
    return to_dev(np.array([W, 1, 0, 0, 0, 0, 0, 0, 0, 1, 1.0]), np.float64)


def unit_records(K, mean=50.0):
    rec = np.zeros((K, M))
    rec[:, 0], rec[:, 1], rec[:, 2] = 2.0, 1, 2.0 * mean
    return rec


@pytest.mark.parametrize("n_bins", [1, 2, 32, 256])
def test_single_rays_at_the_edges_of_the_slab_and_of_the_bins(n_bins):
    slab = 0.1
    above = float(np.nextafter(slab, 1.0))
    #            in the tangential cut      just outside it             its last and first bin      and the same for the sagittal one
    pts = [(slab, 0.3), (-slab, -0.3), (above, 0.3), (-above, 0.6), (0.0, 1.0), (0.0, -1.0),
           (0.3, slab), (-0.3, -slab), (0.3, above), (0.6, -above), (1.0, 0.0), (-1.0, 0.0)]
    n = len(pts)
    u, v = np.array(pts).T
    w = (0.5 + np.arange(n) / 16).astype(np.float32)
    opl, ex, ey = 50 + np.arange(n) / 8, np.arange(n) / 4 - 1, 2 - np.arange(n) / 2
    key = (np.arange(n) % 2).astype(np.uint8)
    rec = unit_records(2)
    out = call_bins(*(to_dev(a, np.float64) for a in (u, v, opl, ex, ey)), to_dev(w, np.float32), to_dev(key, np.uint8), unit_moments(),
                    None, to_dev(rec, np.float64), 2, n_bins, slab)
    bin_of = lambda c: min(int(np.floor((c + 1) / 2 * n_bins)), n_bins - 1)
    want = np.zeros((2, 2, n_bins, BM))
    for fan, rays in ((0, (0, 1, 4, 5)), (1, (6, 7, 10, 11))):
        for r in rays:
            c = pts[r][1 - fan]
            wd = float(w[r])
            want[key[r], fan, bin_of(c)] += [wd, 1, wd * c, wd * ex[r], wd * ey[r], wd * (opl[r] - 50)]
    assert bin_of(1.0) == n_bins - 1 and bin_of(-1.0) == 0
    # (dyadic weights and values, at most two rays per slot: the sums are exact but for w c at c = +-0.3)
    assert np.array_equal(out[..., [0, 1, 3, 4, 5]], want[..., [0, 1, 3, 4, 5]]), out - want
    assert np.allclose(out[..., 2], want[..., 2], rtol=4 * EPS, atol=0)
    bval, bmag, passed = fc.fan_bins(u, v, opl, ex, ey, w, key, 2, unit_moments().cpu().numpy(), None, rec, n_bins, slab)
    fc.check_bins(out, bval, bmag, f"{n_bins} bins")
    assert passed.tolist() == [4, 4] and out[..., 1].sum() == 8


def test_lds_path_and_global_path_agree():
    """32 bands x 256 bins, 786 KiB of sums, go to global memory; 3 bands x 32 bins, 9 KiB, are privatised in LDS.  The rays carry the
    keys 0 .. 2 and 255; eight of the fine bins make one coarse bin exactly, (c + 1) / 2 * 256 being 8 times (c + 1) / 2 * 32."""
    count = 5000
    S, P = build(count, 2, 0, 3, 3, 12)
    u, v, opl = (to_dev(P[a], np.float64) for a in ("u", "v", "opl"))
    w, wl, key = to_dev(P["w"], np.float32), to_dev(P["wl"], np.float32), to_dev(P["key"], np.uint8)
    mom = call_moments(u, v, opl, w, wl)
    ex, ey, _ = call_transverse(S.rays, 3, count, 0, FOCUS, w)
    rec3 = call_bands(opl, ex, ey, w, wl, key, 3)
    rec32 = torch.zeros(32 * M, dtype=torch.float64, device=dev())
    rec32[:3 * M] = rec3
    lds = call_bins(u, v, opl, ex, ey, w, key, mom, None, rec3, 3, 32, 0.25)
    glob = call_bins(u, v, opl, ex, ey, w, key, mom, None, rec32, 32, 256, 0.25)
    assert np.all(glob[3:] == 0)
    coarse = F64(glob[:3].astype(LD).reshape(3, 2, 32, 8, BM).sum(axis=3))
    hex_, hey, hw = ex.cpu().numpy(), ey.cpu().numpy(), w.cpu().numpy()
    rec = rec3.cpu().numpy().reshape(3, M)
    bval, bmag, passed = fc.fan_bins(P["u"], P["v"], P["opl"], hex_, hey, hw, P["key"], 3, mom.cpu().numpy(), None, rec, 32, 0.25)
    fc.check_bins(lds, bval, bmag, "LDS path")
    fc.check_bins(coarse, bval, bmag, "global path, coarsened")
    fine, fmag, _ = fc.fan_bins(P["u"], P["v"], P["opl"], hex_, hey, hw, P["key"], 32, mom.cpu().numpy(), None, rec32.cpu().numpy(), 256, 0.25)
    fc.check_bins(glob, fine, fmag, "global path")
    assert np.array_equal(lds[..., 1], coarse[..., 1]) and lds[..., 1].sum() == passed.sum() > 1000
    bound = 2 * wc.sum_bound(F64(bval[..., 1])[..., None], F64(bmag))
    assert np.all(np.abs(lds - coarse) <= bound), "the two paths differ by more than twice the bound"


# ---- a populated grid ---------------------------------------------------------------------------------------------------------------------
def test_populated_grid_of_analytic_aberrations():
    """64 x 64 pupil points on cell centres, the unit disc given: six columns lie within |x| <= 0.1, four points fall into each of 16
    bins: 24 rays per bin in either fan, 12 per band when the ray index's parity is the band."""
    A, B, Cc, D, E = 0.02, -0.005, 0.001, -0.002, 3e-4
    c = (np.arange(64) + 0.5) / 32 - 1
    x, y = (a.ravel() for a in np.meshgrid(c, c, indexing="ij"))  # ray index = 64 i + j, x from i
    inside = x * x + y * y <= 1
    w = np.where(inside, 0.5 + 0.25 * (np.arange(4096) % 3), 0).astype(np.float32)
    ex, ey, opl = A * x ** 3 + D, A * y ** 3 + B * y + Cc, 50 + E * (x * x + y * y) ** 2
    ex[~inside], ey[~inside], opl[~inside] = np.nan, np.nan, np.nan
    wl = np.full(4096, 550.0, dtype=np.float32)
    dv = lambda a: to_dev(a, np.float64)
    for K, key in ((1, np.zeros(4096, dtype=np.uint8)), (2, (np.arange(4096) % 2).astype(np.uint8))):
        rec_d = call_bands(dv(opl), dv(ex), dv(ey), to_dev(w, np.float32), to_dev(wl, np.float32), to_dev(key, np.uint8), K)
        rec = rec_d.cpu().numpy().reshape(K, M)
        val, mag = fc.band_records(opl, ex, ey, w, wl, key, K, means=fc.record_means(rec))
        fc.check_records(rec, val, mag, f"grid, {K} bands")
        out = call_bins(dv(x), dv(y), dv(opl), dv(ex), dv(ey), to_dev(w, np.float32), to_dev(key, np.uint8), unit_moments(), 1.0, rec_d, K,
                        16, 0.1)
        assert np.all(out[..., 1] == 24 // K), out[..., 1]
        bval, bmag, passed = fc.fan_bins(x, y, opl, ex, ey, w, key, K, unit_moments().cpu().numpy(), 1.0, rec, 16, 0.1)
        fc.check_bins(out, bval, bmag, f"grid, {K} bands")
        assert passed.tolist() == [384, 384]
        # the means per bin, and that they follow the curves up to the cubic's spread over a bin
        a = ot.RayFans(rec, out, 0, [0, 0, 0], 1.0, (0, 0), 1.0, 0.1)
        f = fc.figures(rec, out)
        for name in ("pupil", "ex", "ey", "opd"):
            assert np.allclose(getattr(a, name), F64(f[name]), rtol=1e-14, atol=1e-18), name
        yb, eyb, _ = a.tangential(0)
        assert np.allclose(eyb, A * yb ** 3 + B * yb + Cc, atol=A * 0.125 ** 2 * 3) and np.allclose(a.sagittal(0)[1], A * a.sagittal(0)[0] ** 3 + D, atol=A * 0.05)
        assert np.all(np.diff(yb) > 0.05)


# ---- special bands, nothing to do, bad arguments ---------------------------------------------------------------------------------------
def test_bands_with_no_ray_one_ray_and_one_wave():
    """Five bands over 1500 rays: all the others | none | one ray of the second workgroup | its second wave | none."""
    count, K = 1500, 5
    keys = np.zeros(count, dtype=np.int64)
    keys[256 + 64:256 + 128] = 3
    keys[256 + 17] = 2
    rng = np.random.default_rng(3)
    S, P = build(count, 3, 1, 11, K, 21, keys=keys, far=False)
    # (the wave and the single ray with a weight, a place in the pupil and not in a plane, whatever was drawn)
    r = np.arange(256, 256 + 128)
    S.p[11 + r] = rng.normal(size=(128, 3, 3)) + [0, 0, 10]
    S.p[11 + r, 2, 2] += 5
    S.w[11 + r] = 0.5
    S = Storage(S.p, S.w, S.wl)
    P["w"][r], P["u"][r], P["v"][r], P["opl"][r] = 0.5, rng.normal(size=128) * 0.05, rng.normal(size=128) * 0.3, 50 + rng.normal(size=128) * 1e-3
    rec, out = check_entry_points(S, P, 11, count, 1, K, "special bands")
    assert rec[:, 1].tolist()[1:] == [0, 1, 64, 0] and rec[0, 1] > 900
    assert rec[1].tolist()[:9] == [0] * 9 and rec[1, 12] == 0 and np.all(np.isnan(rec[1, 9:12])) and np.all(out[[1, 4]] == 0)
    # one ray: it is its own mean up to the rounding of w a / w, and carries its wavelength and its path
    one = 256 + 17
    assert rec[2, 0] == 0.5 and rec[2, 5] == 0.5 * np.float64(P["wl"][one]) and rec[2, 6] == rec[2, 7] == P["opl"][one]
    assert rec[2, 8] <= 0.5 * (4 * EPS * 50) ** 2 and rec[2, 12] <= (4 * EPS * 20) ** 2
    a = ot.RayFans(rec, out, 1, FOCUS, 1.0, (0, 0), 1.0, 0.25)
    assert a.opd_rms[2] == 0 and a.rms_radius[2] == 0 and np.isnan(a.opd_rms[1]) and np.all(np.isnan(a.ex[1]))


def test_count_zero_launches_nothing():
    S, P = build(10, 3, 0, 0, 2, 2)
    lib = _capi.load_library()
    full = lambda n, dtype=torch.float64: torch.full((n,), -7.0, dtype=dtype, device=dev())
    ex, ey, rec, out, ws, a = full(4), full(4), full(2 * M), full(2 * 2 * 4 * BM), full(8), full(16)
    w, par, key = full(4, torch.float32), torch.full((1,), 99, dtype=torch.int64, device=dev()), to_dev(P["key"], np.uint8)
    st = stream_ptr()
    _capi.check(lib.ot_fans_transverse(C.byref(S.rays), 10, 0, 0, d3(0, 0, 1), ptr(w), ptr(ex), ptr(ey), ptr(par), st))
    _capi.check(lib.ot_fans_bands(0, ptr(a), ptr(ex), ptr(ey), ptr(w), ptr(w), ptr(key), 2, ptr(ws), ptr(rec), st))
    _capi.check(lib.ot_fans_bins(0, ptr(a), ptr(a), ptr(a), ptr(ex), ptr(ey), ptr(w), ptr(key), ptr(a), np.nan, ptr(rec), 2, 4, 0.1, ptr(out), st))
    for t in (ex, ey, rec, out, ws, w):
        assert np.all(t.cpu().numpy() == -7.0)
    assert int(par.cpu()[0]) == 99 and lib.ot_fans_workspace(0, 2) == 0


def test_bad_arguments_are_refused_before_any_launch():
    S, P = build(10, 3, 0, 0, 2, 2)
    lib = _capi.load_library()
    full = lambda n, dtype=torch.float64: torch.full((n,), -7.0, dtype=dtype, device=dev())
    ex, ey, rec, out, ws, a = full(10), full(10), full(2 * M), full(2 * 2 * 4 * BM), full(64), full(16)
    w, par, key = full(10, torch.float32), torch.full((1,), 99, dtype=torch.int64, device=dev()), to_dev(P["key"], np.uint8)
    st = stream_ptr()
    INVALID, UNSUPPORTED = -1, -3
    tr = lambda first, count, k, f, wp=ptr(w): lib.ot_fans_transverse(C.byref(S.rays), first, count, k, f, wp, ptr(ex), ptr(ey), ptr(par), st)
    assert tr(0, 10, 0, d3(0, 0, 1), None) == INVALID and tr(0, -1, 0, d3(0, 0, 1)) == INVALID and tr(40, 10, 0, d3(0, 0, 1)) == INVALID
    assert tr(0, 10, 2, d3(0, 0, 1)) == INVALID and tr(0, 10, -1, d3(0, 0, 1)) == INVALID and tr(0, 10, 0, d3(0, np.nan, 1)) == INVALID
    assert tr(0, 10, 0, d3(0, 0, np.inf)) == INVALID and b"ot_fans_transverse: focus not finite" in lib.ot_last_error()
    bands = lambda count, K, r=ptr(rec): lib.ot_fans_bands(count, ptr(a), ptr(ex), ptr(ey), ptr(w), ptr(w), ptr(key), K, ptr(ws), r, st)
    assert bands(10, 2, None) == INVALID and bands(-1, 2) == INVALID and bands(10, 0) == UNSUPPORTED and bands(10, 33) == UNSUPPORTED
    bins = lambda count, K, n_bins, slab, pr=np.nan, o=ptr(out): lib.ot_fans_bins(count, ptr(a), ptr(a), ptr(a), ptr(ex), ptr(ey), ptr(w),
                                                                                   ptr(key), ptr(a), pr, ptr(rec), K, n_bins, slab, o, st)
    assert bins(10, 2, 4, 0.1, o=None) == INVALID and bins(-1, 2, 4, 0.1) == INVALID
    assert bins(10, 0, 4, 0.1) == UNSUPPORTED and bins(10, 33, 4, 0.1) == UNSUPPORTED
    assert bins(10, 2, 0, 0.1) == UNSUPPORTED and bins(10, 2, 257, 0.1) == UNSUPPORTED and b"n_bins outside 1 .. 256" in lib.ot_last_error()
    for slab in (0.0, -0.5, 1.0000001, np.nan):
        assert bins(10, 2, 4, slab) == INVALID and b"slab" in lib.ot_last_error()
    assert bins(10, 2, 4, 0.1, pr=0.0) == INVALID and bins(10, 2, 4, 0.1, pr=np.inf) == INVALID
    for t in (ex, ey, rec, out, ws, w):
        assert np.all(t.cpu().numpy() == -7.0)
    assert int(par.cpu()[0]) == 99


# ---- Raytracer.ray_fans on traced rays -------------------------------------------------------------------------------------------------
def check_fans(RT, a, source_index, section, bands, n_bins, slab, pupil_radius, what):
    """Every figure of `a` against the truth evaluated on the storage read back, pass by pass on the device's own planes.
    -> what the agreement tests need: dict of the host planes and the truth of the transverse step."""
    rays = RT.rays
    nt = rays.w_list.shape[1]
    first, end = (0, rays.N) if source_index is None else (int(rays.B_list[source_index]), int(rays.B_list[source_index + 1]))
    count, k = end - first, nt - 2 if section is None else section
    assert a.section == k and a.n_bins == n_bins and a.slab == slab
    u, v, opl, w, missed = call_paths(rays, first, count, k, a.focus, a.radius)
    wl_d = rays._dev["wl"][first:end]
    mom_d = call_moments(u, v, opl, w, wl_d)
    mom = mom_d.cpu().numpy()
    assert a.n_missed == missed and np.array_equal(a.pupil_centre, mom[3:5] / mom[0])
    assert a.pupil_radius == (mom[10] if pupil_radius is None else pupil_radius)
    # the transverse step
    p, wl = rays.p_list, rays.wl_list[first:end]
    t = fc.transverse(p, w.cpu().numpy(), first, count, k, a.focus)
    ex, ey, par = call_transverse(rays._rays_struct(), first, count, k, a.focus, w)
    hu, hv, hl, hex_, hey, hw = (x.cpu().numpy() for x in (u, v, opl, ex, ey, w))
    fc.check_transverse(hex_, hey, hw, par, t, what)
    assert a.n_parallel == par
    # the bands
    key, K, edges = cc.band_keys(wl, hw > 0, bands)
    assert a.n_bands == K and (a.band_edges is None if edges is None else np.array_equal(a.band_edges, edges)), f"{what}: bands"
    assert a.n_out_of_band == np.count_nonzero((hw > 0) & (key == NONE))
    key8 = key.astype(np.uint8)
    rec = a.records
    assert same_bits(rec, call_bands(opl, ex, ey, w, wl_d, to_dev(key8, np.uint8), K).cpu().numpy().reshape(K, M)), f"{what}: the records are the entry point's"
    val, mag = fc.band_records(hl, hex_, hey, hw, wl, key8, K, means=fc.record_means(rec))
    fc.check_records(rec, val, mag, what)
    # the bins
    assert a.bins.shape == (K, 2, n_bins, BM)
    bval, bmag, passed = fc.fan_bins(hu, hv, hl, hex_, hey, hw, key8, K, mom, pupil_radius, rec, n_bins, slab)
    worst = fc.check_bins(a.bins, bval, bmag, what)
    assert np.array_equal(a.count.sum(axis=(0, 2)), passed)
    # the fields are the figures of records and bins
    eq = lambda x, y: np.array_equal(x, y, equal_nan=True)
    assert eq(a.band_N, rec[:, 1]) and eq(a.band_power, rec[:, 0]) and a.N == rec[:, 1].sum() and a.power == rec[:, 0].sum()
    assert eq(a.weight, a.bins[..., 0]) and eq(a.count, a.bins[..., 1])
    f = fc.figures(rec, a.bins)
    many = rec[:, 1] != 1
    for name, want in f.items():
        sel = many if name in ("opd_rms", "opd_rms_waves", "rms_x", "rms_y", "rms_radius") else slice(None)
        # (an extreme of the path difference is a path minus the mean path, both rounded: 8 eps of the path)
        atol = 8 * EPS * np.abs(rec[:, 6:8]).max() if name in ("opd_min", "opd_max", "opd_pv") else 1e-300
        assert np.allclose(getattr(a, name)[sel], F64(want)[sel], rtol=1e-14, atol=atol, equal_nan=True), f"{what}: {name}"
    print(f"{what}: N {a.N}, {K} bands, {passed} rays in the cuts, the bins use at most {worst:.3g} of their bound")
    return dict(t=t, hw=hw, hl=hl, key=key8, K=K, wl=wl, first=first, count=count, k=k)


def spectrum_of(bands):
    return "lines" if isinstance(bands, str) else "continuous"


@pytest.mark.parametrize("name", ["c1_single_lens", "double_gauss"])
@pytest.mark.parametrize("bands", ["lines", 4, EDGES], ids=["lines", "four", "edges"])
def test_ray_fans_of_traced_rays(name, bands):
    RT = traced(name, spectrum_of(bands))
    arg = np.array(bands) if isinstance(bands, list) else bands
    for source_index in [None] + list(range(len(RT.ray_sources))):
        what = f"{name}, source {source_index}, bands {bands if not isinstance(bands, list) else 'edges'}"
        a = RT.ray_fans(source_index=source_index, bands=bands)
        check_fans(RT, a, source_index, None, arg, 32, 0.1, None, what)
        assert ("all rays" if source_index is None else f"RS{source_index}") in a.long_desc and a.N > 0
        # the sphere given, a little off the one found, other bins, a wider cut, a pupil radius that leaves rays out
        focus, radius = a.focus + [0.01, -0.02, 0.05], a.radius * 1.01
        b = RT.ray_fans(source_index=source_index, bands=bands, focus=list(focus), radius=radius, n_bins=9, slab=0.3,
                        pupil_radius=0.8 * a.pupil_radius)
        assert np.array_equal(b.focus, focus) and b.radius == radius
        check_fans(RT, b, source_index, None, arg, 9, 0.3, 0.8 * a.pupil_radius, what + ", sphere given")
        assert 0 < b.count.sum() and b.weight.sum() < a.power


def test_an_earlier_section():
    RT = traced("double_gauss", "lines")
    a = RT.ray_fans(source_index=1, section=3, n_bins=16)
    check_fans(RT, a, 1, 3, "lines", 16, 0.1, None, "double Gauss, section 3")
    assert a.n_bands == 3 and a.N > 0


def test_fans_show_the_colour_of_a_single_lens():
    """F, d, C behind a lens of normal dispersion, the sphere about the focus of all three: blue focuses short, so above the axis its
    rays have crossed it in the focus' plane and red ones have not: the slope of ey over y rises with the wavelength."""
    a = traced("c1_single_lens", "lines").ray_fans(source_index=0)
    assert a.n_bands == 3 and a.band_edges is None and np.all(np.diff(a.wavelengths) > 0)
    slope = []
    for b in range(3):
        y, ey, _ = a.tangential(b)
        ok = np.isfinite(ey)
        assert ok.sum() >= 8
        slope.append(np.polyfit(y[ok], ey[ok], 1)[0])
    assert slope[0] < slope[1] < slope[2]


@pytest.mark.parametrize("name", ["c1_single_lens", "double_gauss"])
def test_one_band_agrees_with_the_wavefront_analysis(name):
    """bands=1 on the sphere of a wavefront analysis: the band's path figures are the bundle's, each side within its sum bounds."""
    RT = traced(name, "lines")
    wa = RT.wavefront_analysis(0)
    a = RT.ray_fans(0, bands=1, focus=list(wa.focus), radius=wa.radius)
    assert a.n_parallel == 0 and a.n_bands == 1 and a.N == wa.N and a.n_missed == wa.n_missed and a.n_out_of_band == 0
    first, end = int(RT.rays.B_list[0]), int(RT.rays.B_list[1])
    u, v, opl, w, _ = call_paths(RT.rays, first, end - first, wa.section, wa.focus, wa.radius)
    hu, hv, hl, hw = (x.cpu().numpy() for x in (u, v, opl, w))
    val, mag = wc.first_moments(hu, hv, hl, hw)
    n, W = int(val[1]), F64(val[0])
    # (a quotient of two sums: the numerator's bound over W, and as much again for W's own; two sides)
    b_mean = 4 * wc.sum_bound(n, F64(mag[2])) / W
    assert abs(a.opl_mean[0] - wa.opl_mean) <= b_mean, (a.opl_mean[0] - wa.opl_mean, b_mean)
    assert abs(a.opd_min[0] - wa.opd_min) <= b_mean + 4 * EPS * wa.opl_mean and abs(a.opd_max[0] - wa.opd_max) <= b_mean + 4 * EPS * wa.opl_mean
    mom = np.array([1.0, n, wa.opl_mean, 0, 0, 0, 0, 0, 0, 0, 0])
    s2, s2_mag, _ = wc.central_moments(hu, hv, hl, hw, mom)
    rms = F64(np.sqrt(s2 / val[0]))
    # (per side 4 eps rms and the sum's bound through the root; the means differ by b_mean at the most, which moves an RMS by no more)
    b_rms = 2 * (4 * EPS * rms + wc.sum_bound(n, F64(s2_mag)) / (W * rms)) + b_mean
    assert abs(a.opd_rms[0] - wa.rms) <= b_rms, (a.opd_rms[0] - wa.rms, b_rms)
    assert abs(a.wavelengths[0] - wa.wavelength) <= 4 * wc.sum_bound(n, 700.0 * W) / W and np.array_equal(a.pupil_centre, wa.pupil_centre)
    assert a.pupil_radius == wa.pupil_radius


@pytest.mark.parametrize("name,bands", [("c1_single_lens", "lines"), ("double_gauss", "lines"), ("double_gauss", 4)])
def test_band_spots_agree_with_the_chromatic_analysis(name, bands):
    """The band's spot in the plane of the focus is the chromatic analysis' on z = focus z: focus xy + centroid, rms_x, rms_y and
    max_radius, within the two sides' sum bounds and the per-ray bound of the transverse step."""
    RT = traced(name, spectrum_of(bands))
    a = RT.ray_fans(0, bands=bands)
    c = RT.chromatic_analysis(0, bands=bands, z=float(a.focus[2]))
    assert a.n_missed == 0 and a.n_parallel == 0 and c.n_parallel == 0 and np.array_equal(a.band_N, c.band_N), "the same rays on both sides"
    g = check_fans(RT, a, 0, None, bands, 32, 0.1, None, f"{name}, {bands}")
    t = g["t"]
    for b in range(a.n_bands):
        m = (g["key"] == b) & (g["hw"] > 0)
        n, wt = int(m.sum()), g["hw"][m].astype(LD)
        W = wt.sum()
        for axis, (e, be, rms_a, rms_c) in enumerate(((t["ex"], t["b_ex"], a.rms_x, c.rms_x), (t["ey"], t["b_ey"], a.rms_y, c.rms_y))):
            f = abs(a.focus[axis])
            # two quotients of sums of w x and w (x - f), and the per-ray rounding of x - f in the weighted mean
            b_c = F64(4 * wc.sum_bound(n, F64((wt * (np.abs(e[m]) + f)).sum())) / W + 2 * be[m].max() + 4 * EPS * f)
            assert abs(a.focus[axis] + a.centroid[b, axis] - c.centroid[b, axis]) <= b_c, (b, axis, b_c)
            mean = (wt * e[m]).sum() / W
            s2 = (wt * (e[m] - mean) ** 2).sum()
            rms = F64(np.sqrt(s2 / W))
            b_rms = 2 * (4 * EPS * rms + wc.sum_bound(n, F64(s2)) / F64(W * rms)) + 2 * F64(be[m].max()) + b_c
            assert abs(rms_a[b] - rms_c[b]) <= b_rms, (b, axis, rms_a[b] - rms_c[b], b_rms)
        b_r = F64(2 * (t["b_ex"][m].max() + t["b_ey"][m].max())) + 2 * b_c + 8 * EPS * c.max_radius[b]
        assert abs(a.max_radius[b] - c.max_radius[b]) <= b_r + 2 * F64(4 * wc.sum_bound(n, F64((wt * (np.abs(t["ex"][m]) + abs(a.focus[0]))).sum())) / W)


def test_all_absorbed_source_gives_the_empty_result():
    RT = lens_tracer(aim_at_aperture=True)
    with ot.global_options.no_warnings():
        RT.trace(1000)
        e = RT.ray_fans(0, n_bins=4)
        f = RT.ray_fans(None, bands=np.array([400.0, 500, 700]), focus=[0, 0, 30], radius=5.0, n_bins=8, slab=0.5, pupil_radius=0.7)
        before = RT.ray_fans(0, section=0, focus=[0, 0, -100], radius=-104.0)  # (the section before the stop is alive)
    assert e.N == 0 and e.power == 0 and e.n_bands == 1 and e.band_edges is None and e.section == 3 and e.n_bins == 4
    assert np.all(np.isnan(e.focus)) and np.isnan(e.radius) and np.all(e.count == 0) and np.all(np.isnan(e.ex)) and np.isnan(e.opd_rms[0])
    assert f.N == 0 and f.n_bands == 2 and f.band_edges.tolist() == [400, 500, 700] and f.focus.tolist() == [0, 0, 30] and f.radius == 5.0
    assert f.pupil_radius == 0.7 and f.slab == 0.5 and f.count.shape == (2, 2, 8) and np.all(np.isnan(f.wavelengths))
    assert before.N == 1000 and before.n_bands == 2


def test_padded_storage_and_stale_index_plane(monkeypatch):
    """A generated trace of 4099 rays in planes 4224 apart, its index plane still unwritten when the fans are asked for."""
    monkeypatch.setattr(RayStorage, "PAD_FROM", 512)
    RT = lens_tracer()
    with ot.global_options.no_warnings():
        RT.trace(4099)
        assert RT.rays._Np == 4224 and RT.rays._n_stale, "nothing here may have read the plane through the hook"
        a = RT.ray_fans(0)
        assert not RT.rays._n_stale
        b = RT.ray_fans(0)
    assert a.N == 4099 and a.n_bands == 2 and np.allclose(a.wavelengths, [486, 656], rtol=1e-12, atol=0) and a.n_missed == 0 and a.radius > 0
    assert same_bits(a.records, b.records) and np.array_equal(a.count, b.count) and np.array_equal(a.focus, b.focus)
    check_fans(RT, a, 0, None, "lines", 32, 0.1, None, "padded storage")
