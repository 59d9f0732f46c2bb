"""Raytracer.footprints and the `ot_footprint_*` entry points on the GPU.

Truth is NumPy longdouble following the definition (tests/footprint_cases.py): on synthetic storages handed to the entry points
through ctypes, and on the device's own ray storage read back for rays injected into the device trace
(tests/golden/trace_*.npz).

Bounds, as stated with the feature: counts equal the truth; minima and maxima are entries of the planes, bit for bit; the largest
squared distance from the axis is within 4 eps relative (two subtractions, two squares, one sum); every sum is within
(n + 40) eps sum |terms| (`footprint_cases.sum_bound`), the second-pass sums about the centroid the device forms from its own
record, which is an input of that pass.  The arriving sums of section i and the living sums of section i - 1 are the same
additions over the same plane in the same order, so they are held to equality.  The maps are the one result that depends on the
order of arrival: every cell is held to the sum bound for the rays the written formula puts there, and a cell without such a ray
to zero."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd._device import ptr, stream_ptr, to_dev

import footprint_cases as fc
import scenes
from helpers import load

pytestmark = pytest.mark.gpu

EPS, LD, M = fc.EPS, fc.LD, fc.M
CAP = 1024  # OT_FP_BLOCKS: most workgroups of 256 per section


def dev():
    return torch.device("cuda", torch.cuda.current_device())


# ---- synthetic storages ----------------------------------------------------------------------------------------------------------
class Storage:
    """Host arrays p (N, nt, 3), w (N, nt) in the layout of the reference and their planes on the device behind an `ot_rays`."""

    def __init__(self, p, w):
        self.p, self.w = p, w
        self.N, self.nt = w.shape
        self.d_p = to_dev(np.ascontiguousarray(p.transpose(2, 1, 0)), np.float64)  # r + N * (i + nt * c)
        self.d_w = to_dev(np.ascontiguousarray(w.T), np.float32)
        self.rays = _capi.Rays()
        self.rays.N, self.rays.nt, self.rays.p, self.rays.w = self.N, self.nt, self.d_p.data_ptr(), self.d_w.data_ptr()


def build(alive, first, seed, behind=37):
    """alive (count, nt) -> (Storage, first, count): the rays of the range live where `alive` says, dead slots hold NaN positions
    and weight 0.  The slots outside the range -- `first` in front, `behind` after it: the stride differs from the count -- hold
    living rays far away, which any read beyond the range would bring into the sums."""
    rng = np.random.default_rng(seed)
    count, nt = alive.shape
    N = first + count + behind
    p = np.full((N, nt, 3), 1e30)
    w = np.full((N, nt), 1e30, dtype=np.float32)
    q = rng.normal(size=(count, nt, 3)) * [3.0, 2.0, 1.0] + [0.5, -0.25, 10.0]
    q[~alive] = np.nan
    p[first:first + count] = q
    w[first:first + count] = np.where(alive, rng.uniform(0.1, 1.0, size=(count, nt)), 0.0).astype(np.float32)
    return Storage(p, w), first, count


def dying(count, nt, seed, keep=0.8):
    """Rays that die for good, a share of 1 - keep of the living at every surface; the last section empty."""
    rng = np.random.default_rng(seed + 1000)
    passes = rng.uniform(size=(count, nt)) < keep
    passes[:, 0] = True
    alive = np.cumprod(passes, axis=1).astype(bool)
    alive[:, nt - 1] = False
    return alive


def random_axis(nt, seed):
    return np.random.default_rng(seed + 2000).uniform(-1, 1, size=(nt, 2))


def call_moments(S, first, count, axis):
    lib = _capi.load_library()
    n_ws = lib.ot_footprint_workspace(count, S.nt)
    assert n_ws == 13 * S.nt * min(-(-count // 256), CAP)
    ws = torch.full((n_ws,), np.nan, dtype=torch.float64, device=dev())  # (a partial read before it is written shows)
    rec = torch.full((S.nt * M,), -7.0, dtype=torch.float64, device=dev())
    d_axis = to_dev(axis, np.float64)
    _capi.check(lib.ot_footprint_moments(C.byref(S.rays), first, count, ptr(d_axis), ptr(ws), ptr(rec), stream_ptr()))
    return rec


def call_maps(S, first, count, axis, rec, n_px):
    lib = _capi.load_library()
    out = torch.zeros(S.nt * n_px * n_px, dtype=torch.float64, device=dev())
    d_axis = to_dev(axis, np.float64)
    _capi.check(lib.ot_footprint_maps(C.byref(S.rays), first, count, ptr(d_axis), ptr(rec), n_px, ptr(out), stream_ptr()))
    return out.cpu().numpy().reshape(S.nt, n_px, n_px)


def check_moments(S, first, count, axis, what):
    """-> the device's record (device tensor, host array)"""
    rec_d = call_moments(S, first, count, axis)
    rec = rec_d.cpu().numpy().reshape(S.nt, M)
    again = call_moments(S, first, count, axis).cpu().numpy().reshape(S.nt, M)
    assert np.array_equal(rec.view(np.uint64), again.view(np.uint64)), f"{what}: two calls, different bits"
    val, mag = fc.records(S.p, S.w, first, count, axis, centroid=fc.record_centroid(rec))
    fc.check_record(rec, val, mag, what)
    # arriving at section i = alive in section i - 1: the same additions
    assert np.array_equal(rec[1:, 2:4], rec[:-1, 0:2]) and np.array_equal(rec[0, 2:4], rec[0, 0:2]), f"{what}: arriving sums"
    return rec_d, rec


@pytest.mark.parametrize("count,nt,first", [
    (1, 3, 5), (255, 3, 5), (256, 3, 33), (257, 3, 5),  # around one workgroup; `first` off the 128-byte lines
    (256 * CAP + 1, 3, 7),                              # one ray more than the launch has lanes: the strided walk's second step
    (1000, 2, 3), (700, 40, 64),                        # the fewest sections there are, and many
])
def test_moments_on_dying_rays(count, nt, first):
    seed = count + nt
    S, first, count = build(dying(count, nt, seed), first, seed)
    assert first + count < S.N
    check_moments(S, first, count, random_axis(nt, seed), f"{count} rays, {nt} sections")


def test_moments_range_ends_with_the_storage_off_the_lines():
    S, first, count = build(dying(999, 4, 8), 13, 8, behind=0)
    assert first % 32 and first + count == S.N
    check_moments(S, first, count, random_axis(4, 8), "first + count == N")


def special_sections():
    """Six sections over 1500 rays: all alive | all alive | the second wave of the second workgroup alone | one ray of it | none
    | none."""
    count, nt = 1500, 6
    alive = np.zeros((count, nt), dtype=bool)
    alive[:, :2] = True
    alive[256 + 64:256 + 128, 2] = True
    alive[256 + 64 + 17, 3] = True
    return build(alive, 11, 21)


def test_moments_of_sections_with_one_wave_one_ray_and_none():
    S, first, count = special_sections()
    axis = random_axis(S.nt, 21)
    _, rec = check_moments(S, first, count, axis, "special sections")
    assert rec[:, 1].tolist() == [1500, 1500, 64, 1, 0, 0] and rec[:, 3].tolist() == [1500, 1500, 1500, 64, 1, 0]
    # one living ray: its position is every extreme, and the squared distance from the axis a single term
    r = first + 256 + 64 + 17
    x, y, z = S.p[r, 3]
    assert rec[3, 7:13].tolist() == [x, x, y, y, z, z] and rec[3, 0] == S.w[r, 3]
    assert rec[3, 16] == (x - axis[3, 0]) ** 2 + (y - axis[3, 1]) ** 2
    # nobody alive: zeros, and no number for the extremes
    for i in (4, 5):
        assert rec[i, [0, 1, 4, 5, 6, 13, 14, 15, 16]].tolist() == [0] * 9 and np.all(np.isnan(rec[i, 7:13]))
    assert rec[5, 2] == 0 and rec[5, 3] == 0 and rec[4, 2] == S.w[r, 3]


def test_moments_all_rays_alive_everywhere():
    S, first, count = build(np.ones((700, 3), dtype=bool), 32, 4)
    _, rec = check_moments(S, first, count, random_axis(3, 4), "all alive")
    assert np.all(rec[:, [1, 3]] == 700) and np.all(np.isfinite(rec))


def test_count_zero_launches_nothing():
    S, first, count = build(np.ones((10, 3), dtype=bool), 0, 2)
    lib = _capi.load_library()
    rec = torch.full((3 * M,), -7.0, dtype=torch.float64, device=dev())
    ws = torch.zeros(8, dtype=torch.float64, device=dev())
    axis = to_dev(np.zeros(6), np.float64)
    _capi.check(lib.ot_footprint_moments(C.byref(S.rays), 10, 0, ptr(axis), ptr(ws), ptr(rec), stream_ptr()))
    _capi.check(lib.ot_footprint_maps(C.byref(S.rays), 10, 0, ptr(axis), ptr(rec), 4, ptr(ws), stream_ptr()))
    assert np.all(rec.cpu().numpy() == -7.0) and np.all(ws.cpu().numpy() == 0)


# ---- maps ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def map_case():
    """Four sections over 5000 rays (five workgroups of the histogram per section): dying rays | the same | all living rays ON the
    axis (R = 0) | none.  -> (Storage, first, count, axis, record on the device, record on the host)"""
    alive = dying(5000, 4, 5, keep=0.7)
    alive[:, 2] &= np.arange(5000) % 3 == 0
    S, first, count = build(alive, 9, 5)
    axis = random_axis(4, 5)
    on_axis = S.p[first:first + count, 2]
    on_axis[alive[:, 2], :2] = axis[2]
    S = Storage(S.p, S.w)  # (uploaded again with the moved rays)
    rec_d, rec = check_moments(S, first, count, axis, "map case")
    assert rec[2, 16] == 0 and rec[2, 1] > 100 and rec[3, 1] == 0 and rec[1, 1] > 1000
    return S, first, count, axis, rec_d, rec


@pytest.mark.parametrize("n_px", [1, 2, 7, 90, 91, 1024])  # 90^2 * 8 B fit into the 64 KiB of LDS the histogram takes, 91^2 * 8 B do not
def test_maps(n_px):
    assert (90 * 90 * 8 <= 64 * 1024 < 91 * 91 * 8)
    S, first, count, axis, rec_d, rec = map_case()
    got = call_maps(S, first, count, axis, rec_d, n_px)
    val, cnt = fc.maps(S.p, S.w, first, count, axis, rec, n_px)
    assert np.array_equal(cnt.sum(axis=(1, 2)), rec[:, 1]), "every living ray has one cell"
    assert np.all(got[cnt == 0] == 0), "a ray sits in a cell the formula does not put it in"
    err = np.abs(got.astype(LD) - val).astype(np.float64)
    bound = fc.sum_bound(cnt, val.astype(np.float64))
    assert np.all(err <= bound), f"cell sums: {np.count_nonzero(err > bound)} cells off, by up to {err.max():.3e}"
    totals = got.astype(LD).sum(axis=(1, 2))
    terr = np.abs(totals - rec[:, 0].astype(LD)).astype(np.float64)
    tbound = fc.sum_bound(rec[:, 1], rec[:, 0])
    print(f"n_px {n_px}: cells off by at most {err.max():.3e}, totals by {terr.max():.3e} of {tbound.max():.3e}")
    assert np.all(terr <= tbound), f"totals against slot 0: {terr} above {tbound}"
    # R = 0: all of the section in cell 0, 0; no living ray: an empty map
    assert got[2, 0, 0] > 0 and np.count_nonzero(got[2]) == 1 and not got[3].any()
    if n_px > 1:
        assert np.count_nonzero(got[0]) > 1


# ---- Raytracer.footprints on traced rays ------------------------------------------------------------------------------------------
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


def expected_axis(RT, source_index):
    surfaces = RT.tracing_surfaces
    return np.array([RT.ray_sources[source_index or 0].pos[:2]] + [s.pos[:2] for s in surfaces] + [[0, 0]], dtype=np.float64)


def check_footprints(RT, f, source_index, what):
    """Every field of `f` against the truth formed from the storage read back."""
    p, w = RT.rays.p_list, RT.rays.w_list
    nt = w.shape[1]
    first, end = (0, w.shape[0]) if source_index is None else (int(RT.rays.B_list[source_index]), int(RT.rays.B_list[source_index + 1]))
    axis = expected_axis(RT, source_index)
    assert np.array_equal(f.axis[:-1], axis[:-1]) and np.all(np.isfinite(f.axis[-1])) and len(f.labels) == nt and f.labels[-1] == "end"
    rec = f.records
    val, mag = fc.records(p, w, first, end - first, f.axis, centroid=fc.record_centroid(rec))
    fc.check_record(rec, val, mag, what)
    assert np.array_equal(rec[1:, 2:4], rec[:-1, 0:2]), "power_in[i] == power[i - 1]: the same sum over the same plane"
    assert rec[nt - 1, 1] == 0, "every ray ends absorbed"
    # the fields are the record's figures
    alive = rec[:, 1] > 0
    assert np.array_equal(f.N, rec[:, 1]) and np.array_equal(f.N_in, rec[:, 3])
    assert np.array_equal(f.power, rec[:, 0]) and np.array_equal(f.power_in, rec[:, 2]) and np.array_equal(f.loss, rec[:, 2] - rec[:, 0])
    assert np.array_equal(f.power_in[1:], f.power[:-1])
    with np.errstate(invalid="ignore", divide="ignore"):
        W = np.where(alive, rec[:, 0], np.nan)
        many = rec[:, 1] > 1
        eq = lambda a, b: np.array_equal(a, b, equal_nan=True)
        assert eq(f.transmission, np.where(rec[:, 3] > 0, rec[:, 0] / rec[:, 2], np.nan))
        assert eq(f.centroid, rec[:, 4:7] / W[:, None]) and eq(f.extent, rec[:, 7:13])
        assert eq(f.rms_x[many], np.sqrt(rec[many, 13] / W[many])) and eq(f.rms_y[many], np.sqrt(rec[many, 14] / W[many]))
        assert eq(f.cov_xy[many], rec[many, 15] / W[many]) and eq(f.rms_radius, np.sqrt(f.rms_x ** 2 + f.rms_y ** 2))
        assert eq(f.max_radius, np.where(alive, np.sqrt(rec[:, 16]), np.nan))
        assert f.total_transmission == rec[nt - 2, 0] / rec[0, 0]
    radii = [np.nan] + [np.hypot(*s.dim) / 2 if isinstance(s, ot.RectangularSurface) else s.r for s in RT.tracing_surfaces] + [np.nan]
    assert eq(f.surface_radius, np.array(radii, dtype=np.float64)) and eq(f.fill, f.max_radius / f.surface_radius)
    # the centroid lies within the extent, the beam within the lens surface it has just passed (to rounding; a ray that misses a
    # lens is absorbed, one that misses a filter or an aperture passes beside it: there `fill` may exceed 1)
    inside = alive & np.array([name.startswith("L") for name in f.labels])
    assert np.all(f.centroid[alive, 0] >= f.extent[alive, 0]) and np.all(f.centroid[alive, 0] <= f.extent[alive, 1])
    assert np.all(f.fill[inside] <= 1 + 1e-9), f"{what}: a beam wider than its surface: {f.fill}"


@pytest.mark.parametrize("name", ["c1_single_lens", "double_gauss", "mixed_geometry", "asphere"])
def test_footprints_of_traced_rays(name):
    """(lenses; lenses and a ring aperture, five sources; ring aperture, filter and ideal lens, two sources; filters, a slit)"""
    _, RT = traced(name)
    f = RT.footprints()
    check_footprints(RT, f, None, f"{name}, all rays")
    assert f.labels[0] == "sources" and f.maps is None and "all rays" in f.long_desc
    for k in range(len(RT.ray_sources)):
        fk = RT.footprints(source_index=k)
        check_footprints(RT, fk, k, f"{name}, source {k}")
        assert fk.labels[0] == f"RS{k}" and fk.N[0] == RT.rays.N_list[k]
    assert f.N[0] == RT.rays.N and f.N[0] == sum(RT.footprints(source_index=k).N[0] for k in range(len(RT.ray_sources)))


def test_labels_and_the_ring_aperture():
    _, RT = traced("double_gauss")
    f = RT.footprints()
    assert f.labels[:4] == ("sources", "L0 front", "L0 back", "L1 front") and f.labels[7] == "AP0" and f.labels[-2:] == ("L6 back", "end")
    i = 7  # the section behind the aperture, tracing surface 6
    ap = RT.tracing_surfaces[i - 1]
    assert isinstance(ap, ot.RingSurface) and f.surface_radius[i] == ap.r
    assert f.N[i] > 0 and f.max_radius[i] <= ap.ri + 1e-9
    assert f.loss[i] >= 0 and f.N_in[i] >= f.N[i]
    _, RT = traced("mixed_geometry")
    f = RT.footprints()
    i = 1 + next(k for k, s in enumerate(RT.tracing_surfaces) if isinstance(s, ot.RingSurface))
    assert f.labels[i] == "AP0" and f.max_radius[i] <= 0.01 + 1e-9 and f.N[i] < f.N_in[i]
    j = f.labels.index("F0")
    assert 0 < f.transmission[j] < 1 and 0 < f.N[j] <= f.N_in[j] and f.loss[j] > 0, "the filter takes power"


def lossless(N, **kw):
    RT = ot.Raytracer(outline=[-5, 5, -5, 5, -5, 30], **kw)
    RT.add(ot.RaySource(ot.CircularSurface(r=1), divergence="None", s=[0, 0, 1], pos=[0.25, -0.5, -2]))
    RT.add(ot.IdealLens(r=3, D=50, pos=[0, 0, 0]))
    with ot.global_options.no_warnings():
        RT.trace(N)
    return RT


def test_maps_and_a_lossless_scene():
    """Ideal lens, no filter, nothing clipped: everything the source emits is there behind the last surface."""
    N = 3000
    RT = lossless(N)
    f = RT.footprints(source_index=0, n_px=32)
    check_footprints(RT, f, 0, "lossless")
    assert f.labels == ("RS0", "L0", "end") and f.N.tolist() == [N, N, 0]
    # both powers are within (n + 40) eps sum of the same true sum
    assert abs(f.total_transmission - 1) <= 2 * (N + 40) * EPS * (1 + EPS) + EPS
    assert f.maps.shape == (3, 32, 32)
    p, w = RT.rays.p_list, RT.rays.w_list
    val, cnt = fc.maps(p, w, 0, N, f.axis, f.records, 32)
    assert np.all(f.maps[cnt == 0] == 0)
    assert np.all(np.abs(f.maps.astype(LD) - val).astype(np.float64) <= fc.sum_bound(cnt, val.astype(np.float64)))
    img = f.image(1)
    assert isinstance(img, ot.ScalarImage) and np.array_equal(img.data, f.maps[1])
    R, (ax, ay) = f.max_radius[1], f.axis[1]
    assert list(img.extent) == [ax - R, ax + R, ay - R, ay + R] and not f.maps[2].any()
    # the beam is the source's disc of radius 1 about (0.25, -0.5), seen from the lens' axis
    assert f.max_radius[1] <= np.hypot(0.25, 0.5) + 1 + 1e-9 and f.max_radius[0] <= 1 + 1e-9
    with pytest.raises(IndexError):
        RT.footprints(source_index=1)


def test_a_source_without_rays_gives_the_empty_result():
    RT = ot.Raytracer(outline=[-5, 5, -5, 5, -5, 30])
    RT.add(ot.RaySource(ot.CircularSurface(r=1), divergence="None", s=[0, 0, 1], pos=[0, 0, -2], power=1.0))
    RT.add(ot.RaySource(ot.CircularSurface(r=1), divergence="None", s=[0, 0, 1], pos=[0, 0, -1], power=1.0))
    RT.add(ot.IdealLens(r=3, D=50, pos=[0, 0, 0]))
    N = 400
    p0 = np.tile([0.1, 0.2, -2.0], (N, 1))
    s0 = np.tile([0.0, 0.0, 1.0], (N, 1))
    pol0 = np.tile([1.0, 0.0, 0.0], (N, 1))
    with ot.global_options.no_warnings():
        RT.trace(N, _initial_rays=(p0, s0, pol0, np.full(N, 1.0 / N), np.full(N, 550.0)), _N_list=[N, 0])
    assert RT.rays.N_list.tolist() == [N, 0]
    f = RT.footprints(source_index=1, n_px=4)
    assert f.N.tolist() == [0, 0, 0] and f.power.tolist() == [0, 0, 0] and f.N_in.tolist() == [0, 0, 0] and f.loss.tolist() == [0, 0, 0]
    for a in (f.centroid, f.extent, f.rms_x, f.rms_y, f.rms_radius, f.cov_xy, f.max_radius, f.fill, f.transmission):
        assert np.all(np.isnan(a))
    assert np.isnan(f.total_transmission) and f.maps.shape == (3, 4, 4) and not f.maps.any()
    g = RT.footprints(source_index=0)
    assert g.N.tolist() == [N, N, 0] and g.rms_radius[1] < 1e-12  # (all rays in one place)


def test_deferred_planes_are_neither_read_nor_filled():
    """A trace that generates its rays on the device leaves the index plane and the polarisation planes unwritten
    (OT_DEFER_INDEX | OT_DEFER_POL).  The footprints of such a storage, its unwritten planes poisoned, are those of the storage
    once it is complete, bit for bit, and asking for them fills nothing."""
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=7)
        RT.trace(20000)
    r = RT.rays
    assert r._pol_stale is not None and r._n_stale
    raw = lambda key: dict.__getitem__(r._dev, key)
    raw("n").fill_(float("nan"))
    raw("pol").fill_(float("nan"))
    before = RT.footprints(n_px=16)
    assert r._pol_stale is not None and r._n_stale, "the footprints filled a deferred plane"
    r._dev["n"], r._dev["pol"]  # (through the hook: the storage is complete now)
    assert r._pol_stale is None and not r._n_stale
    assert np.isfinite(raw("n")[:20000].cpu().numpy()).all()
    after = RT.footprints(n_px=16)
    assert np.array_equal(before.records.view(np.uint64), after.records.view(np.uint64))
    check_footprints(RT, after, None, "device-generated double Gauss")
    assert np.allclose(before.maps, after.maps, rtol=1e-12, atol=0)
