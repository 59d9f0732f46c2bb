"""Raytracer.spot_diagram and the `ot_spotdiag_*` entry points on the GPU.

Truth is NumPy following the definition (tests/spot_diagram_cases.py): on synthetic storages handed to the entry points through
ctypes -- the storages of tests/test_gpu_field.py --, and on the device's own ray storage read back for traced scenes.

Bounds, as stated with the feature: the cell of every ray and the counts are exact; a cell's power within (n_cell + 2) eps of it;
max |e|^2 the oracle's bits, sum w |e|^2 within (n + 40) eps of the sum of its terms; the power of a tile, binned and outside,
slot 0 of the record within (n + 40) eps of it; extents and counts the same bits on a second call, and those of a field alone the
ones it has among others."""
import ctypes as C

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd._device import ptr, stream_ptr, to_dev
from optrace_amd.scene import SectionTable

import chromatic_cases as cc
import field_cases as fc
import scenes
import spot_diagram_cases as sc
from test_gpu_field import Storage, build, dev, double_gauss, flat_ranges, ideal_scene, same_bits

pytestmark = pytest.mark.gpu

EPS = sc.EPS
ORIGIN = (0.25, -0.5, 9.5)


def band_centres(rec, zeta):
    """(slot 2..3 + zeta slot 4..5) / slot 0 of every cell in f64: (F, K, Z, 2), NaN without a ray."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return (rec[:, :, None, 2:4] + np.asarray(zeta)[None, None, :, None] * rec[:, :, None, 4:6]) / rec[:, :, None, 0:1]


def call_spot(S, fields, k, key, key_first, K, zeta, n_px, size, centre=None, origin=ORIGIN):
    """`ot_field_sums`, then the two passes about the band centroids of its records (or `centre`).  -> dict of host arrays"""
    lib = _capi.load_library()
    F, Z = len(fields), len(zeta)
    flat, d_key, org = flat_ranges(fields), to_dev(key, np.uint8), (C.c_double * 3)(*origin)
    ws = torch.full((lib.ot_field_workspace(flat, F, K),), np.nan, dtype=torch.float64, device=dev())
    rec = torch.full((F * K * fc.M,), -7.0, dtype=torch.float64, device=dev())
    _capi.check(lib.ot_field_sums(C.byref(S.rays), flat, F, k, ptr(d_key), key_first, K, org, ptr(ws), ptr(rec), stream_ptr()))
    rec = rec.cpu().numpy().reshape(F, K, fc.M)
    centre = band_centres(rec, zeta) if centre is None else np.asarray(centre, dtype=np.float64)
    d_centre, c_zeta = to_dev(np.ascontiguousarray(centre).reshape(-1), np.float64), (C.c_double * Z)(*zeta)
    n_ws = lib.ot_spotdiag_workspace(flat, F, K, Z)
    assert n_ws == sc.workspace([n for _, n in fields], K, Z)
    ws = torch.full((n_ws,), np.nan, dtype=torch.float64, device=dev())  # (a partial read before it is written shows)
    ext = torch.full((F * K * Z * 2,), -7.0, dtype=torch.float64, device=dev())
    _capi.check(lib.ot_spotdiag_extent(C.byref(S.rays), flat, F, k, ptr(d_key), key_first, K, org, ptr(d_centre), c_zeta, Z, ptr(ws),
                                       ptr(ext), stream_ptr()))
    maps = torch.zeros(F * K * Z * n_px * n_px, dtype=torch.float64, device=dev())
    counts = torch.zeros(F * K * Z * 2, dtype=torch.int64, device=dev())
    outp = torch.zeros(F * K * Z, dtype=torch.float64, device=dev())
    _capi.check(lib.ot_spotdiag_maps(C.byref(S.rays), flat, F, k, ptr(d_key), key_first, K, org, ptr(d_centre), c_zeta, Z, n_px, size,
                                     ptr(maps), ptr(counts), ptr(outp), stream_ptr()))
    return dict(rec=rec, centre=centre, ext=ext.cpu().numpy().reshape(F, K, Z, 2), maps=maps.cpu().numpy().reshape(F, K, Z, n_px, n_px),
                counts=counts.cpu().numpy().reshape(F, K, Z, 2), outside=outp.cpu().numpy().reshape(F, K, Z))


def check_entry_points(S, fields, k, key, key_first, K, Z, n_px, size, what, alone=None, centre=None):
    """-> the device's arrays, checked against the oracle; twice the same bits in extents and counts; the fields `alone` (default:
    all with rays), each on its own, give the extents and counts they have among the others; a tile's power against the record."""
    zeta = np.array([0.75]) if Z == 1 else np.linspace(-1.5, 2.0, Z)
    got = call_spot(S, fields, k, key, key_first, K, zeta, n_px, size, centre)
    again = call_spot(S, fields, k, key, key_first, K, zeta, n_px, size, centre)
    assert same_bits(got["ext"], again["ext"]) and np.array_equal(got["counts"], again["counts"]), f"{what}: two calls differ"
    want = sc.diagram(S.p, S.w, fields, k, key, key_first, K, ORIGIN, got["centre"], zeta, n_px, size)
    assert np.array_equal(want["n"], got["rec"][:, :, 1])
    sc.check_maps(got["maps"], got["counts"], got["outside"], want, what)
    sc.check_extents(got["ext"], want, what)
    n, W = want["n"][:, :, None], got["rec"][:, :, 0:1]
    assert np.array_equal(got["counts"].sum(axis=-1), np.broadcast_to(n, got["outside"].shape)), f"{what}: binned and outside are all rays"
    total = got["maps"].sum(axis=(-1, -2)) + got["outside"]
    assert np.all(np.abs(total - W) <= (n + 40) * EPS * W), f"{what}: the power of a tile against the record"
    if len(fields) > 1:
        for f in (range(len(fields)) if alone is None else alone):
            if fields[f][1]:
                one = call_spot(S, [fields[f]], k, key, key_first, K, zeta, n_px, size, None if centre is None else centre[f:f + 1])
                assert same_bits(got["ext"][f], one["ext"][0]) and np.array_equal(got["counts"][f], one["counts"][0]), \
                    f"{what}: field {f} alone differs"
    return got


@pytest.mark.parametrize("counts,gaps,nt,k,first,K,Z,n_px,size", [
    ([1], None, 2, 0, 5, 1, 1, 1, 1.0),                              # one ray
    ([63, 64, 65], None, 5, 3, 5, 3, 2, 7, 6.0),                     # around a wave; an odd grid
    ([65, 255, 256], [0, 7, 0], 2, 0, 33, 32, 65, 2, 4.0),           # around a workgroup, every band, the most planes, one chunk
    ([257, 0, 3000], [5, 0, 11], 5, 3, 7, 3, 3, 64, 9.0),            # a field of no rays between two; three chunks
    ([300, 65], [2, 0], 5, 3, 9, 5, 1, 5, 5.0),                      # two groups of bands, the second of one band
    ([256 * 1024 + 1, 65], [3, 0], 2, 0, 7, 3, 1, 8, 7.0),           # more rays than a field's launch has lanes
    ([3000], None, 5, 3, 64, 1, 1, 300, 8.0),                        # one tile beyond the LDS: cells added to global memory
])
def test_entry_points_on_random_planes(counts, gaps, nt, k, first, K, Z, n_px, size):
    seed = sum(counts) + 7 * nt + K
    S, fields, key, key_first = build(counts, nt, k, first, K, seed, gaps=gaps)
    got = check_entry_points(S, fields, k, key, key_first, K, Z, n_px, size,
                             f"fields of {counts} rays, nt {nt}, section {k}, {K} bands, {Z} planes, {n_px}^2 cells")
    assert got["counts"][..., 1].sum() > 0 or sum(counts) == 1  # (rays fall outside these tiles: that branch is walked)
    assert _capi.load_library().ot_spotdiag_chunks(K, Z, n_px) == sc.chunks(K, Z, n_px)[0]
    assert sc.chunks(K, Z, n_px)[1] == (n_px != 300)


def test_several_chunks_and_tiles_drawn_about_given_points():
    """Three bands, five planes, 64 x 64 cells: four tiles fit the LDS of a workgroup, the fifteen of a field go in four chunks, and a
    band's planes straddle two of them.  The centres are points of the caller's here, a NaN among them: all rays of that tile
    lie outside."""
    K, Z, n_px = 3, 5, 64
    assert _capi.load_library().ot_spotdiag_chunks(K, Z, n_px) == 4 and sc.chunks(K, Z, n_px) == (4, True)
    assert sc.chunks(32, 65, 2) == (1, True) and sc.chunks(1, 1, 142) == (1, True) and sc.chunks(2, 2, 143) == (1, False)
    S, fields, key, key_first = build([3000, 700], 3, 1, 16, K, 5, far=False)
    rng = np.random.default_rng(9)
    centre = rng.normal(size=(2, K, Z, 2)) * 0.5 + [0.3, 0.2]
    centre[1, 2, 3] = np.nan
    got = check_entry_points(S, fields, 1, key, key_first, K, Z, n_px, 12.0, "four chunks", centre=centre)
    assert got["counts"][1, 2, 3, 0] == 0 and got["counts"][1, 2, 3, 1] == got["rec"][1, 2, 1] > 50 and np.all(got["maps"][1, 2, 3] == 0)


def test_sixty_four_fields_and_the_last_ends_with_the_storage():
    counts = [(37 * f) % 131 + (f % 3 == 0) for f in range(64)]
    S, fields, key, key_first = build(counts, 4, 2, 13, 3, 8, gaps=[(f + 1) % 2 for f in range(64)], behind=0)
    assert fields[-1][0] + fields[-1][1] == S.N and any(a % 16 for a, _ in fields)
    check_entry_points(S, fields, 2, key, key_first, 3, 3, 6, 5.0, "64 fields", alone=(1, 17, 63))


def test_no_ray_in_any_field_launches_nothing():
    S, fields, key, key_first = build([10], 3, 0, 0, 2, 2)
    lib = _capi.load_library()
    out = torch.full((2 * 2 * 4 * 4,), -7.0, dtype=torch.float64, device=dev())
    cnt = torch.full((2 * 2 * 2,), -7, dtype=torch.int64, device=dev())
    ws = torch.zeros(256, dtype=torch.float64, device=dev())
    d_key = to_dev(key, np.uint8)
    head = (C.byref(S.rays), flat_ranges([(10, 0), (3, 0)]), 2, 0, ptr(d_key), 0, 2, (C.c_double * 3)(0, 0, 0), ptr(ws), (C.c_double * 1)(0.5), 1)
    _capi.check(lib.ot_spotdiag_extent(*head, ptr(ws), ptr(out), stream_ptr()))
    _capi.check(lib.ot_spotdiag_maps(*head, 4, 1.0, ptr(out), ptr(cnt), ptr(out), stream_ptr()))
    assert np.all(out.cpu().numpy() == -7.0) and np.all(cnt.cpu().numpy() == -7) and np.all(ws.cpu().numpy() == 0)


# ---- edges of the cells ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shift", [0, -1, -3])
def test_rays_on_the_edges_of_the_cells(shift):
    """m = 0, a on the grid j / 8 (scaled by 2^shift with the tile), centre 0, size = n_px / 8 * 2^shift: e * scale + half is the exact
    integer j + n_px / 2 for every ray.  Every ray sits in exactly that cell: the ray at -size / 2 in cell 0, the one at +size / 2
    outside.  Beside them a ray of NaN positions and positive weight, which is no used ray, and one with d_z = 0, slot 7 of the
    record: they enter nothing."""
    n_px, s = 8, 2.0 ** shift
    j = np.arange(-6, 7)
    jx, jy = [v.ravel() for v in np.meshgrid(j, j)]
    n = jx.shape[0] + 2
    p = np.zeros((n, 2, 3))
    p[:-2, 0, 0] = p[:-2, 1, 0] = jx / 8 * s
    p[:-2, 0, 1] = p[:-2, 1, 1] = jy / 8 * s
    p[:, 1, 2] = 1.0
    p[-2] = np.nan
    p[-1, 1] = [0.25, 0.0, 0.0]  # (a length, and d_z = 0)
    w = np.full((n, 2), 0.5, dtype=np.float32)
    w[:-2, 0] = np.linspace(0.1, 1.0, n - 2)
    S = Storage(p, w, np.full(n, 550.0, dtype=np.float32))
    key = np.zeros(n, dtype=np.uint8)
    size = n_px / 8 * s
    got = call_spot(S, [(0, n)], 0, key, 0, 1, np.array([0.5]), n_px, size, centre=np.zeros((1, 1, 1, 2)), origin=(0.0, 0.0, 0.0))
    assert got["rec"][0, 0, 1] == n - 2 and got["rec"][0, 0, 7] == 1
    want = np.zeros((n_px, n_px), dtype=np.float32)
    inside = (jx >= -4) & (jx < 4) & (jy >= -4) & (jy < 4)
    want[jy[inside] + 4, jx[inside] + 4] = w[:-2, 0][inside]  # (one ray per cell)
    assert np.array_equal(got["maps"][0, 0, 0], want.astype(np.float64)), "a ray in another cell than its own"
    assert got["maps"][0, 0, 0, 0, 0] == w[:-2, 0][(jx == -4) & (jy == -4)][0]  # (-size / 2: cell 0)
    assert got["counts"][0, 0, 0].tolist() == [64, n - 2 - 64]
    assert got["outside"][0, 0, 0] == pytest.approx(w[:-2, 0][~inside].astype(np.float64).sum(), rel=(n + 2) * EPS)
    assert got["ext"][0, 0, 0, 0] == 2 * (6 / 8 * s) ** 2
    oracle = sc.diagram(p, w, [(0, n)], 0, key, 0, 1, (0.0, 0.0, 0.0), got["centre"], [0.5], n_px, size)
    sc.check_maps(got["maps"], got["counts"], got["outside"], oracle, "edges")
    sc.check_extents(got["ext"], oracle, "edges")


# ---- Raytracer.spot_diagram on traced rays ---------------------------------------------------------------------------------------------
def check_diagram(RT, sd, sources, section, bands, what):
    """`sd` against the truth formed from the storage read back, about the centres the device was given.  -> the oracle's dict"""
    p, w, wl = RT.rays.p_list, RT.rays.w_list, RT.rays.wl_list
    nt = w.shape[1]
    k = nt - 2 if section is None else section
    fields = [(int(RT.rays.B_list[s]), int(RT.rays.B_list[s + 1] - RT.rays.B_list[s])) for s in sources]
    origin = np.array(SectionTable(RT).origin(k, None), dtype=np.float64)
    used = np.zeros(w.shape[0], dtype=bool)
    for first, count in fields:
        used[first:first + count] = cc.used_rays(p, w, first, count, k)[0]
    key, K, edges = cc.band_keys(wl, used, bands)
    assert sd.n_bands == K and sd.section == k and sd.n_fields == len(sources) and sd.sources.tolist() == list(sources)
    assert np.array_equal(sd.origin, origin) and (sd.band_edges is None if edges is None else np.array_equal(sd.band_edges, edges))
    want = sc.diagram(p, w, fields, k, key, 0, K, origin, sd.centre_rel, sd.planes - origin[2], sd.n_px, sd.size)
    assert np.array_equal(want["n"], sd.band_N)
    sc.check_maps(sd.power, np.stack([sd.N, sd.outside_N], axis=-1), sd.outside_power, want, what)
    sc.check_extents(sd.extents, want, what)
    some = sd.band_N[:, :, None] > 0
    assert np.array_equal(sd.geo_radius[np.broadcast_to(some, sd.N.shape)], np.sqrt(want["r2max"])[np.broadcast_to(some, sd.N.shape)])
    assert np.all(np.isnan(sd.geo_radius[~np.broadcast_to(some, sd.N.shape)])) and np.array_equal(sd.power_all, sd.power.sum(axis=1))
    return want


def test_an_ideal_lens_puts_every_field_into_the_centre_cell_of_its_image_plane():
    with ot.global_options.no_warnings():
        RT = ideal_scene()
        RT.trace(6000)
    image_z = RT.tma(550.0).image_position(-30.0)
    dz = np.array([-0.2, -0.1, 0.0, 0.1, 0.2])
    sd = RT.spot_diagram(z=image_z, dz=dz, n_px=9, size=0.05)
    assert (sd.n_fields, sd.n_bands, sd.n_planes, sd.n_px, sd.size) == (3, 1, 5, 9, 0.05) and np.all(sd.band_N[:, 0] == 2000)
    assert np.array_equal(sd.planes, image_z + dz) and "RS0, RS1, RS2" in sd.long_desc
    check_diagram(RT, sd, [0, 1, 2], None, "lines", "ideal lens")
    assert np.all(sd.outside_N == 0) and np.all(sd.N == 2000)
    on_image = sd.power[:, 0, 2]
    assert np.all(on_image[:, 4, 4] == on_image.sum(axis=(1, 2))) and np.all(on_image[:, 4, 4] > 0)  # (all power in the centre cell)
    g = sd.geo_radius[:, 0]
    print(f"ideal lens: geo_radius {g}")
    assert np.all(g[:, 0] > g[:, 1]) and np.all(g[:, 1] > g[:, 2]) and np.all(g[:, 2] < g[:, 3]) and np.all(g[:, 3] < g[:, 4])
    # (a cone through one point: the radius grows in proportion to |dz|, the same on either side)
    assert np.all(g[:, 2] < 1e-9) and np.allclose(g[:, [0, 4]], 2 * g[:, [1, 3]], rtol=1e-9) and np.allclose(g[:, 0], g[:, 4], rtol=1e-9)
    # the default size: no ray outside, on the device and by the oracle alike; the default plane is the field analysis's
    se = RT.spot_diagram(dz=dz, n_px=8)
    want = check_diagram(RT, se, [0, 1, 2], None, "lines", "ideal lens, default size")
    assert np.all(se.outside_N == 0) and np.all(want["outside_N"] == 0) and se.size == sc.SIZE_FACTOR * se.geo_radius.max()
    fa = RT.field_analysis()
    assert se.z == fa.z and same_bits(se.records, fa.records)


def test_double_gauss_three_fields_three_lines_five_planes():
    RT = double_gauss()
    fa = RT.field_analysis(sources=[0, 1, 2])
    dz = np.array([-0.4, -0.15, 0.0, 0.2, 0.5])
    sd = RT.spot_diagram(sources=[0, 1, 2], dz=dz, n_px=33)
    want = check_diagram(RT, sd, [0, 1, 2], None, "lines", "double Gauss, sources 0 1 2")
    assert sd.n_bands == 3 and sd.reference_band == 1 and sd.z == fa.z and same_bits(sd.records, fa.records)
    assert np.array_equal(sd.planes, fa.z + dz) and np.array_equal(sd.band_N, fa.band_N)
    assert np.all(sd.outside_N == 0) and np.all(want["outside_N"] == 0) and sd.size == sc.SIZE_FACTOR * np.nanmax(sd.geo_radius)
    # one centre for all bands of a field and plane: the band tiles of an off-axis field lie apart by the differences of their
    # centroids -- the power-weighted mean cell position against `fa.centroid`, to one cell
    assert np.all(sd.centre[:, 0] == sd.centre[:, 1]) and np.all(sd.centre[:, 0] == sd.centre[:, 2])
    at = (np.arange(33) + 0.5) / 33 - 0.5
    W = sd.power[:, :, 2].sum(axis=(-1, -2))
    mean_x = sd.centre[:, :, 2, 0] + sd.size * (sd.power[:, :, 2].sum(axis=-2) * at).sum(axis=-1) / W
    mean_y = sd.centre[:, :, 2, 1] + sd.size * (sd.power[:, :, 2].sum(axis=-1) * at).sum(axis=-1) / W
    print(f"double Gauss: lateral colour of field 2 {fa.centroid[2, :, 1] - fa.centroid[2, 1, 1]}, cell {sd.size / 33}")
    assert np.all(np.abs(mean_x - fa.centroid[:, :, 0]) <= sd.size / 33) and np.all(np.abs(mean_y - fa.centroid[:, :, 1]) <= sd.size / 33)
    # the order of the sources is the order of the result
    sb = RT.spot_diagram(sources=[2, 0], dz=dz, z=sd.z, n_px=33, size=sd.size)
    assert sb.sources.tolist() == [2, 0] and np.array_equal(sb.field, sd.field[[2, 0]], equal_nan=True)
    for mine, theirs in ((0, 2), (1, 0)):
        assert same_bits(sb.extents[mine], sd.extents[theirs]) and np.array_equal(sb.N[mine], sd.N[theirs])
        assert same_bits(sb.centre[mine], sd.centre[theirs])
        allow = (want["n_cell"][theirs] + 2) * EPS * want["power"][theirs].astype(np.float64)
        assert np.all(np.abs(sb.power[mine] - sd.power[theirs]) <= 2 * allow)  # (each within its allowance of the truth)
    # every band about its own centroid: the RMS radius of the field analysis, within the rounding of the quadratic it evaluates
    sc_ = RT.spot_diagram(sources=[0, 1, 2], centre="band", n_px=16)
    check_diagram(RT, sc_, [0, 1, 2], None, "lines", "double Gauss, centre band")
    rec, zeta = fa.records, fa.z - fa.origin[2]
    bound = EPS * (rec[:, :, 1] + 40) * (rec[:, :, 8] + rec[:, :, 10] + 2 * abs(zeta) * (np.abs(rec[:, :, 11]) + np.abs(rec[:, :, 14]))
                                          + zeta ** 2 * (rec[:, :, 15] + rec[:, :, 17])) / rec[:, :, 0]
    apart = np.abs(sc_.rms_radius[:, :, 0] ** 2 - fa.rms_radius ** 2)
    print(f"double Gauss: rms_radius^2 against the field analysis off by at most {apart.max():.3e}, allowed {bound.min():.3e}")
    assert np.all(apart <= bound) and np.array_equal(sc_.centre[:, :, 0], fa.centroid) and np.all(sc_.outside_N == 0)
    # the centroid of the reference band; an array of points
    sr = RT.spot_diagram(sources=[0, 1, 2], centre="reference", n_px=16)
    assert np.array_equal(sr.centre[:, 0, 0], fa.centroid[:, 1]) and np.array_equal(sr.centre[:, 2, 0], fa.centroid[:, 1])
    points = fa.centroid[:, 1] + [0.001, -0.002]
    sp = RT.spot_diagram(sources=[0, 1, 2], centre=points, dz=[-0.1, 0.1], n_px=16)
    check_diagram(RT, sp, [0, 1, 2], None, "lines", "double Gauss, centre given")
    assert np.all(np.abs(sp.centre - points[:, None, None, :]) <= 4 * EPS * (np.abs(points[:, None, None, :]) + np.abs(sp.origin[:2])))
    assert np.all(sp.outside_N == 0)
    # an earlier section, bands as edges, one plane
    edges = np.array([450.0, 550, 600, 700])
    se = RT.spot_diagram(sources=[1, 3], section=3, bands=edges, z=0.0, n_px=12)
    want = check_diagram(RT, se, [1, 3], 3, edges, "double Gauss, section 3, edges")
    assert np.all(se.outside_N == 0) and np.all(want["outside_N"] == 0)
    img = se.image(1, 0, 2)
    assert img.shape == (12, 12) and np.allclose(img.extent, [se.centre[1, 2, 0, 0] - se.size / 2, se.centre[1, 2, 0, 0] + se.size / 2,
                                                              se.centre[1, 2, 0, 1] - se.size / 2, se.centre[1, 2, 0, 1] + se.size / 2])


def test_deferred_planes_are_neither_read_nor_filled():
    """A trace that generates its rays on the device leaves the index plane and the polarisation planes unwritten.  The spot diagram
    of such a storage, its unwritten planes poisoned, is that of the storage once it is complete -- counts and extents bit for
    bit --, and asking for it fills nothing."""
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=11)
        RT.trace(20000)
    r = RT.rays
    assert r._pol_stale is not None and r._n_stale
    raw = lambda key: dict.__getitem__(r._dev, key)
    raw("n").fill_(float("nan"))
    raw("pol").fill_(float("nan"))
    before = RT.spot_diagram(sources=[0, 2, 4], dz=[-0.1, 0.0, 0.1], n_px=20)
    assert r._pol_stale is not None and r._n_stale, "the spot diagram filled a deferred plane"
    r._dev["n"], r._dev["pol"]  # (through the hook: the storage is complete now)
    assert r._pol_stale is None and not r._n_stale
    after = RT.spot_diagram(sources=[0, 2, 4], dz=[-0.1, 0.0, 0.1], n_px=20)
    assert same_bits(before.extents, after.extents) and np.array_equal(before.N, after.N) and before.z == after.z and before.size == after.size
    assert before.n_bands == 3 and np.all(after.outside_N == 0)
    check_diagram(RT, after, [0, 2, 4], None, "lines", "device-generated double Gauss")


def test_a_source_without_rays():
    RT = ot.Raytracer(outline=[-5, 5, -5, 5, -5, 30])
    RT.add(ot.RaySource(ot.CircularSurface(r=1), divergence="None", s=[0, 0, 1], pos=[0, 0, -2], power=1.0))
    RT.add(ot.RaySource(ot.CircularSurface(r=1), divergence="None", s=[0, 0, 1], pos=[0, 0, -1], power=1.0))
    RT.add(ot.Lens(ot.SphericalSurface(r=3, R=8), ot.SphericalSurface(r=3, R=-8), de=0.1, n=ot.RefractionIndex("Constant", n=1.5),
                   pos=[0, 0, 0]))
    N = 400
    rng = np.random.default_rng(1)
    p0 = np.concatenate([rng.uniform(-0.5, 0.5, size=(N, 2)), np.full((N, 1), -2.0)], axis=1)
    s0 = np.tile([0.0, 0.0, 1.0], (N, 1))
    pol0 = np.tile([1.0, 0.0, 0.0], (N, 1))
    with ot.global_options.no_warnings():
        RT.trace(N, _initial_rays=(p0, s0, pol0, np.full(N, 1.0 / N), np.full(N, 550.0)), _N_list=[N, 0])
    assert RT.rays.N_list.tolist() == [N, 0]
    sd = RT.spot_diagram(dz=[-0.5, 0.0, 0.5], n_px=10)
    assert sd.band_N[:, 0].tolist() == [N, 0] and np.all(sd.N[0] == N) and np.all(sd.outside_N == 0) and 5 < sd.z < 12
    assert np.all(sd.power[1] == 0) and np.all(sd.N[1] == 0) and np.all(sd.outside_power[1] == 0)
    assert np.all(np.isnan(sd.geo_radius[1])) and np.all(np.isnan(sd.rms_radius[1])) and np.all(np.isnan(sd.centre[1]))
    assert np.all(np.isfinite(sd.rms_radius[0])) and np.all(sd.rms_radius[0] <= sd.geo_radius[0])
    check_diagram(RT, sd, [0, 1], None, "lines", "a source without rays")
    with pytest.raises(ValueError, match="no ray"):
        sd.image(1, 0, 0)
    # the reference field has no ray: no default plane; with a plane, the other field still gives the scale
    with pytest.raises(RuntimeError, match="pass `z`"):
        RT.spot_diagram(reference_field=1)
    assert RT.spot_diagram(reference_field=1, z=8.0).size > 0
    # the centroid of a band without a ray in the field: no centre, and with no ray anywhere about a centre no scale
    with pytest.raises(ValueError, match="pass `size`"):
        RT.spot_diagram(sources=[0], z=8.0, centre=np.array([[1e200, 0.0]]), n_px=4)
    # no chosen ray at all: the empty result, what the caller fixed stays
    e = RT.spot_diagram(sources=[1], bands=np.array([400.0, 500, 600]), z=3.0, dz=[0.0, 1.0], n_px=5, size=0.5)
    assert e.n_bands == 2 and e.z == 3.0 and e.reference_band == -1 and e.band_N.tolist() == [[0, 0]] and e.sources.tolist() == [1]
    assert e.planes.tolist() == [3.0, 4.0] and e.size == 0.5 and e.power.shape == (1, 2, 2, 5, 5) and np.all(e.power == 0)
    assert e.N.shape == (1, 2, 2) and np.all(np.isnan(e.centre)) and np.all(np.isnan(e.geo_radius)) and e.power_all.shape == (1, 2, 5, 5)
    e = RT.spot_diagram(sources=[1])
    assert e.n_bands == 1 and np.isnan(e.z) and e.band_edges is None and np.isnan(e.size) and e.power.shape == (1, 1, 1, 64, 64)
    assert RT.spot_diagram(bands=np.array([600.0, 700]), z=5.0, size=1.0).band_N.sum() == 0
