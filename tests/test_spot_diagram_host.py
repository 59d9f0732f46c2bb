"""Raytracer.spot_diagram without a device: the oracle (tests/spot_diagram_cases.py) against `np.histogram2d` and on the edges of the
cells, the factor of the default size on the reference side, the host arithmetic of `ot.SpotDiagram` on hand-made arrays, its
images, and the argument checks."""
import pathlib
import re

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd import mtf
from optrace_amd import spot_diagram as sdm

import spot_diagram_cases as sc

EPS, LD, NAN = sc.EPS, sc.LD, float("nan")


# ---- the oracle ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_px,size", [(1, 3.0), (7, 2.5), (64, 0.01), (33, 1e6)])
def test_the_oracle_against_histogram2d_on_points_away_from_the_edges(n_px, size):
    """Points drawn inside their cells, at least a thousandth of a cell from every edge, some of them in cells outside the tile: the
    two ways of finding a cell agree wherever rounding cannot matter."""
    rng = np.random.default_rng(n_px)
    n = 5000
    cell = rng.integers(-2, n_px + 2, size=(n, 2))
    e = ((cell + rng.uniform(0.001, 0.999, size=(n, 2))) / n_px - 0.5) * size
    wt = rng.uniform(0.1, 1.0, size=n).astype(np.float32)
    one = sc.tile(e, wt, n_px, size)
    inside = np.all((cell >= 0) & (cell < n_px), axis=1)
    assert one["N"] == np.count_nonzero(inside) and one["outside_N"] == n - one["N"] and 0 < one["N"] < n
    edges = np.linspace(-size / 2, size / 2, n_px + 1)
    hist, _, _ = np.histogram2d(e[inside, 1], e[inside, 0], bins=[edges, edges], weights=wt[inside].astype(np.float64))  # [row = y][column = x]
    count, _, _ = np.histogram2d(e[inside, 1], e[inside, 0], bins=[edges, edges])
    assert np.array_equal(one["n_cell"], count.astype(np.int64))
    assert np.all(np.abs(one["power"].astype(np.float64) - hist) <= (count + 2) * EPS * hist)
    assert abs(float(one["outside_power"]) - wt[~inside].astype(np.float64).sum()) <= (n + 2) * EPS * wt.sum()
    r2 = (e.astype(LD) ** 2).sum(axis=1)
    assert abs(one["r2max"] - float(r2.max())) <= 4 * EPS * one["r2max"]
    assert abs(float(one["wr2"] - (wt.astype(LD) * r2).sum())) <= 8 * EPS * float(one["wr2_mag"])


def test_the_oracle_on_the_edges_of_the_cells():
    """e on the grid j / 8 with size = n_px / 8 * 2^k: e * scale + half is an exact integer.  -size / 2 lies in cell 0, +size / 2
    outside; what is no number lies outside."""
    n_px = 8
    for shift in (0, -1, -4):
        s = 2.0 ** shift
        j = np.arange(-6, 7)
        e = np.stack([j / 8 * s, np.zeros(13)], axis=1)
        inside, col, row = sc.cells_of(e, n_px, n_px / 8 * s)
        assert inside.tolist() == [bool(-4 <= v < 4) for v in j] and col[inside].tolist() == list(range(8)) and np.all(row[inside] == 4)
    e = np.array([[NAN, 0.0], [0.0, NAN], [np.inf, 0.0], [0.0, -np.inf], [0.0, 0.0]])
    one = sc.tile(e, np.ones(5, dtype=np.float32), 3, 1.0)
    assert one["N"] == 1 and one["outside_N"] == 4 and one["power"][1, 1] == 1 and one["outside_power"] == 4 and one["r2max"] == np.inf
    assert sc.offsets(np.array([[1.0, 2.0, 0.5, -0.25]]), (0.25, 0.5), 2.0).tolist() == [[1.75, 1.0]]


@pytest.mark.parametrize("n_px", [1, 2, 3, 7, 64, 1000, 1024])
def test_the_default_size_leaves_no_ray_outside_by_the_oracle(n_px):
    """size = SIZE_FACTOR * sqrt(max |e|^2), the maximum formed as the device forms it: by the arithmetic of the definition no ray lies
    outside -- points on the circle of the largest radius, on the axes and on the diagonals, and at every scale."""
    rng = np.random.default_rng(n_px)
    for scale in (1e-150, 1e-9, 1.0, 3.7e5, 1e150):
        ang = np.concatenate([rng.uniform(0, 2 * np.pi, 2000), np.arange(8) * np.pi / 4])
        rad = np.concatenate([np.ones(1000), rng.uniform(0, 1, 1000), np.ones(8)])
        e = np.stack([rad * np.cos(ang), rad * np.sin(ang)], axis=1) * scale
        e = np.concatenate([e, [[scale, 0], [-scale, 0], [0, scale], [0, -scale]]])
        r2max = np.fmax.reduce(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
        size = sc.SIZE_FACTOR * np.sqrt(r2max)
        inside, col, row = sc.cells_of(e, n_px, size)
        assert np.all(inside), f"{np.count_nonzero(~inside)} points outside at scale {scale}"
        assert col.min() == 0 and col.max() == n_px - 1 and size <= 2 * np.sqrt(r2max) * (1 + 1e-9)
    assert sdm.SIZE_FACTOR == sc.SIZE_FACTOR


def test_mirrors_of_the_launch_shapes():
    assert sc.workspace([1], 1, 1) == 16 and sc.workspace([257], 3, 5) == 2 * 2 * 18 and sc.workspace([300], 5, 1) == 2 * 2 * 16
    assert sc.chunks(3, 5, 64) == (4, True) and sc.chunks(32, 65, 2) == (1, True) and sc.chunks(32, 65, 1024) == (1, False)
    assert sc.chunks(1, 1, 142) == (1, True) and sc.chunks(1, 1, 143) == (1, False) and sc.chunks(32, 65, 16) == (28, True)


# ---- ot.SpotDiagram on hand-made arrays ----------------------------------------------------------------------------------------------
def hand_made(F=2, K=3, Z=2, n_px=4, size=0.5, empty=((1, 2),)):
    rng = np.random.default_rng(3)
    rec = np.zeros((F, K, _capi.FIELD_M))
    rec[:, :, 0] = rng.uniform(1, 2, size=(F, K))
    rec[:, :, 1] = rng.integers(5, 50, size=(F, K))
    rec[:, :, 6] = rec[:, :, 0] * np.array([486.0, 589.0, 656.0])[:K]
    rec[:, :, 2:6] = rng.normal(size=(F, K, 4)) * rec[:, :, 0:1]
    power = rng.uniform(0, 1, size=(F, K, Z, n_px, n_px))
    counts = np.stack([np.repeat(rec[:, :, 1, None], Z, axis=2) - 1, np.ones((F, K, Z))], axis=-1)
    outside = rng.uniform(0, 0.1, size=(F, K, Z))
    ext = rng.uniform(0.01, 0.04, size=(F, K, Z, 2))
    for f, b in empty:
        rec[f, b, :8], rec[f, b, 8:] = 0, NAN
        power[f, b], counts[f, b], outside[f, b], ext[f, b] = 0, 0, 0, 0
    origin, planes = np.array([0.25, -0.5, 9.5]), 12.0 + np.linspace(-0.1, 0.1, Z)
    rel = sdm.centres(rec, planes - origin[2], "band", 1, origin[:2])
    sd = ot.SpotDiagram(power, counts, outside, ext, rel, rec, origin, 12.0, planes, n_px, size, 1, 0, 3, list(range(F)),
                        [[0, 0], [0, 1.5]][:F], long_desc="hand-made")
    return sd, rec, power, counts, outside, ext, rel


def test_shapes_radii_and_the_rule_for_a_cell_without_a_ray():
    sd, rec, power, counts, outside, ext, rel = hand_made()
    assert (sd.n_fields, sd.n_bands, sd.n_planes, sd.n_px, sd.size, sd.section, sd.z) == (2, 3, 2, 4, 0.5, 3, 12.0)
    assert sd.power.shape == (2, 3, 2, 4, 4) and sd.power_all.shape == (2, 2, 4, 4) and sd.centre.shape == (2, 3, 2, 2)
    assert sd.N.dtype == np.int64 and sd.N.shape == sd.outside_N.shape == sd.outside_power.shape == sd.geo_radius.shape == (2, 3, 2)
    assert np.array_equal(sd.N, counts[..., 0]) and np.array_equal(sd.outside_N, counts[..., 1])
    assert np.array_equal(sd.power_all, power.sum(axis=1)) and np.allclose(sd.wavelengths, [486, 589, 656]) and np.allclose(sd.t, [[0, 1]] * 2)
    some = np.ones((2, 3), dtype=bool)
    some[1, 2] = False
    assert np.array_equal(sd.geo_radius[some], np.sqrt(ext[..., 0])[some])
    assert np.array_equal(sd.rms_radius[some], np.sqrt(ext[some][:, :, 1] / rec[some][:, 0:1]))
    assert np.array_equal(sd.centre[some], (sd.origin[:2] + rel)[some]) and np.all(np.isfinite(sd.centre[some]))
    for a in (sd.geo_radius, sd.rms_radius, sd.centre):
        assert np.all(np.isnan(a[1, 2]))
    assert np.all(sd.power[1, 2] == 0) and np.all(sd.N[1, 2] == 0) and sd.band_N[1, 2] == 0
    with pytest.raises(RuntimeError, match="read-only"):
        sd.size = 2.0  # (locked)
    # bounds of what the constructor takes
    args = lambda **kw: {**dict(power=power, counts=counts, outside_power=outside, extents=ext, centre_rel=rel, records=rec, origin=sd.origin,
                                z=12.0, planes=sd.planes, n_px=4, size=0.5, reference_band=1, reference_field=0, section=3, sources=[0, 1],
                                field=[[0, 0], [0, 1.5]]), **kw}
    ot.SpotDiagram(**args())
    for bad in (dict(n_px=0), dict(n_px=1025), dict(n_px=5), dict(size=0.0), dict(size=-1.0), dict(reference_band=3), dict(reference_field=2),
                dict(planes=[1.0] * 66), dict(sources=[0]), dict(band_edges=[400, 500, 600]), dict(counts=counts[:1])):
        with pytest.raises(ValueError):
            ot.SpotDiagram(**args(**bad))
    ot.SpotDiagram(**args(band_edges=[400, 500, 600, 700]))


def test_centres():
    sd, rec, *_ = hand_made()
    zeta = np.array([2.4, 2.6])
    band = sdm.centres(rec, zeta, "band", 1, (0.25, -0.5))
    with np.errstate(invalid="ignore"):
        assert np.array_equal(band[0, 1, 1], (rec[0, 1, 2:4] + 2.6 * rec[0, 1, 4:6]) / rec[0, 1, 0]) and np.all(np.isnan(band[1, 2]))
    ref = sdm.centres(rec, zeta, "reference", 1, (0.25, -0.5))
    assert np.array_equal(ref[:, 0], band[:, 1]) and np.array_equal(ref[:, 2], band[:, 1]) and ref.shape == (2, 3, 2, 2)
    assert np.all(np.isnan(sdm.centres(rec, zeta, "reference", -1, (0.25, -0.5))))
    mid = sdm.centres(rec, zeta, "centroid", 1, (0.25, -0.5))
    want = (rec[1, :, 2:4].sum(axis=0) + 2.4 * rec[1, :, 4:6].sum(axis=0)) / rec[1, :, 0].sum()  # (the band without a ray adds zeros)
    assert np.allclose(mid[1, 0, 0], want, rtol=4 * EPS, atol=0) and np.array_equal(mid[:, 0], mid[:, 1]) and np.array_equal(mid[:, 0], mid[:, 2])
    given = sdm.centres(rec, zeta, np.array([[1.0, 2.0], [3.0, 4.0]]), 1, (0.25, -0.5))
    assert given.shape == (2, 3, 2, 2) and np.all(given[0] == [0.75, 2.5]) and np.all(given[1] == [2.75, 4.5]) and given.flags.c_contiguous


def test_images_and_the_matrix():
    sd, rec, power, *_ = hand_made()
    img = sd.image(0, 1, 2)
    c = sd.centre[0, 2, 1]
    assert isinstance(img, ot.ScalarImage) and img.shape == (4, 4) and np.array_equal(img.data, power[0, 2, 1])
    assert np.allclose(img.extent, [c[0] - 0.25, c[0] + 0.25, c[1] - 0.25, c[1] + 0.25], rtol=1e-15) and "hand-made" in img.long_desc
    assert np.array_equal(sd.image(-1, -1, -3).data, power[1, 0, 1])
    both = sd.image(0, 0)
    W = rec[0, :, 0]
    mean = (W[:, None] * sd.centre[0, :, 0]).sum(axis=0) / W.sum()
    assert np.array_equal(both.data, sd.power_all[0, 0]) and np.allclose(both.extent, [mean[0] - 0.25, mean[0] + 0.25, mean[1] - 0.25, mean[1] + 0.25])
    part = sd.image(1, 0)  # (the band without a ray has no say)
    mean = (rec[1, :2, 0, None] * sd.centre[1, :2, 0]).sum(axis=0) / rec[1, :2, 0].sum()
    assert np.allclose(part.extent[:2], [mean[0] - 0.25, mean[0] + 0.25])
    with pytest.raises(ValueError, match="no ray"):
        sd.image(1, 0, 2)
    for bad in ((2, 0, 0), (0, 2, 0), (0, 0, 3), (-3, 0, 0)):
        with pytest.raises(IndexError):
            sd.image(*bad)
    with pytest.raises(TypeError):
        sd.image(0.0, 0)
    # the matrix: fields in rows, field 0 at the bottom (row 0 is the lowest y), planes in columns
    for band, tiles in ((None, sd.power_all), (1, power[:, 1])):
        m = sd.matrix(band)
        assert m.shape == (8, 8) and np.allclose(m.extent, [0, 1.0, 0, 1.0])
        for f in range(2):
            for j in range(2):
                assert np.array_equal(m.data[4 * f:4 * f + 4, 4 * j:4 * j + 4], tiles[f, j])
    with pytest.raises(IndexError):
        sd.matrix(3)


def test_the_empty_result():
    dz = np.array([0.0, 1.0])
    e = sdm._empty(2, np.array([400.0, 500, 600]), 3.0, dz, 5, 0.5, origin=(0, 0, 1), reference_field=0, sources=[1], field=[[0, 1]])
    assert e.n_bands == 2 and e.z == 3.0 and e.planes.tolist() == [3.0, 4.0] and e.size == 0.5 and e.reference_band == -1
    assert e.power.shape == (1, 2, 2, 5, 5) and e.power_all.shape == (1, 2, 5, 5) and np.all(e.power == 0) and np.all(e.N == 0)
    assert np.all(np.isnan(e.centre)) and np.all(np.isnan(e.geo_radius)) and np.all(np.isnan(e.rms_radius)) and np.all(np.isnan(e.wavelengths))
    e = sdm._empty(2, "lines", None, np.zeros(1), 64, None, origin=(0, 0, 1), reference_field=1, sources=[0, 1], field=[[0, 1]] * 2)
    assert e.n_bands == 1 and np.isnan(e.z) and np.isnan(e.size) and e.band_edges is None and e.power.shape == (2, 1, 1, 64, 64)
    with pytest.raises(ValueError):
        e.matrix()


# ---- argument checks ---------------------------------------------------------------------------------------------------------------------
def test_check_arguments():
    assert sdm.check_arguments(64, None, "centroid", 3) == (64, None, "centroid")
    n_px, size, centre = sdm.check_arguments(np.int64(1024), 2, [[0, 1], [2, 3]], 2)
    assert (n_px, size) == (1024, 2.0) and type(n_px) is int and centre.dtype == np.float64 and centre.tolist() == [[0, 1], [2, 3]]
    for n_px in (0, -1, 1025):
        with pytest.raises(ValueError, match="n_px"):
            sdm.check_arguments(n_px, None, "band", 1)
    for n_px in (1.0, "8", None):
        with pytest.raises(TypeError):
            sdm.check_arguments(n_px, None, "band", 1)
    for size in (0, -1.0, NAN, np.inf):
        with pytest.raises(ValueError, match="size"):
            sdm.check_arguments(8, size, "band", 1)
    with pytest.raises(TypeError):
        sdm.check_arguments(8, "1", "band", 1)
    with pytest.raises(ValueError, match="centre"):
        sdm.check_arguments(8, None, "paraxial", 1)
    for centre in ([[0, 1]], [0, 1], np.zeros((2, 3)), [[0, 1], [NAN, 0]], [[0, 1], [np.inf, 0]]):
        with pytest.raises(ValueError, match="centre"):
            sdm.check_arguments(8, None, centre, 2)
    with pytest.raises(TypeError):
        sdm.check_arguments(8, None, [["a", "b"]], 1)
    with pytest.raises(TypeError):
        sdm.check_arguments(8, None, None, 1)
    # the cap on all cells, said on the host
    sdm.check_cap(64, 4, 1, 1024)
    for shape in ((64, 4, 2, 1024), (1, 1, 65, 2048), (3, 32, 65, 256)):
        with pytest.raises(RuntimeError, match="cells"):
            sdm.check_cap(*shape)
    # dz: the check of the MTF analysis
    assert mtf.check_arguments(None, None)[1].tolist() == [0.0]
    with pytest.raises(ValueError, match="dz"):
        mtf.check_arguments(None, [0.0, 0.0])


def test_raytracer_checks_before_it_looks_for_rays():
    RT = ot.Raytracer(outline=[-5, 5, -5, 5, -5, 30])
    RT.add(ot.RaySource(ot.Point(), pos=[0, 0, -2]))
    RT.add(ot.RaySource(ot.Point(), pos=[0, 1, -2]))
    for kwargs, err in ((dict(n_px=0), ValueError), (dict(size=0.0), ValueError), (dict(centre="middle"), ValueError),
                        (dict(centre=[[0, 0]]), ValueError), (dict(dz=[1.0, 0.0]), ValueError), (dict(dz=list(range(66))), ValueError),
                        (dict(sources=[0, 0]), ValueError), (dict(sources=[2]), IndexError), (dict(reference_field=2), IndexError),
                        (dict(bands=0), ValueError), (dict(z=NAN), ValueError), (dict(n_px=8.0), TypeError)):
        with pytest.raises(err):
            RT.spot_diagram(**kwargs)
    assert ot.SpotDiagram is sdm.SpotDiagram and callable(ot.Raytracer.spot_diagram)


def test_constants_match_the_header():
    text = (pathlib.Path(__file__).resolve().parents[1] / "include" / "optrace_amd.h").read_text()
    value = lambda name: int(re.search(rf"#define {name} (\d+)", text).group(1))
    assert value("OT_SD_MAX_PX") == _capi.SD_MAX_PX == sc.MAX_PX == 1024
    assert re.search(r"#define OT_SD_MAX_CELLS \(\(int64_t\)1 << 28\)", text) and _capi.SD_MAX_CELLS == sc.MAX_CELLS == 1 << 28
    assert value("OT_SD_BLOCKS") == _capi.SD_BLOCKS == sc.BLOCKS and value("OT_SD_MIN_BLOCKS") == _capi.SD_MIN_BLOCKS == sc.MIN_BLOCKS
    assert re.search(r"#define OT_SD_LDS_BYTES \(159 \* 1024\)", text) and _capi.SD_LDS_BYTES == sc.LDS_BYTES == 159 * 1024
    assert value("OT_ABI_VERSION") == _capi.ABI_VERSION == 9
    for name in ("ot_spotdiag_workspace", "ot_spotdiag_chunks", "ot_spotdiag_extent", "ot_spotdiag_maps"):
        assert name in _capi.SIGNATURES and re.search(rf"\b{name}\(", text)
