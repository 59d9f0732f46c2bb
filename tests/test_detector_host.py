"""Host side of the detector stage (CPU only): the request record from spec to C struct (`detector.DetectorRequest`,
`Raytracer._detector_requests`, `detector._requests`), the batching rule of its launches (`detector.batches`) and the image
builder (`RenderImage.on_grid`) against the extent and pixel-count rules it wraps (render_image.py:224-255, :383-387)."""
import ctypes as C

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi, detector as _detector
from optrace_amd.render_image import RenderImage


def record(first=0, count=100, projection=None, crop=None, **kw):
    return _detector.DetectorRequest(first, count, _capi.Surface(), projection, crop, 0, None, "", **kw)


# ---- batches --------------------------------------------------------------------------------------------------------
def check_batches(reqs):
    """-> batches as lists of indices; every index once, no batch over DET_MAX or over two ray ranges, ranges in order of
    first appearance, indices of a range in order"""
    got = list(_detector.batches(reqs))
    for idx, part in got:
        assert 1 <= len(idx) <= _capi.DET_MAX
        assert len(part) == len(idx) and all(rq is reqs[n] for n, rq in zip(idx, part))
        assert len({(rq.first, rq.count) for rq in part}) == 1
    flat = [n for idx, _ in got for n in idx]
    assert sorted(flat) == list(range(len(reqs)))
    ranges = list(dict.fromkeys((rq.first, rq.count) for rq in reqs))  # order of first appearance
    want = [n for r in ranges for n, rq in enumerate(reqs) if (rq.first, rq.count) == r]
    assert flat == want
    return [idx for idx, _ in got]


@pytest.mark.parametrize("n", [0, 1, 8, 9, 19])
def test_batches_of_one_ray_range(n):
    assert _capi.DET_MAX == 8
    got = check_batches([record() for _ in range(n)])
    assert got == [list(range(b, min(b + 8, n))) for b in range(0, n, 8)]


@pytest.mark.parametrize("n", [0, 1, 8, 9, 19, 30])
def test_batches_of_three_interleaved_ray_ranges(n):
    ranges = [(50, 20), (0, 100), (0, None)]  # (the last: the whole of the storage a plan is launched on)
    reqs = [record(*ranges[k % 3]) for k in range(n)]
    got = check_batches(reqs)
    per_range = [len(range(r, n, 3)) for r in range(3)]
    assert len(got) == sum(-(-m // 8) for m in per_range)
    if n == 30:  # ten per range: 8 + 2 each, range by range
        assert got[0] == list(range(0, 24, 3)) and got[1] == [24, 27] and got[2] == list(range(1, 25, 3))


# ---- record -> C struct ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("struct", [_capi.DetectorReq, _capi.DetectorImageReq])
def test_requests_fill_the_struct_from_the_record(struct):
    crops = [None, np.array([-1.5, 2.0, -0.25, 0.125]), None, [0.0, 1.0, 2.0, 3.0]]
    projections = [None, "Equidistant", "Orthographic", "Stereographic"]
    reqs = [record(projection=p, crop=c) for p, c in zip(projections, crops)]
    ill = torch.zeros(2 * len(reqs), dtype=torch.int64)
    arr, keep = _detector._requests(struct, reqs, ill)
    assert len(arr) == len(reqs)
    for k, (rq, r) in enumerate(zip(reqs, arr)):
        assert r.detector == C.addressof(rq.surf)
        assert r.projection == _capi.PROJECTIONS[projections[k]] == rq.proj_id
        if crops[k] is None:
            assert not r.crop4
        else:
            assert list((C.c_double * 4).from_address(r.crop4)) == [float(v) for v in crops[k]]
        assert r.ill_count == ill.data_ptr() + 16 * k


# ---- image builder -------------------------------------------------------------------------------------------------------
EXTENTS = {"point": [1.0, 1.0, -2.0, -2.0], "horizontal line": [-1.0, 3.0, 0.5, 0.5], "vertical line": [0.25, 0.25, -1.0, 2.0],
           "ratio 1.9": [0.0, 4.0, 0.0, 4.0 / 1.9], "ratio 2.0": [-2.1, 2.1, -1.05, 1.05], "ratio 4.4": [0.0, 1.0, 0.0, 4.4],
           "ratio 5.1": [0.0, 5.1, 1.0, 2.0], "strip 40:1": [-20.0, 20.0, 0.0, 1.0]}


@pytest.mark.parametrize("limit", [None, 5])
@pytest.mark.parametrize("name", list(EXTENTS))
def test_image_builder_equals_the_steps_it_wraps(name, limit):
    extent = np.array(EXTENTS[name])
    ref = RenderImage(extent=extent.copy(), projection=None, long_desc="label")
    ref._limit = limit
    ref._fix_extent()
    Nx_ref, Ny_ref = ref._pixel_counts()
    img, Nx, Ny = RenderImage.on_grid(extent.copy(), None, "label", limit)
    assert (Nx, Ny) == (Nx_ref, Ny_ref) and min(Nx, Ny) == RenderImage.MAX_IMAGE_SIDE
    assert img.extent.tobytes() == ref.extent.tobytes()
    assert img._extent0.tobytes() == extent.tobytes()
    assert img.limit == ref.limit and img.long_desc == "label" and img.projection is None and not img.has_image()
    again = RenderImage(extent=extent.copy())  # and `render` fixes its grid the same way
    assert again._grid(limit) == (Nx, Ny) and again.extent.tobytes() == ref.extent.tobytes()


def test_attached_histogram_is_the_image():
    img, Nx, Ny = RenderImage.on_grid([0.0, 3.0, 0.0, 1.0])
    hist = torch.arange(Ny * Nx * 4, dtype=torch.float64)
    img._attach(hist, Nx, Ny)
    assert img.shape == (Ny, Nx, 4) and img._dev.data_ptr() == hist.data_ptr()
    assert img._data[1, 2, 3] == (Nx + 2) * 4 + 3


# ---- labels -----------------------------------------------------------------------------------------------------------------
def test_labels():
    RT = ot.Raytracer(outline=[-5, 5, -5, 5, -5, 40])
    RT.add(ot.RaySource(ot.CircularSurface(r=1), divergence="None", s=[0, 0, 1], pos=[0, 0, 0]))
    RT.add(ot.Detector(ot.RectangularSurface(dim=[4, 4]), pos=[0, 0, 30]))
    RT.add(ot.Detector(ot.RectangularSurface(dim=[4, 4]), pos=[0, 0, 12.3456789], desc="film"))
    plain, named, moved = RT._detector_requests([dict(detector_index=0), dict(detector_index=1, source_index=0),
                                                 dict(detector_index=1, pos=[0, 0, 20.5])], no_rays=True)
    assert plain.label == plain.image_label == "DET0 at z = 30 mm"
    assert named.label == "DET1: film at z = 12.346 mm"
    assert named.image_label == "Rays from RS0 at DET1: film at z = 12.346 mm"
    assert moved.label == moved.image_label == "DET1: film at z = 20.5 mm"
    assert (plain.detector_index, plain.source_index, named.detector_index, named.source_index) == (0, None, 1, 0)
    assert (plain.first, plain.count) == (0, None)  # a plan made before the rays exist: the whole storage
    assert np.array_equal(plain.centre, [0, 0, 0, 0]) and plain.centre.dtype == np.float64
    off_axis = RT._detector_requests([dict(detector_index=0, pos=[0.5, -1.25, 30])], no_rays=True)[0]
    assert np.array_equal(off_axis.centre, [0.5, 0.5, -1.25, -1.25])
    assert plain.crop is None and not (plain.want_z or plain.compact or plain.weights_only)
    again = RT._detector_requests([plain, named])  # made already: as they are
    assert again[0] is plain and again[1] is named
