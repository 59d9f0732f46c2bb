"""ot.random and random_positions without a GPU: the names and signatures of the reference's sampling module, what comes back
for N = 0, the reference's errors, the argument checks of the C entry points (made before a device is looked for), the
refusal to run without a device, the shared range cutting and the fixture tests/golden/sampling.npz (generator:
tests/golden/generate_golden_sampling.py)."""
import ctypes as C
import inspect

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd.ray_storage import stratification_blocks
from helpers import load
import sampling_cases as sc

E = inspect.Parameter.empty
SHAPES = {"point": lambda: ot.Point(), "line": lambda: ot.Line(r=2, angle=30), "circle": lambda: ot.CircularSurface(r=2),
          "ring": lambda: ot.RingSurface(r=3, ri=1), "rect": lambda: ot.RectangularSurface(dim=[2, 3])}


@pytest.fixture(scope="module")
def g():
    return load("sampling.npz")


@pytest.fixture(scope="module")
def lib():
    return _capi.load_library()


def test_names_and_signatures():
    sig = lambda f: {k: (v.default, v.kind == v.KEYWORD_ONLY) for k, v in inspect.signature(f).parameters.items() if k != "self"}  # noqa: E731
    extra = dict(seed=(None, True), device=(False, True))
    r = ot.random
    assert sig(r.stratified_interval_sampling) == dict(a=(E, False), b=(E, False), N=(E, False), shuffle=(True, False), **extra)
    assert sig(r.stratified_rectangle_sampling) == dict(a=(E, False), b=(E, False), c=(E, False), d=(E, False), N=(E, False), **extra)
    assert sig(r.stratified_ring_sampling) == dict(ri=(E, False), r=(E, False), N=(E, False), polar=(False, False), **extra)
    assert sig(r.inverse_transform_sampling) == dict(x=(E, False), f=(E, False), S=(E, False), kind=("continuous", False), **extra)
    assert sig(r.random_wavelengths_from_srgb) == dict(rgb=(E, False), **extra)
    assert not hasattr(ot.color, "random_wavelengths_from_srgb") and "random.random_wavelengths_from_srgb" in ot.color.__doc__
    for name, make in SHAPES.items():
        assert sig(type(make()).random_positions) == dict(N=(E, False), seed=(None, True)), name


def test_zero_samples_need_no_device():
    r = ot.random
    singles = [r.stratified_interval_sampling(0, 1, 0), r.stratified_interval_sampling(0, 1, 0, shuffle=False),
               r.inverse_transform_sampling(np.arange(3.), np.ones(3), 0),
               r.inverse_transform_sampling(np.arange(3.), np.ones(3), np.array([]), kind="discrete"),
               r.random_wavelengths_from_srgb(np.zeros((0, 3)))]
    pairs = [r.stratified_rectangle_sampling(0, 1, 0, 1, 0), r.stratified_ring_sampling(0, 1, 0), r.stratified_ring_sampling(1, 2, 0, polar=True)]
    for a in singles + [v for p in pairs for v in p]:
        assert isinstance(a, np.ndarray) and a.dtype == np.float64 and a.shape == (0,)
    assert all(isinstance(p, tuple) and len(p) == 2 for p in pairs)
    for name, make in SHAPES.items():
        p = make().random_positions(0)
        assert p.shape == (0, 3) and p.dtype == np.float64, name


def test_reference_errors():
    x = np.arange(4.)
    for kind in ("continuous", "discrete"):
        with pytest.raises(RuntimeError, match="Cumulated probability is zero."):
            ot.random.inverse_transform_sampling(x, np.zeros(4), 10, kind=kind)
        with pytest.raises(RuntimeError, match="Got negative value in pdf."):
            ot.random.inverse_transform_sampling(x, np.array([1., -0.5, 1., 1.]), 10, kind=kind)
    go = ot.global_options
    old = go.wavelength_range
    try:
        go.__dict__["wavelength_range"] = [400., 780.]  # (the setter refuses such a range; the function checks for itself)
        with pytest.raises(RuntimeError, match="does not include range"):
            ot.random.random_wavelengths_from_srgb(np.ones((2, 3)))
    finally:
        go.__dict__["wavelength_range"] = old


def _ranges(*blocks):
    rng = (_capi.SourceRange * len(blocks))()
    for r, (first, count) in zip(rng, blocks):
        r.first, r.count = first, count
    return rng


def _refused(lib, status, code, *words):
    assert status == code
    msg = lib.ot_last_error().decode()
    for w in words:
        assert w in msg, msg


def test_entry_points_refuse_bad_arguments_before_the_device(lib):
    """Every refusal names its entry point and comes with OT_ERR_INVALID (-1) or OT_ERR_UNSUPPORTED (-3), never with the
    missing device's OT_ERR_NO_DEVICE: the checks come first.  (The pointers are never followed: 8 is not a buffer.)"""
    INVALID, UNSUPPORTED, P = -1, _capi.ERR_UNSUPPORTED, C.c_void_p(8)
    b = lambda *v: (C.c_double * 4)(*v)  # noqa: E731
    one = _ranges((0, 10))
    strat = lib.ot_sample_stratified
    _refused(lib, strat(0, 1, b(0, 1), one, 1, 1, 10, None, None, None), INVALID, "ot_sample_stratified", "null")
    _refused(lib, strat(1, 0, b(0, 1, 0, 1), one, 1, 1, 10, P, None, None), INVALID, "ot_sample_stratified", "null")
    _refused(lib, strat(0, 1, None, one, 1, 1, 10, P, None, None), INVALID, "ot_sample_stratified", "null")
    _refused(lib, strat(7, 1, b(0, 1), one, 1, 1, 10, P, P, None), INVALID, "ot_sample_stratified", "kind")
    _refused(lib, strat(0, 1, b(0, 1), one, 1, 1, -1, P, None, None), INVALID, "ot_sample_stratified", "negative")
    _refused(lib, strat(0, 1, b(1, 0), one, 1, 1, 10, P, None, None), INVALID, "ot_sample_stratified", "bound")
    _refused(lib, strat(1, 0, b(0, 1, 2, 1), one, 1, 1, 10, P, P, None), INVALID, "ot_sample_stratified", "bound")
    _refused(lib, strat(2, 0, b(2, 2), one, 1, 1, 10, P, P, None), INVALID, "ot_sample_stratified", "ri < r")
    _refused(lib, strat(0, 1, b(0, 1), None, 0, 1, 10, P, None, None), INVALID, "ot_sample_stratified", "range")
    _refused(lib, strat(0, 1, b(0, 1), _ranges((0, 4), (5, 5)), 2, 1, 10, P, None, None), INVALID, "ot_sample_stratified", "cover")
    _refused(lib, strat(0, 1, b(0, 1), one, 1, 1, 11, P, None, None), INVALID, "ot_sample_stratified", "cover")
    _refused(lib, strat(0, 1, b(0, 1), _ranges((0, 2**32)), 1, 1, 2**32, P, None, None), UNSUPPORTED, "ot_sample_stratified", "2^32")
    assert strat(0, 1, b(0, 1), None, 0, 1, 0, P, None, None) == 0  # n = 0: nothing to do, no device needed

    pos = lib.ot_sample_positions
    s = _capi.Source()
    s.shape = _capi.SRC_RING
    s.r, s.ri = 1.0, 1.0
    _refused(lib, pos(C.byref(s), one, 1, 1, 10, P, None), INVALID, "ot_sample_positions", "ri < r")
    s.shape = _capi.SRC_IMAGE_RGB
    _refused(lib, pos(C.byref(s), one, 1, 1, 10, P, None), UNSUPPORTED, "ot_sample_positions", "image")
    s.shape = _capi.SRC_IMAGE_GRAY
    _refused(lib, pos(C.byref(s), one, 1, 1, 10, P, None), UNSUPPORTED, "ot_sample_positions", "image")
    s.shape = 9
    _refused(lib, pos(C.byref(s), one, 1, 1, 10, P, None), INVALID, "ot_sample_positions", "shape")
    s.shape = _capi.SRC_POINT
    _refused(lib, pos(None, one, 1, 1, 10, P, None), INVALID, "ot_sample_positions", "null")
    _refused(lib, pos(C.byref(s), one, 1, 1, 10, None, None), INVALID, "ot_sample_positions", "null")
    _refused(lib, pos(C.byref(s), one, 1, 1, -5, P, None), INVALID, "ot_sample_positions", "negative")
    _refused(lib, pos(C.byref(s), None, 0, 1, 10, P, None), INVALID, "ot_sample_positions", "range")
    assert pos(C.byref(s), None, 0, 1, 0, P, None) == 0

    inv = lib.ot_sample_inverse
    x, f = (C.c_double * 3)(1, 2, 3), (C.c_double * 3)(1, 0, 1)
    _refused(lib, inv(1, None, f, 3, None, 10, one, 1, 1, P, None), INVALID, "ot_sample_inverse", "null")
    _refused(lib, inv(1, x, f, 3, None, 10, one, 1, 1, None, None), INVALID, "ot_sample_inverse", "null")
    _refused(lib, inv(1, x, f, 0, None, 10, one, 1, 1, P, None), INVALID, "ot_sample_inverse", "pdf")
    _refused(lib, inv(2, x, f, 3, None, 10, one, 1, 1, P, None), INVALID, "ot_sample_inverse", "kind")
    _refused(lib, inv(0, x, f, 3, None, -1, one, 1, 1, P, None), INVALID, "ot_sample_inverse", "negative count")
    _refused(lib, inv(0, x, (C.c_double * 3)(1, -1, 1), 3, None, 10, one, 1, 1, P, None), INVALID, "ot_sample_inverse", "negative value")
    _refused(lib, inv(1, x, (C.c_double * 3)(0, 0, 0), 3, None, 10, one, 1, 1, P, None), INVALID, "ot_sample_inverse", "zero")
    _refused(lib, inv(0, x, f, 3, None, 10, None, 0, 1, P, None), INVALID, "ot_sample_inverse", "range")
    assert inv(0, x, f, 3, None, 0, None, 0, 1, P, None) == 0

    wl = lib.ot_sample_srgb_wavelengths
    _refused(lib, wl(None, 10, one, 1, 1, P, None), INVALID, "ot_sample_srgb_wavelengths", "null")
    _refused(lib, wl(P, 10, one, 1, 1, None, None), INVALID, "ot_sample_srgb_wavelengths", "null")
    _refused(lib, wl(P, -1, one, 1, 1, P, None), INVALID, "ot_sample_srgb_wavelengths", "negative")
    _refused(lib, wl(P, 10, _ranges((0, 3), (3, 3)), 2, 1, P, None), INVALID, "ot_sample_srgb_wavelengths", "cover")
    assert wl(P, 0, None, 0, 1, P, None) == 0


@pytest.mark.skipif(torch.cuda.is_available(), reason="a device is present: the samplers run")
def test_no_fallback_without_a_device(lib):
    r = ot.random
    calls = [lambda: r.stratified_interval_sampling(0, 1, 5), lambda: r.stratified_rectangle_sampling(0, 1, 0, 1, 5),
             lambda: r.stratified_ring_sampling(0, 1, 5), lambda: r.inverse_transform_sampling(np.arange(3.), np.ones(3), 5),
             lambda: r.inverse_transform_sampling(np.arange(3.), np.ones(3), np.array([0.5]), kind="discrete"),
             lambda: r.random_wavelengths_from_srgb(np.ones((5, 3)))] + [lambda m=m: m().random_positions(5) for m in SHAPES.values()]
    for call in calls:
        with pytest.raises(ot.BackendError):
            call()
    # the library itself: valid arguments get as far as the device lookup
    status = lib.ot_sample_stratified(0, 1, (C.c_double * 4)(0, 1), _ranges((0, 10)), 1, 1, 10, C.c_void_p(8), None, None)
    assert status == -4 and b"no HIP device" in lib.ot_last_error()


def test_range_cutting_is_shared_with_the_ray_storage():
    """Power-of-two blocks from 2^16 on, largest first, and one ragged rest -- and RayStorage cuts a source's rays with the
    same function, so that equal (seed, N) give equal draws."""
    assert stratification_blocks(0, 1000, 64) == [(0, 1000)]
    assert stratification_blocks(0, 1 << 20, 64) == [(0, 1 << 20)]
    assert stratification_blocks(7, (1 << 16) + 1000, 64) == [(7, 1 << 16), (7 + (1 << 16), 1000)]
    assert stratification_blocks(0, (1 << 20) + (1 << 17) + 3, 64) == [(0, 1 << 20), (1 << 20, 1 << 17), ((1 << 20) + (1 << 17), 3)]
    assert stratification_blocks(0, 7 << 16, 2) == [(0, 4 << 16), (4 << 16, 3 << 16)]  # no more blocks than asked for
    assert stratification_blocks(0, 0, 64) == [(0, 0)]
    rs = ot.RayStorage()
    src = [ot.RaySource(ot.CircularSurface(r=1), pos=[0, 0, 0]), ot.RaySource(ot.Point(), pos=[0, 0, 0])]
    rs.__dict__.update(N_list=np.array([(1 << 17) + 5, 300]), B_list=np.array([0, (1 << 17) + 5, (1 << 17) + 305]),
                       ray_source_list=src, _powers=[1.0, 1.0], _ranges=None)
    got = [(r.source, r.first, r.count) for r in rs._source_ranges()]
    want = [(0, f, c) for f, c in stratification_blocks(0, (1 << 17) + 5, 32)] + [(1, (1 << 17) + 5, 300)]
    assert got == want and len(got) == 3


def test_fixture_shape(g):
    for kind, case in (("discrete", sc.discrete_case), ("continuous", sc.continuous_case)):
        x, f, S = case()
        for key, val in (("x", x), ("f", f), ("S", S)):
            assert g[f"inverse/{kind}/{key}"].tobytes() == val.tobytes(), (kind, key)
        assert g[f"inverse/{kind}/out"].shape == S.shape and np.all(np.isfinite(g[f"inverse/{kind}/out"]))
    x, f, S = sc.discrete_case()
    assert x.shape == (12,) and np.count_nonzero(f == 0) == 3 and S.shape == (511,) and S[0] == 0 and S[1] == 1
    assert set(g["inverse/discrete/out"]) == set(x[f > 0])  # every entry with weight is drawn, no other
    x, f, S = sc.continuous_case()
    assert x.shape == (200,) and np.count_nonzero(f == 0) == 30 and S.shape == (500,)
    out = g["inverse/continuous/out"]
    assert not np.any((out > x[80]) & (out < x[109]))  # nothing is drawn inside the stretch of zeros
    assert np.array_equal(g["srgb/edges"], sc.EDGES) and sc.EDGES.shape == (41,)
    for name, rgb in sc.COLOURS.items():
        cdf = g[f"srgb/{name}/cdf"]
        assert np.array_equal(g[f"srgb/{name}/rgb"], np.array(rgb))
        assert cdf.shape == (41,) and cdf[0] == 0 and abs(cdf[-1] - 1) < 1e-12 and np.all(np.diff(cdf) >= 0)
        assert 0.5 / sc.N_WL < float(g[f"srgb/{name}/worst"]) < 4 / sc.N_WL  # a stratified sample: a few counts
    assert g["srgb/red/cdf"][20] < 0.1 < 0.9 < g["srgb/blue/cdf"][20]  # 580 nm: blue lies below, red above
    for N in sc.RING_N:
        assert 0 < float(g[f"cells/ring/{N}"]) < 1
    assert float(g["cells/ring/4096"]) < float(g["cells/ring/1000"])
    assert 0 < float(g[f"cells/rect/{sc.RECT_N}"]) < 1 and int(g["cells/rect/extra"]) == 39
