"""`Raytracer.huygens_stack` without a device: its argument checks and those of `ot_psf_stack` and `ot_psf_combine`, which come
before any device call, the workspace mirror, the band assignment rule at the edges, the diffraction MTF on the longdouble truth
of a perfect wave, the band weights by hand and the host-only side of `ot.HuygensStack`."""
import ctypes as C

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd import psf as hp

import psf_cases as pc
from test_wavefront_host import tracer


@pytest.mark.parametrize("kwargs,error", [
    # what huygens_psf refuses
    (dict(n_px=8.0), TypeError), (dict(n_px=None), TypeError), (dict(n_px=True), TypeError), (dict(n_px=0), ValueError),
    (dict(n_px=1025), ValueError), (dict(size="1"), TypeError), (dict(size=0.0), ValueError), (dict(size=np.nan), ValueError),
    (dict(section=1.0), TypeError), (dict(section=-1), ValueError), (dict(section=3), ValueError),
    (dict(focus=3.0), TypeError), (dict(focus=[0, 1]), ValueError), (dict(focus=[0, np.nan, 1]), ValueError),
    (dict(radius="1"), TypeError), (dict(radius=0.0), ValueError), (dict(radius=-np.inf), ValueError),
    (dict(source_index=0.0), TypeError),
    # dz: a finite number, or 1 .. 64 of them in one dimension
    (dict(dz="0"), TypeError), (dict(dz=None), TypeError), (dict(dz=np.nan), ValueError), (dict(dz=-np.inf), ValueError),
    (dict(dz=[]), ValueError), (dict(dz=np.zeros(65)), ValueError), (dict(dz=np.zeros((2, 2))), ValueError),
    (dict(dz=[0.0, np.nan]), ValueError), (dict(dz=[0.0, np.inf]), ValueError), (dict(dz=[0.0, "1"]), TypeError),
    (dict(dz=[0.0, None]), TypeError),
    # bands: "lines", an int in 1 .. 32, or 2 .. 33 strictly ascending finite edges
    (dict(bands="line"), ValueError), (dict(bands=None), TypeError), (dict(bands=2.0), TypeError), (dict(bands=True), TypeError),
    (dict(bands=0), ValueError), (dict(bands=-1), ValueError), (dict(bands=33), ValueError),
    (dict(bands=[500.0]), ValueError), (dict(bands=[]), ValueError), (dict(bands=np.linspace(400, 700, 35)), ValueError),
    (dict(bands=[400.0, 400.0]), ValueError), (dict(bands=[500.0, 400.0]), ValueError), (dict(bands=[400.0, np.nan]), ValueError),
    (dict(bands=[400.0, np.inf]), ValueError), (dict(bands=[400.0, "500"]), TypeError), (dict(bands=np.zeros((2, 2))), ValueError),
])
def test_argument_errors_come_before_the_device(kwargs, error, monkeypatch):
    """(no rays traced, and `require_device` made to fail loudly: the argument is what the call complains about)"""
    from optrace_amd import raytracer

    def touched():
        raise AssertionError("the device was asked for before the arguments were checked")
    monkeypatch.setattr(raytracer, "require_device", touched)
    with pytest.raises(error):
        tracer().huygens_stack(**kwargs)


def test_good_arguments_reach_the_device_question():
    if torch.cuda.is_available():
        pytest.skip("device present")
    for kwargs in (dict(), dict(dz=[-0.1, 0.0, 0.1]), dict(dz=np.zeros(64), bands=32), dict(bands=[400, 500.5, 700], n_px=1),
                   dict(bands=np.linspace(380, 780, 33), dz=(0.5,), section=2, focus=(0, 0, 20), radius=-3, size=0.5)):
        with pytest.raises(ot.BackendError):
            tracer().huygens_stack(**kwargs)


def test_entry_points_check_their_arguments_before_anything_else():
    """In the pattern of `psf_cases.entry_point_argument_checks`: the code, the entry's name in `ot_last_error`, no device looked
    for, so that the addresses are never dereferenced -- but `starts` and `dz`, which are host arrays."""
    lib = _capi.load_library()
    st = C.c_void_p()
    buf = (C.c_double * 8)()
    a = C.addressof(buf)
    INVALID, UNSUPPORTED = -1, -3
    nan, inf = float("nan"), float("inf")
    i64s = lambda *v: (C.c_int64 * len(v))(*v)
    dbl = lambda *v: (C.c_double * len(v))(*v)

    def refused(code, name, rc):
        assert rc == code, (name, rc)
        assert name.encode() in lib.ot_last_error(), lib.ot_last_error()

    stack = lambda n, rec, K, starts, radius, n_px, size, Z, dz, ws, field, sums: lib.ot_psf_stack(n, rec, K, starts, radius, n_px, size,
                                                                                                    Z, dz, ws, field, sums, st)
    ok = [a, 2, i64s(0, 4, 10), 5.0, 8, 0.1, 2, dbl(0.0, 0.1), a, a, a]
    for i in (0, 2, 7, 8, 9, 10):
        refused(INVALID, "ot_psf_stack: null argument", stack(10, *[None if j == i else x for j, x in enumerate(ok)]))
    refused(INVALID, "ot_psf_stack", stack(-1, *ok))
    refused(INVALID, "ot_psf_stack: n_px below 1", stack(10, *ok[:4], 0, *ok[5:]))
    refused(UNSUPPORTED, "ot_psf_stack: n_px above 1024", stack(10, *ok[:4], 1025, *ok[5:]))
    refused(INVALID, "ot_psf_stack: n_bands below 1", stack(10, ok[0], 0, *ok[2:]))
    refused(UNSUPPORTED, "ot_psf_stack: n_bands above 32", stack(10, ok[0], 33, *ok[2:]))
    refused(INVALID, "ot_psf_stack: n_planes below 1", stack(10, *ok[:6], 0, *ok[7:]))
    refused(UNSUPPORTED, "ot_psf_stack: n_planes above 64", stack(10, *ok[:6], 65, *ok[7:]))
    for starts in (i64s(1, 4, 10), i64s(0, 4, 9), i64s(0, 4, 11), i64s(0, 11, 10), i64s(0, -1, 10)):
        refused(INVALID, "ot_psf_stack: starts", stack(10, *ok[:2], starts, *ok[3:]))
    for size in (0.0, -1.0, inf, nan):
        refused(INVALID, "ot_psf_stack: size", stack(10, *ok[:5], size, *ok[6:]))
    for dz in (dbl(0.0, inf), dbl(nan, 0.0)):
        refused(INVALID, "ot_psf_stack: dz", stack(10, *ok[:7], dz, *ok[8:]))
    for radius in (0.0, nan, inf):
        refused(INVALID, "ot_psf_stack: radius", stack(10, *ok[:3], radius, *ok[4:]))
    # the cap: workspace bound plus field above 2^28 doubles, whatever n is
    refused(UNSUPPORTED, "ot_psf_stack: workspace and field", stack(10, ok[0], 32, i64s(*([0] * 32), 10), 5.0, 1024, 0.1, 64, dbl(*([0.0] * 64)), a, a, a))
    refused(UNSUPPORTED, "ot_psf_stack: workspace and field", stack(0, ok[0], 32, i64s(*([0] * 33)), 5.0, 1024, 0.1, 64, dbl(*([0.0] * 64)), a, a, a))
    assert stack(0, ok[0], 2, i64s(0, 0, 0), *ok[3:]) == 0  # (no record: no launch)

    comb = lambda K, Z, n_px, *p: lib.ot_psf_combine(K, Z, n_px, *p, st)
    ptrs = [a] * 7
    for i in range(7):
        refused(INVALID, "ot_psf_combine: null argument", comb(2, 3, 8, *[None if j == i else x for j, x in enumerate(ptrs)]))
    refused(INVALID, "ot_psf_combine: n_px below 1", comb(2, 3, 0, *ptrs))
    refused(UNSUPPORTED, "ot_psf_combine: n_px above 1024", comb(2, 3, 1025, *ptrs))
    refused(INVALID, "ot_psf_combine: n_bands below 1", comb(0, 3, 8, *ptrs))
    refused(UNSUPPORTED, "ot_psf_combine: n_bands above 32", comb(33, 3, 8, *ptrs))
    refused(INVALID, "ot_psf_combine: n_planes below 1", comb(2, 0, 8, *ptrs))
    refused(UNSUPPORTED, "ot_psf_combine: n_planes above 64", comb(2, 65, 8, *ptrs))
    assert (_capi.PSF_MAX_BANDS, _capi.PSF_MAX_PLANES, _capi.PSF_STACK_CAP) == (32, 64, 2 ** 28)


def test_workspace_mirror_is_the_librarys():
    lib = _capi.load_library()
    for n, n_px in ((1, 1), (63, 2), (257, 33), (257, 64), (70001, 8), (1000000, 128), (10 ** 7, 256), (5, 1024), (130000, 31)):
        assert lib.ot_psf_stack_workspace(n, 1, n_px, 1) == _capi.psf_stack_ws(n, 1, n_px, 1) == _capi.psf_ws(n, n_px) > 0, (n, n_px)
        for K, Z in ((2, 3), (5, 2), (3, 21), (32, 64), (1, 64), (32, 1)):
            assert lib.ot_psf_stack_workspace(n, K, n_px, Z) == _capi.psf_stack_ws(n, K, n_px, Z) > 0, (n, n_px, K, Z)
    # by hand: 928721 records, 64^2 + 1 points in 5 tiles, 21 planes: 4 x 1024 / 105 = 39 chunks, two more for three bands
    assert _capi.psf_stack_ws(928721, 3, 64, 21) == 21 * 41 * (2 * 4097 + 2)
    for bad in ((-1, 1, 8, 1), (10, 0, 8, 1), (10, 33, 8, 1), (10, 1, 0, 1), (10, 1, 1025, 1), (10, 1, 8, 0), (10, 1, 8, 65)):
        assert lib.ot_psf_stack_workspace(*bad) == 0


def f32(*v):
    return torch.tensor(v, dtype=torch.float32)


def test_band_assignment_at_the_edges():
    """float32 wavelengths exactly on float64 edges: a lower edge is in, the upper edge of an inner band belongs to the next band,
    the upper edge of the last band is in; what lies outside, and what is not live, gets K."""
    edges = np.array([400.0, 500.0, 600.25, 700.0])
    below, above = np.nextafter(np.float32(400), np.float32(0)), np.nextafter(np.float32(700), np.float32(1e9))
    inner = np.nextafter(np.float32(500), np.float32(0))
    wl = f32(400.0, 500.0, 600.25, 700.0, below, above, inner, 450.0, 650.0)
    live = torch.ones(9, dtype=torch.bool)
    live[7] = False
    key, K, table = hp.assign_bands(wl, live, edges)
    assert K == 3 and key.tolist() == [0, 1, 2, 2, 3, 3, 0, 3, 2] and np.array_equal(table.numpy(), edges)
    # an edge that no float32 holds: 486.1327 as float32 lies below the float64 486.1327, and it is the float32 that is compared
    assert float(np.float32(486.1327)) < 486.1327
    key, _, _ = hp.assign_bands(f32(486.1327), torch.ones(1, dtype=torch.bool), np.array([400.0, 486.1327, 700.0]))
    assert key.tolist() == [0]
    # an int: equal bands over [min, max] of the live rays; the dead ray's wavelength does not widen them
    wl = f32(400.0, 500.0, 550.0, 599.0, 600.0, 900.0)
    live = torch.tensor([True] * 5 + [False])
    key, K, table = hp.assign_bands(wl, live, 2)
    assert K == 2 and np.array_equal(table.numpy(), [400, 500, 600]) and key.tolist() == [0, 1, 1, 1, 1, 2]
    # one wavelength and K = 4: every ray on the last edge, which the host reads as one band
    key, K, table = hp.assign_bands(f32(550.0, 550.0, 550.0), torch.ones(3, dtype=torch.bool), 4)
    assert key.tolist() == [3, 3, 3]
    rec = torch.arange(18, dtype=torch.float64)
    grouped, starts, tab, order = hp.group_records(rec, 3, key, K, table)
    assert starts.tolist() == [0, 0, 0, 0, 3] and torch.equal(grouped, rec)
    K1, starts1, edges1 = hp.settle_bands(4, K, starts, tab)
    assert K1 == 1 and starts1.tolist() == [0, 3] and edges1.tolist() == [550, 550]


def test_lines_and_the_stable_group_by():
    wl = f32(656.2725, 486.1327, 587.5618, 486.1327, 656.2725, 700.0, 486.1327)
    live = torch.tensor([True, True, True, True, True, False, True])
    key, K, table = hp.assign_bands(wl, live, "lines")
    assert K == 32 and key.tolist() == [2, 0, 1, 0, 2, 32, 0] and table[0] == 3
    rec = torch.arange(6 * 7, dtype=torch.float64)
    grouped, starts, tab, order = hp.group_records(rec, 7, key, K, table)
    assert order.tolist() == [1, 3, 6, 2, 0, 4], "band by band, ascending ray order within a band, the dead ray dropped"
    assert np.array_equal(grouped.view(6, 6)[3].numpy(), 21 + np.array([1, 3, 6, 2, 0, 4]))
    K, starts, edges = hp.settle_bands("lines", K, starts, tab)
    assert K == 3 and starts.tolist() == [0, 3, 4, 6] and edges is None
    assert np.array_equal(tab[1:4], np.float32([486.1327, 587.5618, 656.2725]).astype(np.float64))
    # 32 lines are taken, 33 are refused with the count and the way out
    for n_lines in (32, 33):
        wl = torch.arange(n_lines, dtype=torch.float32) + 400
        key, K, table = hp.assign_bands(wl, torch.ones(n_lines, dtype=torch.bool), "lines")
        _, starts, tab, _ = hp.group_records(torch.zeros(6 * n_lines, dtype=torch.float64), n_lines, key, K, table)
        if n_lines == 32:
            assert hp.settle_bands("lines", K, starts, tab)[0] == 32 and starts.tolist() == list(range(33))
        else:
            with pytest.raises(RuntimeError, match="33 distinct wavelengths.*edges or a number"):
                hp.settle_bands("lines", K, starts, tab)


N_RINGS = 48
MTF_DEVIATION = 0.0693  # measured on the CPU from the truth: 0.06923 (largest above the cutoff: 0.0011)


def test_mtf_of_a_perfect_wave_is_the_circular_pupils():
    """A perfect wave of NA 0.05 at 550 nm, 48 rings = 6912 rays, R = 50 mm, 64 x 64 points over the default size
    10 lambda / NA = 0.11 mm: `mtf()` of the longdouble truth against (2 / pi) (acos nu - nu sqrt(1 - nu^2)), nu = f lambda / (2 NA).
    The deviation comes from cutting the Airy tails at the window and from the finite ray rule -- the stratified rule carries no
    random background, so the noise floor 1 / n that `mtf` subtracts, 4096 / 6912 = 0.59 against a summed intensity of 13, is the
    larger share, and it shrinks as 1 / n --; measured here on the CPU it is 0.0692 at the most, along x and y alike, 0.0011
    above the cutoff, and 1.25 times 0.0693 is allowed, also for MTF = 0 above nu = 1."""
    na, wl, n_px = 0.05, 550.0, 64
    size = 10 * wl * 1e-6 / na
    rec = pc.perfect_wave(N_RINGS, na, wl, 50.0)
    n = rec.shape[1]
    assert n == 3 * N_RINGS ** 2
    # (every ring of the rule is symmetric about the x axis, and so is the image: the lower half of the rows is summed, the upper mirrored)
    half = n_px * n_px // 2
    re, im, bound, A, A2, _ = pc.truth(rec, 50.0, n_px, size, 0.0, points=np.append(np.arange(half), n_px * n_px))
    inten = ((re * re + im * im) / (A * A)).astype(np.float64)
    lower = inten[:-1].reshape(n_px // 2, n_px)
    inten = np.append(np.concatenate([lower, lower[::-1]]).ravel(), inten[-1])
    st = ot.HuygensStack(n, float(A2), 0, 0, 2, (0, 0, 50), 50.0, size, [0.0], None, [n], [float(A2)], [wl], [1.0], inten[:-1].reshape(1, n_px, n_px),
                         [inten[-1]], [[inten[-1]]], float(A2 / (A * A)))
    m = st.mtf(0, n_f=81)
    assert m.f.shape == m.mtf_x.shape == m.mtf_y.shape == (81,) and m.f[0] == 0 and m.f[-1] == pytest.approx(n_px / (2 * size), rel=1e-15)
    assert m.mtf_x[0] == 1 and m.mtf_y[0] == 1
    nu = m.f * wl * 1e-6 / (2 * na)
    want = np.where(nu < 1, 2 / np.pi * (np.arccos(np.minimum(nu, 1)) - nu * np.sqrt(np.maximum(1 - nu * nu, 0))), 0.0)
    dev = max(np.abs(m.mtf_x - want).max(), np.abs(m.mtf_y - want).max())
    print("largest deviation of the MTF from the circular pupil's", dev, "above the cutoff", np.abs(m.mtf_x[nu > 1]).max())
    assert nu[-1] > 1.5 and np.count_nonzero(nu > 1) > 20
    assert dev <= 1.25 * MTF_DEVIATION
    # f_max: up to the sampling limit, not beyond
    half = st.mtf(0, n_f=5, f_max=100.0)
    assert np.array_equal(half.f, [0, 25, 50, 75, 100]) and half.mtf_x[0] == 1
    with pytest.raises(ValueError):
        st.mtf(0, f_max=n_px / (2 * size) * 1.001)
    with pytest.raises(ValueError):
        st.mtf(1)
    with pytest.raises(RuntimeError):
        m.f = None


def hand_built():
    """Two bands, W = 2 and 1, kappa_mean = 2000 and 1000 per mm: W kappa^2 = 8e6 and 1e6, g = 8/9 and 1/9.  The combine step is
    the device's; here the formulas of the definition on the host, as `HuygensStack` holds them."""
    W, kb, A = np.array([2.0, 1.0]), np.array([2000.0, 1000.0]), np.array([10.0, 4.0])
    g = W * kb ** 2 / (W * kb ** 2).sum()
    assert g == pytest.approx([8 / 9, 1 / 9], rel=1e-15)
    band_strehl = np.array([[0.9, 0.45], [0.5, 0.9]])
    strehl = band_strehl @ g
    assert strehl == pytest.approx([0.85, 49 / 90], rel=1e-15)
    floor = (g * W / A ** 2).sum()
    assert floor == pytest.approx(8 / 9 * 0.02 + 1 / 9 / 16, rel=1e-15)
    inten = np.stack([np.full((2, 2), 0.1), np.full((2, 2), 0.2)])
    inten[0, 1, 1], inten[1, 0, 0] = 0.85, 0.5
    st = ot.HuygensStack(30, 3.0, 1, 4, 2, (0, 0, 20), 9.0, 0.02, [-0.1, 0.1], [400, 500, 700], [20, 10], W, [450.0, 600.0], g, inten, strehl,
                         band_strehl, floor, long_desc="by hand")
    assert st.N == 30 and st.power == 3 and st.n_missed == 1 and st.n_out_of_band == 4 and st.section == 2 and st.radius == 9
    assert st.best_focus == -0.1 and st.peak.tolist() == [0.85, 0.5] and st.wavelength == pytest.approx((2 * 450 + 600) / 3, rel=1e-15)
    assert st.band_N.dtype == np.int64 and st.band_edges.tolist() == [400, 500, 700] and st.dz.tolist() == [-0.1, 0.1]
    return st


def test_band_weights_by_hand():
    hand_built()


def test_result_object():
    st = hand_built()
    assert ot.HuygensStack._tracked is False
    with pytest.raises(RuntimeError):
        st.strehl = None
    for arr in (st.intensity, st.strehl, st.band_strehl, st.dz, st.band_weight, st.focus):
        assert not arr.flags.writeable
    with pytest.raises(AttributeError):
        st.something_else = 1
    one = st.psf(1)
    assert isinstance(one, ot.HuygensPSF) and one.dz == 0.1 and one.strehl == st.strehl[1] and one.peak == 0.5 and one.N == 30
    assert np.array_equal(one.intensity, st.intensity[1]) and one.noise_floor == st.noise_floor and one.size == 0.02
    assert one.wavelength == st.wavelength and one.long_desc == "by hand" and st.psf().dz == -0.1
    img = st.to_image(1)
    assert isinstance(img, ot.GrayscaleImage) and img.shape == (2, 2) and img.data[0, 0] == pytest.approx(1, abs=1e-15)
    assert np.array_equal(img.data, one.to_image().data) and np.argmax(st.to_image().data) == 3
    for bad, error in ((2, ValueError), (-1, ValueError), (1.0, TypeError)):
        with pytest.raises(error):
            st.psf(bad)
    # first maximum of equal Strehl ratios
    tie = ot.HuygensStack(1, 1.0, 0, 0, 0, (0, 0, 1), 1.0, 0.1, [0.3, -0.2, 0.1], None, [1], [1.0], [500.0], [1.0], np.ones((3, 1, 1)),
                          [0.5, 0.7, 0.7], np.ones((3, 1)), 1.0)
    assert tie.best_focus == -0.2 and tie.band_edges is None


def test_empty_result():
    dz = np.array([-0.5, 0.0, 0.5])
    st = hp._empty_stack(2, None, None, 5, None, dz, "lines", long_desc="nothing")
    assert isinstance(st, ot.HuygensStack) and st.N == 0 and st.power == 0 and st.n_missed == 0 and st.n_out_of_band == 0
    assert st.intensity.shape == (3, 5, 5) and np.all(np.isnan(st.intensity)) and st.band_edges is None
    assert st.strehl.shape == (3,) and st.band_strehl.shape == (3, 1) and st.peak.shape == (3,) and st.band_N.tolist() == [0]
    for val in (st.strehl, st.band_strehl, st.peak, st.noise_floor, st.best_focus, st.wavelength, st.band_wavelength, st.band_weight,
                st.focus, st.radius, st.size):
        assert np.all(np.isnan(val))
    assert np.array_equal(st.dz, dz) and st.section == 2
    edges = np.array([400.0, 500.0, 600.0])
    kept = hp._empty_stack(0, np.array([0.0, 0.0, 1.0]), 2.0, 1, 0.25, dz[:1], edges, n_missed=7, n_out_of_band=3)
    assert np.array_equal(kept.focus, [0, 0, 1]) and kept.radius == 2 and kept.size == 0.25 and kept.n_missed == 7 and kept.n_out_of_band == 3
    assert np.array_equal(kept.band_edges, edges) and kept.band_strehl.shape == (1, 2) and kept.band_power.tolist() == [0, 0]
    pc.check_empty(kept.psf(0), 1)
    with pytest.raises(RuntimeError):
        kept.to_image()
