"""Raytracer.mtf_analysis and the `ot_mtf_*` entry points on the GPU.

Truth is NumPy longdouble following the definition (tests/mtf_cases.py): on synthetic storages handed to the entry points through
ctypes -- the storages of tests/test_gpu_field.py --, and on the device's own ray storage read back for traced scenes.

Bounds, as stated with the feature: every sum within the oracle's allowance, taken about the means the device forms from its own
`ot_field_sums` record, which are an input of the pass; two calls return the same bits; a field's sums do not depend on the other
fields of the call; the column of nu = 0 is slot 0 of the record within (n + 40) eps of it, its imaginary parts are 0."""
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
import mtf_cases as mc
import scenes
from test_gpu_field import build, dev, double_gauss, flat_ranges, ideal_scene, same_bits

pytestmark = pytest.mark.gpu

EPS = mc.EPS
ORIGIN = (0.25, -0.5, 9.5)
DIRECTIONS = [(0.0, 1.0), (0.6, 0.8), (-0.8, 0.6), (1.0, 0.0)]  # (per field in turn: on the axes and on diagonals)


def planes_and_frequencies(Z, Q):
    zeta = np.array([0.75]) if Z == 1 else np.linspace(-1.5, 2.0, Z)
    freq = np.linspace(0.0, 40.0, Q) if Q > 1 else np.array([0.0 if Z == 1 else 25.0])
    return zeta, freq


def call_mtf(S, fields, k, key, key_first, K, t, zeta, freq, origin=ORIGIN):
    """`ot_field_sums`, then `ot_mtf_sums` on its records.  -> (records (F, K, 18), sums (F, K, Z, Q, 4)) on the host"""
    lib = _capi.load_library()
    F, Z, Q = len(fields), len(zeta), len(freq)
    flat, d_key, org = flat_ranges(fields), to_dev(key, np.uint8), (C.c_double * 3)(*origin)
    ws = torch.full((lib.ot_field_workspace(flat, F, K),), np.nan, dtype=torch.float64, device=dev())
    rec = torch.full((F * K * fc.M,), -7.0, dtype=torch.float64, device=dev())
    _capi.check(lib.ot_field_sums(C.byref(S.rays), flat, F, k, ptr(d_key), key_first, K, org, ptr(ws), ptr(rec), stream_ptr()))
    n_ws = lib.ot_mtf_workspace(flat, F, K, Z, Q)
    assert n_ws == mc.workspace([n for _, n in fields], K, Z, Q)
    ws = torch.full((n_ws,), np.nan, dtype=torch.float64, device=dev())  # (a partial read before it is written shows)
    sums = torch.full((F * K * Z * Q * 4,), -7.0, dtype=torch.float64, device=dev())
    d_freq = to_dev(freq, np.float64)
    _capi.check(lib.ot_mtf_sums(C.byref(S.rays), flat, F, k, ptr(d_key), key_first, K, org, ptr(rec),
                                (C.c_double * (2 * F))(*np.asarray(t, dtype=np.float64).reshape(-1)), (C.c_double * Z)(*zeta), Z,
                                ptr(d_freq), Q, ptr(ws), ptr(sums), stream_ptr()))
    return rec.cpu().numpy().reshape(F, K, fc.M), sums.cpu().numpy().reshape(F, K, Z, Q, 4)


def check_entry_point(S, fields, k, key, key_first, K, Z, Q, what, alone=None):
    """-> (records, sums) of the device, the sums checked against the oracle; twice the same bits; the fields `alone` (default: all
    with rays), each on its own, give the bits they have among the others; the column of nu = 0."""
    zeta, freq = planes_and_frequencies(Z, Q)
    t = np.array([DIRECTIONS[f % 4] for f in range(len(fields))])
    rec, sums = call_mtf(S, fields, k, key, key_first, K, t, zeta, freq)
    rec2, sums2 = call_mtf(S, fields, k, key, key_first, K, t, zeta, freq)
    assert same_bits(rec, rec2) and same_bits(sums, sums2), f"{what}: two calls, different bits"
    val, allow, n = mc.sums(S.p, S.w, fields, k, key, key_first, K, ORIGIN, fc.record_means(rec), t, zeta, freq)
    assert np.array_equal(n, rec[:, :, 1])
    mc.check_sums(sums, val, allow, what)
    assert np.all(sums[n == 0] == 0), f"{what}: the sums of a cell without a ray"
    if freq[0] == 0:
        W = rec[:, :, 0:1]
        for c in (0, 2):
            assert np.all(np.abs(sums[:, :, :, 0, c] - W) <= (n[:, :, None] + 40) * EPS * W), f"{what}: nu = 0 against the power"
            assert np.all(sums[:, :, :, 0, c + 1] == 0), f"{what}: nu = 0 has a phase"
    if len(fields) > 1:
        for f in (range(len(fields)) if alone is None else alone):
            if fields[f][1]:
                one = call_mtf(S, [fields[f]], k, key, key_first, K, t[f:f + 1], zeta, freq)
                assert same_bits(rec[f], one[0][0]) and same_bits(sums[f], one[1][0]), f"{what}: field {f} alone differs"
    return rec, sums


@pytest.mark.parametrize("counts,gaps,nt,k,first,K,Z,Q", [
    ([1], None, 2, 0, 5, 1, 1, 1),
    ([63, 64, 65], None, 5, 3, 5, 3, 1, 8),                     # around a wave; one full tile
    ([65, 255, 256], [0, 7, 0], 2, 0, 33, 32, 65, 64),          # around a workgroup, every band, the most planes and frequencies
    ([257, 0, 3000], [5, 0, 11], 5, 3, 7, 3, 3, 64),            # a field of no rays between two, gaps of rays of no field
    ([3000, 1, 64], [1, 1, 1], 5, 0, 3, 32, 65, 1),             # a field of one ray; a tile that ends within a plane's row
    ([256 * 1024 + 1, 65], [3, 0], 2, 0, 7, 3, 1, 9),           # more rays than a field's launch has lanes; a second tile of one pair
    ([3000], None, 5, 3, 64, 1, 1, 9),
    ([64, 300], None, 2, 0, 5, 2, 3, 64),                       # two bands side by side in a lane
    ([300, 65], [2, 0], 5, 3, 9, 5, 1, 9),                      # two groups of bands, the second of one band
])
def test_entry_point_on_random_planes(counts, gaps, nt, k, first, K, Z, Q):
    seed = sum(counts) + 7 * nt + K
    S, fields, key, key_first = build(counts, nt, k, first, K, seed, gaps=gaps)
    check_entry_point(S, fields, k, key, key_first, K, Z, Q, f"fields of {counts} rays, nt {nt}, section {k}, {K} bands, {Z} x {Q}")


def test_sixty_four_fields_and_the_last_ends_with_the_storage():
    counts = [(37 * f) % 131 + (f % 3 == 0) for f in range(64)]
    S, fields, key, key_first = build(counts, 4, 2, 13, 3, 8, gaps=[(f + 1) % 2 for f in range(64)], behind=0)
    assert fields[-1][0] + fields[-1][1] == S.N and any(a % 16 for a, _ in fields)
    check_entry_point(S, fields, 2, key, key_first, 3, 3, 64, "64 fields", alone=(1, 17, 63))


def test_no_ray_in_any_field_launches_nothing():
    S, fields, key, key_first = build([10], 3, 0, 0, 2, 2)
    lib = _capi.load_library()
    sums = torch.full((2 * 2 * 4,), -7.0, dtype=torch.float64, device=dev())
    ws = torch.zeros(256, dtype=torch.float64, device=dev())
    d_key, d_freq = to_dev(key, np.uint8), to_dev(np.zeros(1), np.float64)
    _capi.check(lib.ot_mtf_sums(C.byref(S.rays), flat_ranges([(10, 0), (3, 0)]), 2, 0, ptr(d_key), 0, 2, (C.c_double * 3)(0, 0, 0),
                                ptr(ws), (C.c_double * 4)(0, 1, 0, 1), (C.c_double * 1)(0.5), 1, ptr(d_freq), 1, ptr(ws), ptr(sums),
                                stream_ptr()))
    assert np.all(sums.cpu().numpy() == -7.0) and np.all(ws.cpu().numpy() == 0)


# ---- Raytracer.mtf_analysis on traced rays -------------------------------------------------------------------------------------------
def check_analysis(RT, ma, sources, section, bands, what):
    """The sums of `ma` against the truth formed from the storage read back, about the means of its records.  -> (val, allow)"""
    p, w, wl = RT.rays.p_list, RT.rays.w_list, RT.rays.wl_list
    nt = w.shape[1]
    k = nt - 2 if section is None else section
    fields = [(int(RT.rays.B_list[s]), int(RT.rays.B_list[s + 1] - RT.rays.B_list[s])) for s in sources]
    origin = np.array(SectionTable(RT).origin(k, None), dtype=np.float64)
    used = np.zeros(w.shape[0], dtype=bool)
    for first, count in fields:
        used[first:first + count] = cc.used_rays(p, w, first, count, k)[0]
    key, K, edges = cc.band_keys(wl, used, bands)
    assert ma.n_bands == K and ma.section == k and ma.n_fields == len(sources) and ma.sources.tolist() == list(sources)
    assert np.array_equal(ma.origin, origin) and (ma.band_edges is None if edges is None else np.array_equal(ma.band_edges, edges))
    val, allow, n = mc.sums(p, w, fields, k, key, 0, K, origin, fc.record_means(ma.records), ma.t, ma.planes - origin[2], ma.frequencies)
    assert np.array_equal(n, ma.band_N)
    mc.check_sums(ma.sums, val, allow, what)
    return val, allow


def test_an_ideal_lens_has_the_mtf_one_on_its_image_plane_and_its_peak_there():
    with ot.global_options.no_warnings():
        RT = ideal_scene()
        RT.trace(6000)
    image_z = RT.tma(550.0).image_position(-30.0)
    dz, freq = np.array([-0.2, -0.1, 0.0, 0.1, 0.2]), np.array([0.0, 10.0, 50.0])
    ma = RT.mtf_analysis(z=image_z, dz=dz, frequencies=freq)
    assert (ma.n_fields, ma.n_bands, ma.n_planes, ma.n_frequencies) == (3, 1, 5, 3) and np.all(ma.band_N[:, 0] == 2000)
    assert np.array_equal(ma.planes, image_z + dz) and np.allclose(ma.t, [[0, 1]] * 3) and "RS0, RS1, RS2" in ma.long_desc
    val, allow = check_analysis(RT, ma, [0, 1, 2], None, "lines", "ideal lens")
    # on the image plane every ray of a field goes through one point up to the rounding of the trace: MTF 1 within the allowance
    # of the sums over the power
    W = ma.band_power[:, 0, None, None]
    off = np.stack([np.abs(ma.mtf_t[:, 0, 2] - 1), np.abs(ma.mtf_s[:, 0, 2] - 1)], axis=-1)
    print(f"ideal lens: MTF on the image plane off 1 by at most {off.max():.3e}, allowed {(allow[:, 0, 2] / W).min():.3e}; "
          f"through-focus peaks {ma.focus_mtf_t[:, 0, 1:].ravel() - image_z}")
    assert np.all(off <= allow[:, 0, 2] / W)
    assert np.all(ma.mtf_t[:, 0, [0, 4], 2] < 0.9)  # (a tenth of a millimetre away the contrast at 50 cycles per mm has dropped)
    # planes symmetric about the image: the peak of the parabola lies on it (nu = 0 has no peak: 1 on every plane, the first counts)
    for peak in (ma.focus_mtf_t, ma.focus_mtf_s):
        assert np.all(np.isnan(peak[:, 0, 0])) and np.all(np.abs(peak[:, 0, 1:] - image_z) <= 1e-9 * image_z)
    # one plane, the default one and the default frequencies: those of the field analysis
    fa = RT.field_analysis()
    mb = RT.mtf_analysis(frequencies=[20.0])
    assert mb.z == fa.z and mb.planes.tolist() == [fa.z] and same_bits(mb.records, fa.records) and np.all(np.isnan(mb.focus_mtf_t))


def test_double_gauss_three_fields_three_lines_five_planes():
    RT = double_gauss()
    fa = RT.field_analysis(sources=[0, 1, 2])
    dz = np.array([-0.4, -0.15, 0.0, 0.2, 0.5])
    ma = RT.mtf_analysis(sources=[0, 1, 2], dz=dz)
    check_analysis(RT, ma, [0, 1, 2], None, "lines", "double Gauss, sources 0 1 2")
    assert ma.n_bands == 3 and ma.reference_band == 1 and ma.z == fa.z and same_bits(ma.records, fa.records)
    assert np.array_equal(ma.planes, fa.z + dz) and np.array_equal(ma.frequencies, np.linspace(0, 1 / fa.rms_radius[0, 1], 17))
    assert np.allclose(ma.wavelengths, [486.1327, 589.2938, 656.272], rtol=1e-6) and np.allclose(ma.t, [[0, 1], [0, -1], [0, -1]])
    assert np.array_equal(ma.band_N, fa.band_N) and np.array_equal(ma.centroid[:, :, 2], fa.centroid)
    assert np.all(ma.mtf_t[:, :, :, 0] == pytest.approx(1.0, abs=1e-12)) and np.all(ma.mtf_t_all <= 1 + 1e-12)
    print(f"double Gauss: mtf_t_all on z {ma.mtf_t_all[:, 2, ::4]}, mtf_s_all {ma.mtf_s_all[:, 2, ::4]}")
    # the order of the sources is the order of the result
    mb = RT.mtf_analysis(sources=[2, 0], dz=dz, z=ma.z, frequencies=ma.frequencies)
    assert mb.sources.tolist() == [2, 0] and same_bits(mb.sums[0], ma.sums[2]) and same_bits(mb.sums[1], ma.sums[0])
    assert same_bits(mb.mtf_t_all[1], ma.mtf_t_all[0]) and np.array_equal(mb.field, ma.field[[2, 0]], equal_nan=True)
    # an earlier section, bands as edges, one plane
    edges = np.array([450.0, 550, 600, 700])
    me = RT.mtf_analysis(sources=[1, 3], section=3, bands=edges, z=0.0, frequencies=[0.0, 0.01, 0.02])
    check_analysis(RT, me, [1, 3], 3, edges, "double Gauss, section 3, edges")


def test_one_band_on_the_axis_against_the_spot_analysis_on_a_detector_there():
    """`bands=1` on the field on the axis, t = (0, 1): mtf_t is the spot's mtf_y and mtf_s its mtf_x on a detector at the plane z.
    Tolerance: the spot test's own for the device against its hit list (2e-13 + 2 pi nu d, d = 2e-13 of the mean absolute
    coordinate), plus 2 pi nu_max 64 eps max(|x| + |zeta m|) for the two ways of forming the crossing point."""
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=7)
        RT.trace(20000)
        z = RT.mtf_analysis(sources=[0], bands=1, frequencies=[0.0]).z
        RT.detectors[0].move_to([0, 0, z])  # (a detector is no part of what a trace depends on: the rays stay current)
        ma = RT.mtf_analysis(sources=[0], bands=1, z=z)
        sa = RT.spot_analysis(0, 0, frequencies=ma.frequencies)
    assert ma.n_bands == 1 and ma.band_N[0, 0] == sa.N and np.allclose(ma.t, [[0, 1]])
    p, w = RT.rays.p_list, RT.rays.w_list
    first, count, k = int(RT.rays.B_list[0]), int(RT.rays.B_list[1] - RT.rays.B_list[0]), w.shape[1] - 2
    _, inside, am = fc.lines(p, w, first, count, k, ma.origin)
    zeta = z - ma.origin[2]
    wt = w[first:first + count, k][inside].astype(np.float64)
    x = ma.origin[:2] + am[inside, :2] + zeta * am[inside, 2:]
    reach = np.max(np.abs(ma.origin[:2]) + np.abs(am[inside, :2]) + np.abs(zeta * am[inside, 2:]), axis=0)
    d = 2e-13 * (wt[:, None] * np.abs(x)).sum(axis=0) / wt.sum()
    nu = ma.frequencies
    for mine, theirs, c in ((ma.mtf_t[0, 0, 0], sa.mtf_y, 1), (ma.mtf_s[0, 0, 0], sa.mtf_x, 0)):
        tol = 2e-13 + 2 * np.pi * nu * d[c] + 2 * np.pi * nu.max() * 64 * EPS * reach[c]
        apart = np.abs(mine - theirs)
        print(f"axis {c}: MTF against the spot analysis off by at most {apart.max():.3e}, allowed {tol.min():.3e} .. {tol.max():.3e}")
        assert np.all(apart <= tol)
    assert np.all(np.abs(ma.centroid[0, 0, 0] - sa.centroid) <= d + 64 * EPS * reach)


def test_deferred_planes_are_neither_read_nor_filled():
    """A trace that generates its rays on the device leaves the index plane and the polarisation planes unwritten.  The MTF of such
    a storage, its unwritten planes poisoned, is that of the storage once it is complete, bit for bit, and asking for it fills
    nothing."""
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=11)
        RT.trace(20000)
    r = RT.rays
    assert r._pol_stale is not None and r._n_stale
    raw = lambda key: dict.__getitem__(r._dev, key)
    raw("n").fill_(float("nan"))
    raw("pol").fill_(float("nan"))
    before = RT.mtf_analysis(sources=[0, 2, 4], dz=[-0.1, 0.0, 0.1])
    assert r._pol_stale is not None and r._n_stale, "the MTF analysis filled a deferred plane"
    r._dev["n"], r._dev["pol"]  # (through the hook: the storage is complete now)
    assert r._pol_stale is None and not r._n_stale
    after = RT.mtf_analysis(sources=[0, 2, 4], dz=[-0.1, 0.0, 0.1])
    assert same_bits(before.sums, after.sums) and before.z == after.z and before.n_bands == 3
    check_analysis(RT, after, [0, 2, 4], None, "lines", "device-generated double Gauss")


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
    ma = RT.mtf_analysis(dz=[-0.5, 0.0, 0.5])
    assert ma.band_N[:, 0].tolist() == [N, 0] and np.all(np.isfinite(ma.mtf_t[0])) and np.all(ma.sums[1] == 0)
    assert np.all(np.isnan(ma.mtf_t[1])) and np.all(np.isnan(ma.centroid[1])) and np.all(np.isnan(ma.mtf_s_all[1]))
    assert 5 < ma.z < 12 and ma.frequencies.shape == (17,) and ma.frequencies[0] == 0 and np.all(np.abs(ma.mtf_t[0, 0, :, 0] - 1) <= 1e-12)
    check_analysis(RT, ma, [0, 1], None, "lines", "a source without rays")
    # the reference field has no ray: no default plane; and with a plane no default frequencies
    with pytest.raises(RuntimeError, match="pass `z`"):
        RT.mtf_analysis(reference_field=1)
    with pytest.raises(ValueError, match="pass `frequencies`"):
        RT.mtf_analysis(reference_field=1, z=8.0)
    # no chosen ray at all: the empty result, what the caller fixed stays
    e = RT.mtf_analysis(sources=[1], bands=np.array([400.0, 500, 600]), z=3.0, dz=[0.0, 1.0], frequencies=[5.0])
    assert e.n_bands == 2 and e.z == 3.0 and e.reference_band == -1 and e.band_N.tolist() == [[0, 0]] and e.sources.tolist() == [1]
    assert e.planes.tolist() == [3.0, 4.0] and e.frequencies.tolist() == [5.0] and np.all(np.isnan(e.mtf_t)) and e.mtf_t.shape == (1, 2, 2, 1)
    e = RT.mtf_analysis(sources=[1])
    assert e.n_bands == 1 and np.isnan(e.z) and e.band_edges is None and e.frequencies.shape == (17,) and np.all(np.isnan(e.planes))
    # rays outside every band: the empty result too
    assert RT.mtf_analysis(bands=np.array([600.0, 700]), z=5.0, frequencies=[1.0]).band_N.sum() == 0
