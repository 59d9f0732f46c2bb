"""Raytracer.huygens_field and the `ot_psf_field_*` entry points on the GPU.

Truth of the sum is `psf_cases.truth` (NumPy longdouble, the definition of DESIGN.md "Huygens PSF") applied to each cell's slice of
the grouped records with the radius of the cell's field and each plane's dz; the bound it returns is the tolerance, per point and
for Re and Im alike, as in tests/test_gpu_psf_stack.py.  Each pass is measured on the inputs it was given: the sum against the
grouped records, the combine step and the transfer function against the device's own field, sums and intensity, the whole call
against the records the device forms."""
import ctypes as C

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd import psf_field as pf
from optrace_amd._device import ptr, stream_ptr, to_dev
from optrace_amd.presets import spectral_lines

import psf_cases as pc
import scenes
import wavefront_cases as wc
from test_gpu_psf import check_records
from test_gpu_psf_stack import band_starts, call_stack, combine_by_definition, stack_truth
from test_gpu_wavefront import dev, within
from test_psf_field_host import exact_transfer, otf_bound

pytestmark = pytest.mark.gpu

EPS, LD = wc.EPS, wc.LD
RADII = [100.0, -60.0, 45.0]  # one per field


def call_field_sum(rec_d, starts, radius, F, K, n_px, size, dz):
    """`ot_psf_field_sum` on the device records rec_d (6 n) -> (field (F, Z, K, 2, n_px^2), sums (F, Z, K, 5)) on the host, the device
    tensors"""
    lib = _capi.load_library()
    n, Z, cells = rec_d.shape[0] // 6, len(dz), F * K
    assert len(starts) == cells + 1
    ws = torch.full((max(1, _capi.psf_field_ws(n, F, K, n_px, Z)),), np.nan, dtype=torch.float64, device=dev())
    table = torch.full((_capi.psf_field_table(cells),), -1, dtype=torch.int64, device=dev())
    field = torch.full((F * Z * K * 2 * n_px * n_px,), np.nan, dtype=torch.float64, device=dev())
    sums = torch.full((F * Z * K * 5,), np.nan, dtype=torch.float64, device=dev())
    _capi.check(lib.ot_psf_field_sum(n, ptr(rec_d), F, K, (C.c_int64 * (cells + 1))(*starts), (C.c_double * F)(*radius), n_px, float(size),
                                     Z, (C.c_double * Z)(*dz), ptr(table), ptr(ws), ptr(field), ptr(sums), stream_ptr()))
    return field.cpu().numpy().reshape(F, Z, K, 2, n_px * n_px), sums.cpu().numpy().reshape(F, Z, K, 5), field, sums


def call_field_combine(field_d, sums_d, F, K, Z, n_px):
    """-> (intensity (F, Z, n_px^2), band_strehl (F, Z, K), strehl (F, Z), g (F, K), noise_floor (F)), and the device buffer"""
    lib = _capi.load_library()
    parts = [F * Z * n_px * n_px, F * Z * K, F * Z, F * K, F]
    out = torch.full((sum(parts),), -7.0, dtype=torch.float64, device=dev())
    i, bs, s, g, fl = out.split(parts)
    _capi.check(lib.ot_psf_field_combine(F, K, Z, n_px, ptr(field_d), ptr(sums_d), ptr(i), ptr(bs), ptr(s), ptr(g), ptr(fl), stream_ptr()))
    i, bs, s, g, fl = np.split(out.cpu().numpy(), np.cumsum(parts)[:-1])
    return i.reshape(F, Z, n_px * n_px), bs.reshape(F, Z, K), s.reshape(F, Z), g.reshape(F, K), fl


def call_field_otf(inten, floor, t, n_px, size, freq):
    """intensity (F, Z, n_px, n_px), noise_floor (F), t (F, 2) on the host -> out (F, Z, M, 6) on the host"""
    lib = _capi.load_library()
    F, Z, M = inten.shape[0], inten.shape[1], len(freq)
    out = torch.full((F * Z * M * 6,), np.nan, dtype=torch.float64, device=dev())
    inten_d, floor_d = to_dev(inten.reshape(-1), np.float64), to_dev(floor, np.float64)  # (held until the result is read)
    _capi.check(lib.ot_psf_field_otf(F, Z, n_px, float(size), ptr(inten_d), ptr(floor_d),
                                     (C.c_double * (2 * F))(*np.asarray(t, dtype=np.float64).reshape(-1)), M, (C.c_double * M)(*freq),
                                     ptr(out), stream_ptr()))
    return out.cpu().numpy().reshape(F, Z, M, 6)


def field_records(counts, K, seed):
    """Records of F K cells with `counts` rays each, those of field f about a sphere of radius RADII[f].  -> (rec (6, n), starts)"""
    parts = [pc.synthetic_records(c, seed + 17 * i, RADII[i // K]) for i, c in enumerate(counts) if c]
    rec = np.concatenate(parts, axis=1) if parts else np.zeros((6, 0))
    return np.ascontiguousarray(rec), [0] + np.cumsum(counts).tolist()


def check_field_sum(rec, starts, F, K, n_px, size, dz):
    """`ot_psf_field_sum` on the host records rec (6, n), cells by `starts`, against the truth of every (cell, plane)."""
    Z = len(dz)
    field, sums, _, _ = call_field_sum(to_dev(rec, np.float64), starts, RADII[:F], F, K, n_px, size, dz)
    assert np.all(np.isfinite(field)) and np.all(np.isfinite(sums))
    for cell in range(F * K):
        f, b = divmod(cell, K)
        sl = rec[:, starts[cell]:starts[cell + 1]]
        nb = sl.shape[1]
        if not nb:
            assert not field[f, :, b].any() and not sums[f, :, b].any(), "a cell without a record gives zeros"
            continue
        a, kappa = sl[5].astype(LD), sl[4].astype(LD)
        for z in range(Z):
            re, im, bound, A, A2, _ = pc.truth(sl, RADII[f], n_px, size, dz[z])
            within(np.append(field[f, z, b, 0], sums[f, z, b, 0]), re, bound, f"Re U, field {f} plane {z} band {b}")
            within(np.append(field[f, z, b, 1], sums[f, z, b, 1]), im, bound, f"Im U, field {f} plane {z} band {b}")
            within(sums[f, z, b, 2], A, (nb + 40) * EPS * A, "sum a")
            within(sums[f, z, b, 3], A2, (nb + 40) * EPS * A2, "sum a^2")
            within(sums[f, z, b, 4], (a * a * kappa).sum(), (nb + 40) * EPS * (a * a * kappa).sum(), "sum a^2 kappa")


# ---- 1. the hot sum on grouped synthetic records --------------------------------------------------------------------------------------
# cells of 0, 1, 63, 65 and 257 records: an empty cell in the middle and an empty last one, a cell of one record, boundaries inside
# what would be a chunk (386 records of two fields in chunks of 97, of three fields in chunks of 65)
CELLS = {(1, 1, 1): [[1], [63], [65], [257]],
         (2, 3, 2): [[257, 0, 1, 65, 63, 0], [1, 63, 0, 0, 257, 65]],
         (3, 2, 1): [[65, 1, 0, 257, 63, 0], [0, 257, 63, 65, 1, 0]]}
SUM_CASES = [(fkz, i, n_px) for fkz, lists in CELLS.items() for i in range(len(lists)) for n_px in (1, 2, 33)]


@pytest.mark.parametrize("fkz,which,n_px", SUM_CASES)
def test_sum_of_synthetic_cells(fkz, which, n_px):
    F, K, Z = fkz
    counts = CELLS[fkz][which]
    rec, starts = field_records(counts, K, 1000 * sum(counts) + n_px + which)
    check_field_sum(rec, starts, F, K, n_px, 1.0 if which else 0.02, [0.05, -0.03][:Z])


def test_sum_of_two_fields_with_several_chunks_per_cell():
    """n = 70001 in two cells of two fields: chunks of 128 records, 235 and 313 to the cells."""
    rec, starts = field_records([30000, 40001], 1, 5)
    check_field_sum(rec, starts, 2, 1, 8, 0.02, [0.04])


def test_no_record_launches_nothing():
    out = torch.full((16,), -3.0, dtype=torch.float64, device=dev())
    rc = _capi.load_library().ot_psf_field_sum(0, ptr(out), 2, 1, (C.c_int64 * 3)(0, 0, 0), (C.c_double * 2)(1.0, -1.0), 4, 0.1, 1,
                                               (C.c_double * 1)(0.0), ptr(out), ptr(out), ptr(out), ptr(out), stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and np.array_equal(out.cpu().numpy(), np.full(16, -3.0))


# ---- 2., 3. bits --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_px,K,Z", [(257, 33, 5, 2), (70001, 8, 3, 2), (65, 2, 2, 3)])
def test_one_field_is_ot_psf_stack_bit_for_bit(n, n_px, K, Z):
    starts, dz = band_starts(n, K), [0.05, 0.0, -0.03][:Z]
    rec = to_dev(pc.synthetic_records(n, 3 * n, -80.0), np.float64)
    field, sums, _, _ = call_field_sum(rec, starts, [-80.0], 1, K, n_px, 0.03, dz)
    f1, s1, _, _ = call_stack(rec, starts, -80.0, n_px, 0.03, dz)
    assert np.array_equal(field[0], f1) and np.array_equal(sums[0], s1)


@pytest.mark.parametrize("counts,n_px", [([[400, 600], [1500, 0], [2749, 1]], 8), ([[30, 34], [64, 0], [1, 63]], 33)])
def test_fields_do_not_depend_on_each_other(counts, n_px):
    """F fields in one call against F calls of one field each, bit for bit; and the same call twice.  The chunk length is part of
    what fixes the bits, and it follows from the mean size of a call's fields with records: the two routes share it where 128 records per chunk
    is what limits the chunks on both and the counts divide alike -- 1000, 1500 and 2750 records in 8, 12 and 22 chunks of 125, their
    mean of 1750 in 14 --, or where every cell is one chunk (three fields of 64 records); beyond that they agree to the truth's bound
    only."""
    F, K, Z = len(counts), 2, 2
    dz = [0.05, -0.03]
    flat = [c for row in counts for c in row]
    n = sum(flat)
    tiles, mean = -(-(n_px * n_px + 1) // 1024), -(-n // F)
    chunk = lambda m: -(-m // -(-m // 128))
    assert -(-max(sum(row) for row in counts) // 128) <= 1024 * min(Z, 4) // (tiles * Z)
    rec, starts = field_records(flat, K, 7 * n)
    field, sums, _, _ = call_field_sum(to_dev(rec, np.float64), starts, RADII[:F], F, K, n_px, 0.02, dz)
    again = call_field_sum(to_dev(rec, np.float64), starts, RADII[:F], F, K, n_px, 0.02, dz)
    assert np.array_equal(field, again[0]) and np.array_equal(sums, again[1]), "two calls, different bits"
    for f in range(F):
        lo, hi = starts[f * K], starts[(f + 1) * K]
        own = [s - lo for s in starts[f * K:(f + 1) * K + 1]]
        assert chunk(mean) == chunk(hi - lo) or max(flat) <= min(chunk(mean), chunk(hi - lo)), "the two routes share the chunks"
        f1, s1, _, _ = call_field_sum(to_dev(np.ascontiguousarray(rec[:, lo:hi]), np.float64), own, [RADII[f]], 1, K, n_px, 0.02, dz)
        assert np.array_equal(field[f], f1[0]) and np.array_equal(sums[f], s1[0]), f"field {f}"


# ---- 4. the combine step ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("counts,K,n_px,Z", [([257, 0, 63, 0, 0, 0, 1, 65, 30], 3, 33, 2), ([65, 63], 1, 2, 3)])
def test_combine_against_the_definition(counts, K, n_px, Z):
    """`ot_psf_field_combine` against the formulas in float64 NumPy per field, on the device's own field and sums, to (10 + 2 K) eps,
    the bar and the reasoning of `test_gpu_psf_stack.test_combine_against_the_definition`.  A field without a ray: NaN, g = 0."""
    F = len(counts) // K
    rec, starts = field_records(counts, K, 31)
    field, sums, field_d, sums_d = call_field_sum(to_dev(rec, np.float64), starts, RADII[:F], F, K, n_px, 0.02, [0.0, 0.04, -0.02][:Z])
    inten, bs, s, g, floor = call_field_combine(field_d, sums_d, F, K, Z, n_px)
    tol = (10 + 2 * K) * EPS
    for f in range(F):
        if not sum(counts[f * K:(f + 1) * K]):
            assert np.all(np.isnan(inten[f])) and np.all(np.isnan(s[f])) and np.isnan(floor[f]) and np.all(np.isnan(bs[f])) and not g[f].any()
            continue
        w_i, w_bs, w_s, w_g, w_floor = combine_by_definition(field[f], sums[f])
        print("bit for bit:", np.array_equal(inten[f], w_i), np.array_equal(s[f], w_s), np.array_equal(g[f], w_g), floor[f] == w_floor)
        within(inten[f], w_i, tol * w_i, f"intensity, field {f}")
        within(s[f], w_s, tol * w_s, f"strehl, field {f}")
        within(g[f], w_g, tol * w_g, f"g, field {f}")
        within(floor[f], w_floor, tol * w_floor, f"noise floor, field {f}")
        empty = sums[f, 0, :, 3] == 0
        assert np.all(np.isnan(bs[f][:, empty])) and np.all(g[f][empty] == 0)
        within(bs[f][:, ~empty], w_bs[:, ~empty], tol * w_bs[:, ~empty], f"band strehl, field {f}")
        assert g[f].sum() == pytest.approx(1, abs=K * EPS)


# ---- 5. the transfer function -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_px,size", [(16, 0.05), (33, 0.8), (1, 0.01)])
def test_transfer_function(n_px, size):
    """`ot_psf_field_otf` for t = (0, 1), (1, 0) and (0.6, 0.8) on two planes, at six frequencies from 0 to the sampling limit (two
    blocks of four, the second half empty), against sum_p J_p exp(-2 pi i nu (d . x_p)) in longdouble within
    (n_px^2 + 6 pi nu size + 16) eps sum_p |J_p| -- n_px^2 + 16 for the additions and the sine-cosine kernels, three roundings of a
    phase of at most nu size turns.  The float64 restatement `psf_field.transfer` follows the device's order, but its sines and
    cosines are NumPy's and the device's are polynomial kernels of its own: bit for bit is reported, not asked for; at nu = 0, where
    both are exact, it is."""
    rng = np.random.default_rng(n_px)
    t = np.array([[0.0, 1.0], [1.0, 0.0], [0.6, 0.8]])
    inten = rng.uniform(0.0, 1.0, (3, 2, n_px, n_px)) * np.exp(-rng.uniform(0, 6, (3, 2, n_px, n_px)))
    floor = np.array([1e-3, 0.0, 2e-2])
    limit = pf.sampling_limit(n_px, size)
    freq = [0.0, limit / 7, limit / 3, 0.5 * limit, 0.9 * limit, limit]
    out = call_field_otf(inten, floor, t, n_px, size, freq)
    assert np.all(np.isfinite(out))
    same = 0
    for f in range(3):
        for z in range(2):
            J = inten[f, z] - floor[f]
            bound = otf_bound(J, n_px, size, freq)
            want = exact_transfer(inten[f, z], floor[f], size, t[f], freq)
            for k, name in enumerate(("t", "s")):
                within(out[f, z, :, 2 * k], want[k].real, bound, f"Re OTF_{name}, field {f} plane {z}")
                within(out[f, z, :, 2 * k + 1], want[k].imag, bound, f"Im OTF_{name}, field {f} plane {z}")
                mod = np.sqrt(out[f, z, :, 2 * k].astype(LD) ** 2 + out[f, z, :, 2 * k + 1].astype(LD) ** 2)
                j0 = abs(LD(out[f, z, 0, 2 * k]))
                within(out[f, z, :, 4 + k], mod / j0, 4 * EPS * mod / j0, f"MTF_{name}: two squares, a sum, a root and a quotient")
            host = pf.transfer(inten[f, z], floor[f], size, t[f], freq)
            assert out[f, z, 0, 0] == host[0][0].real == out[f, z, 0, 2] and out[f, z, 0, 1] == 0 and out[f, z, 0, 3] == 0, "nu = 0: sum J"
            assert out[f, z, 0, 4] == 1 and out[f, z, 0, 5] == 1
            same += int(np.array_equal(out[f, z, :, 0], host[0].real) and np.array_equal(out[f, z, :, 2], host[1].real))
    print(f"float64 restatement bit for bit in {same} of 6 tiles")


# ---- 6. a traced scene ----------------------------------------------------------------------------------------------------------------------
F_LINE, C_LINE = spectral_lines.F, spectral_lines.C
N_RAYS, N_PX, DZ = 20000, 16, [0.0, 0.05]


@pytest.fixture(scope="module")
def traced():
    """The singlet of `scenes.c1_single_lens` with its source replaced by three point sources of the F and C lines at three field
    points, each aimed at the lens, and a fourth aimed past it; 20 000 rays."""
    RT = scenes.c1_single_lens(ot, no_pol=True, seed=5)
    RT.remove(RT.ray_sources[0])
    spectrum = ot.LightSpectrum("Lines", lines=[F_LINE, C_LINE], line_vals=[1, 1])
    for x, y in ((0.0, 0.0), (0.6, 0.8), (0.0, 2.0)):
        RT.add(ot.RaySource(ot.Point(), divergence="Isotropic", div_angle=1.5, pos=[x, y, -20], s=[-x, -y, 20], spectrum=spectrum))
    RT.add(ot.RaySource(ot.Point(), divergence="Isotropic", div_angle=1.5, pos=[0, -1, -20], s=[0, 9, 20], spectrum=spectrum))
    with ot.global_options.no_warnings():
        RT.trace(N_RAYS)
        hf = RT.huygens_field(sources=[0, 1, 2], n_px=N_PX, dz=DZ)
    return RT, hf


def own_records(RT, hf):
    """The records of the fields of `hf` as the device forms them: `ot_wavefield_paths` and `_moments` with the spheres of `hf`,
    then `ot_psf_field_rays`.  -> (rec (6, span) on the host, lo, band key per entry on the host, K)"""
    lib = _capi.load_library()
    rays = RT.rays
    F, K, k = hf.n_fields, hf.n_bands, hf.section
    ranges = [RT._stored_range(int(s)) for s in hf.sources]
    lo, hi = min(a for a, _ in ranges), max(e for _, e in ranges)
    span = hi - lo
    flat = (C.c_int64 * (2 * F))(*[v for a, e in ranges for v in (a, e - a)])
    wl = rays._dev["wl"][lo:hi]
    lines = np.float32([F_LINE, C_LINE])
    key = np.full(span, 255, dtype=np.uint8)
    hwl = wl.cpu().numpy()
    for b in range(K):
        key[hwl == lines[b]] = b
    key_d = to_dev(key, np.uint8)
    rays._dev["n"]
    R = rays._rays_struct()
    spheres = np.concatenate([hf.focus, hf.radius[:, None]], axis=1)[:, None, :].repeat(K, axis=1)
    u, v, opl = (torch.full((span,), np.nan, dtype=torch.float64, device=dev()) for _ in range(3))
    w = torch.zeros(span, dtype=torch.float32, device=dev())
    counts = torch.zeros(F * K * 2, dtype=torch.int64, device=dev())
    mom = torch.zeros(F * K * _capi.WFF_M, dtype=torch.float64, device=dev())
    pupil = torch.zeros(F * _capi.WFF_PUPIL_M, dtype=torch.float64, device=dev())
    ws = torch.empty(max(1, lib.ot_wavefield_workspace(flat, F, K, 1)), dtype=torch.float64, device=dev())
    st = stream_ptr()
    d_sph = to_dev(spheres.reshape(-1), np.float64)
    _capi.check(lib.ot_wavefield_paths(C.byref(R), flat, F, k, ptr(key_d), lo, K, ptr(d_sph), ptr(u), ptr(v), ptr(opl), ptr(w), ptr(counts), st))
    _capi.check(lib.ot_wavefield_moments(flat, F, ptr(u), ptr(v), ptr(opl), ptr(w), ptr(wl), ptr(key_d), lo, K, ptr(ws), ptr(mom), ptr(pupil), st))
    rec = torch.full((6 * span,), -7.0, dtype=torch.float64, device=dev())
    _capi.check(lib.ot_psf_field_rays(C.byref(R), flat, F, k, ptr(key_d), lo, span, K, ptr(d_sph), ptr(opl), ptr(mom), ptr(rec), st))
    return rec.cpu().numpy().reshape(6, span), lo, key, ranges, pupil.cpu().numpy().reshape(F, -1)


def test_traced_fields_against_the_definition(traced):
    """Three fields, two lines, two planes, 16 x 16 points: every figure of every field against the longdouble definition on the
    device's own records, grouped here by (field, band) in ray order; then, per field, the records against those of
    `huygens_stack` for the same sphere."""
    RT, hf = traced
    assert isinstance(hf, ot.HuygensField) and hf.sources.tolist() == [0, 1, 2] and hf.section == 2 and hf.band_edges is None
    assert hf.intensity.shape == (3, 2, N_PX, N_PX) and hf.mtf_t.shape == (3, 2, 17) and hf.frequencies[-1] == pf.sampling_limit(N_PX, hf.size)
    assert np.array_equal(hf.wavelengths, np.float32([F_LINE, C_LINE]).astype(np.float64)) and hf.dz.tolist() == DZ
    assert hf.band_N.sum() == sum(e - a for a, e in (RT._stored_range(s) for s in range(3))) and np.all(hf.band_N > 2000)
    assert not hf.n_missed.any() and not hf.n_no_sphere.any() and np.all(np.isfinite(hf.focus)) and np.all(hf.radius > 0)
    assert np.allclose(hf.t, [[0, 1], [0.6, 0.8], [0, 1]]) and np.allclose(hf.band_weight.sum(axis=1), 1, atol=4 * EPS)
    assert np.all(hf.band_weight[:, 0] > hf.band_weight[:, 1]), "(n / lambda)^2 favours F"
    assert np.all(hf.focus[1:, 1] < 0) and hf.focus[1, 0] < 0, "the images lie across the axis from their sources"

    rec, lo, key, ranges, pupil = own_records(RT, hf)
    K = hf.n_bands
    lam = (hf.band_power * hf.wavelengths).sum(axis=1) / hf.band_power.sum(axis=1) * 1e-6
    assert hf.size == pytest.approx((10 * lam / pupil[:, 3]).max(), rel=1e-12), "the default size: the largest 10 lambda_f / rho_f"
    axis = N_PX * N_PX
    pts = np.append(np.arange(0, N_PX, 2) * (N_PX + 1), axis)  # eight points of the diagonal and the axis
    for f, (a, e) in enumerate(ranges):
        sl, kf = rec[:, a - lo:e - lo], key[a - lo:e - lo]
        live = sl[5] != 0
        groups = [sl[:, live & (kf == b)] for b in range(K)]
        starts = [0] + np.cumsum([g.shape[1] for g in groups]).tolist()
        assert np.array_equal(np.diff(starts), hf.band_N[f])
        rec_g = np.concatenate(groups, axis=1)
        n = rec_g.shape[1]
        for z in range(2):
            p = np.append(np.arange(axis), axis) if (f, z) == (1, 0) else pts
            value, bound, per_band, per_bound, g = stack_truth(rec_g, starts, hf.radius[f], N_PX, hf.size, DZ[z], p)
            within(hf.intensity[f, z].ravel()[p[:-1]], value[:-1], bound[:-1], f"intensity, field {f} plane {z}")
            within(hf.strehl[f, z], value[-1], bound[-1], f"strehl, field {f} plane {z}")
            within(hf.band_strehl[f, z], per_band[:, -1], per_bound[:, -1] + 8 * (n + 40) * EPS * per_band[:, -1], f"band strehl, field {f}")
        within(hf.band_weight[f], g, 8 * (n + 40) * EPS * g, f"band weights, field {f}")
        kappa_mean = np.array([(gr[5].astype(LD) ** 2 * gr[4].astype(LD)).sum() / (gr[5].astype(LD) ** 2).sum() for gr in groups])
        within(hf.cutoff[f], 2 * pupil[f, 3] * kappa_mean, 8 * (n + 40) * EPS * hf.cutoff[f], f"cutoff, field {f}")
        assert np.array_equal(hf.peak[f], hf.intensity[f].max(axis=(1, 2))) and hf.best_focus[f] == DZ[int(np.argmax(hf.strehl[f]))]
        # the transfer function of the field's own image
        for z in range(2):
            J = hf.intensity[f, z] - hf.noise_floor[f]
            want = exact_transfer(hf.intensity[f, z], hf.noise_floor[f], hf.size, hf.t[f], hf.frequencies)
            bound = otf_bound(J, N_PX, hf.size, hf.frequencies)
            within(hf.otf_t[f, z].real, want[0].real, bound, f"Re OTF_t, field {f}")
            within(hf.otf_s[f, z].imag, want[1].imag, bound, f"Im OTF_s, field {f}")
            assert hf.mtf_t[f, z, 0] == 1 and hf.mtf_s[f, z, 0] == 1
        # against huygens_stack of the source with the field's sphere and size
        with ot.global_options.no_warnings():
            st = RT.huygens_stack(f, focus=hf.focus[f], radius=float(hf.radius[f]), n_px=N_PX, size=hf.size, dz=DZ)
        assert np.array_equal(st.band_N, hf.band_N[f]) and np.array_equal(st.focus, hf.focus[f])
        single, _, _, _ = check_records(RT.rays, a, e, hf.section, hf.focus[f], hf.radius[f])
        assert np.array_equal(single[[0, 1, 2, 4, 5]], sl[[0, 1, 2, 4, 5]]), "q, kappa and a: the bits of ot_psf_rays"
        for b in range(K):
            m = live & (kf == b)
            d = sl[3, m].astype(LD) - single[3, m].astype(LD)
            # tau0 = (opl - mean) / lambda with one lambda per band: the two means differ by a constant, and each tau0 carries the
            # rounding of its difference and of its quotient, an eps of itself -- so the intervals d +- bound share a point
            b_d = EPS * (np.abs(sl[3, m]) + np.abs(single[3, m])).astype(LD)
            print(f"field {f} band {b}: tau0 apart by {float(d.mean()):.6e} turns, spread {float(d.max() - d.min()):.3e}")
            assert (d - b_d).max() <= (d + b_d).min(), f"field {f} band {b}: tau0 differs by more than one constant"


def test_sources_in_another_order_permute_the_result(traced):
    RT, hf = traced
    with ot.global_options.no_warnings():
        other = RT.huygens_field(sources=[2, 0, 1], n_px=N_PX, dz=DZ)
    perm = [2, 0, 1]
    assert other.size == hf.size and other.sources.tolist() == perm
    for key in ("field", "t", "focus", "radius", "band_N", "band_power", "band_weight", "cutoff", "intensity", "band_strehl", "strehl",
                "noise_floor", "peak", "best_focus", "otf_t", "otf_s", "mtf_t", "mtf_s"):
        assert np.array_equal(getattr(other, key), getattr(hf, key)[perm]), key


def test_a_source_aimed_past_the_lens_is_the_nan_field(traced):
    """The field without a ray is NaN and leaves the others unchanged, bit for bit: the chunk length follows from the fields that
    hold a record."""
    RT, hf = traced
    with ot.global_options.no_warnings():
        three = RT.huygens_field(sources=[0, 3, 1], n_px=N_PX, dz=DZ, size=hf.size)
        two = RT.huygens_field(sources=[0, 1], n_px=N_PX, dz=DZ, size=hf.size)
    assert three.band_N[1].tolist() == [0, 0] and three.band_power[1].tolist() == [0, 0] and not three.n_missed[1].any()
    for key in ("focus", "radius", "band_weight", "cutoff", "intensity", "band_strehl", "strehl", "noise_floor", "peak", "best_focus",
                "otf_t", "otf_s", "mtf_t", "mtf_s"):
        assert np.all(np.isnan(getattr(three, key)[1])), key
        assert np.array_equal(getattr(three, key)[[0, 2]], getattr(two, key)), key
    for key in ("band_N", "band_power", "n_missed", "n_no_sphere"):
        assert np.array_equal(getattr(three, key)[[0, 2]], getattr(two, key)), key
    assert np.array_equal(three.wavelengths, two.wavelengths) and np.array_equal(three.frequencies, two.frequencies)
    pc.check_empty(three.psf(1), N_PX)
    # alone it is the empty result
    with ot.global_options.no_warnings():
        none = RT.huygens_field(sources=[3], n_px=4, dz=DZ, size=0.1)
    assert none.band_N.tolist() == [[0]] and np.all(np.isnan(none.intensity)) and none.intensity.shape == (1, 2, 4, 4) and none.size == 0.1


def test_grid_goes_to_convolve_field(traced):
    RT, _ = traced
    with ot.global_options.no_warnings():
        hf = RT.huygens_field(sources=[0, 1, 2], n_px=64)
    yy, xx = np.mgrid[0:64, 0:64]
    img = ot.GrayscaleImage(((xx // 8 + yy // 8) % 2).astype(np.float64), s=[2 * hf.size, 2 * hf.size])
    with ot.global_options.no_warnings():
        res = ot.convolve_field(img, hf.grid(), cargs=dict(normalize=False))
        want = ot.convolve_field(img, [[hf.psf(f) for f in range(3)]], cargs=dict(normalize=False))
        column = ot.convolve_field(img, hf.grid(shape=(3, 1)), cargs=dict(normalize=False))
    assert res.shape == want.shape and np.array_equal(res.data, want.data) and np.all(np.isfinite(res.data))
    assert column.shape == res.shape and not np.array_equal(column.data, res.data)


def test_over_the_cap_is_refused_without_an_allocation_of_that_size(traced):
    lib = _capi.load_library()
    rec = to_dev(pc.synthetic_records(65, 3, 50.0), np.float64)
    out = torch.full((16,), -3.0, dtype=torch.float64, device=dev())
    starts = (C.c_int64 * 2049)(*([0] * 2048 + [65]))
    assert _capi.psf_field_ws(65, 64, 32, 1024, 64) + 64 * 64 * 32 * 2 * 1024 * 1024 > _capi.PSF_STACK_CAP
    rc = lib.ot_psf_field_sum(65, ptr(rec), 64, 32, starts, (C.c_double * 64)(*([50.0] * 64)), 1024, 0.1, 64, (C.c_double * 64)(),
                              ptr(out), ptr(out), ptr(out), ptr(out), stream_ptr())
    assert rc == _capi.ERR_UNSUPPORTED and b"ot_psf_field_sum: workspace and field" in lib.ot_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.full(16, -3.0))
    RT, _ = traced
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.max_memory_allocated()
    with pytest.raises(RuntimeError, match="fewer fields, planes, bands or image points"):
        RT.huygens_field(sources=[0, 1, 2], n_px=1024, dz=np.zeros(64))
    assert torch.cuda.max_memory_allocated() - before < 8 * _capi.PSF_STACK_CAP // 64, "nothing near the cap was asked of the device"
