"""Raytracer.huygens_stack, `ot_psf_stack` and `ot_psf_combine` on the GPU.

Truth is `psf_cases.truth` (NumPy longdouble, the definition of DESIGN.md "Huygens PSF") applied to each band's slice of the
grouped records with each plane's dz; the bound it returns is the tolerance, per point and for Re and Im alike, exactly as
tests/test_gpu_psf.py uses it.  Each pass is measured on the inputs it was given: the sum against the grouped records, the combine
step against the device's own field and sums, the whole call against the records and the band assignment the device forms."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd import psf as hp
from optrace_amd._device import ptr, stream_ptr, to_dev
from optrace_amd._warn import OptraceWarning
from optrace_amd.presets import spectral_lines
from optrace_amd.ray_storage import RayStorage

import psf_cases as pc
import wavefront_cases as wc
from test_gpu_psf import call_sum, check_records, mono_tracer
from test_gpu_wavefront import dev, lens_tracer, within

pytestmark = pytest.mark.gpu

EPS, LD = wc.EPS, wc.LD


def call_stack(rec_d, starts, radius, n_px, size, dz):
    """`ot_psf_stack` on the device records rec_d (6 n) -> (field (Z, K, 2, n_px^2), sums (Z, K, 5)) on the host, the device tensors"""
    lib = _capi.load_library()
    n, K, Z = rec_d.shape[0] // 6, len(starts) - 1, len(dz)
    ws = torch.full((_capi.psf_stack_ws(n, K, n_px, Z),), np.nan, dtype=torch.float64, device=dev())
    field = torch.full((Z * K * 2 * n_px * n_px,), np.nan, dtype=torch.float64, device=dev())
    sums = torch.full((Z * K * 5,), np.nan, dtype=torch.float64, device=dev())
    _capi.check(lib.ot_psf_stack(n, ptr(rec_d), K, (C.c_int64 * (K + 1))(*starts), float(radius), n_px, float(size), Z,
                                 (C.c_double * Z)(*dz), ptr(ws), ptr(field), ptr(sums), stream_ptr()))
    return field.cpu().numpy().reshape(Z, K, 2, n_px * n_px), sums.cpu().numpy().reshape(Z, K, 5), field, sums


def call_combine(field_d, sums_d, K, Z, n_px):
    """-> (intensity (Z, n_px^2), band_strehl (Z, K), strehl (Z,), g (K,), noise_floor)"""
    lib = _capi.load_library()
    parts = [Z * n_px * n_px, Z * K, Z, K, 1]
    out = torch.full((sum(parts),), np.nan, dtype=torch.float64, device=dev())
    i, bs, s, g, fl = out.split(parts)
    _capi.check(lib.ot_psf_combine(K, Z, n_px, ptr(field_d), ptr(sums_d), ptr(i), ptr(bs), ptr(s), ptr(g), ptr(fl), stream_ptr()))
    i, bs, s, g, fl = np.split(out.cpu().numpy(), np.cumsum(parts)[:-1])
    return i.reshape(Z, n_px * n_px), bs.reshape(Z, K), s, g, fl[0]


def band_starts(n, K):
    """Starts that leave a band empty, give one a single record and put the boundaries off the multiples of every chunk length met
    here (86 for n = 257, 137 for n = 70001; below 129 records there is one chunk)."""
    if K == 1:
        return [0, n]
    if K == 2:
        return [0, 0, n] if n in (1, 65) else [0, 1, n]  # an empty band and, for n = 1, a single record | a single record
    if K == 3:
        return [0, 12345, 12346, n]
    c1, c2 = (0, 1) if n == 1 else (n // 3 + 2, 2 * n // 3 + 3)
    return [0, c1, c1, min(c1 + 1, n), max(c2, min(c1 + 1, n)), n]  # band 1 empty, band 2 a single record


def check_stack(rec, starts, radius, n_px, size, dz):
    """`ot_psf_stack` on the host records rec (6, n), bands by `starts`, against the truth of every (plane, band)."""
    K, Z = len(starts) - 1, len(dz)
    field, sums, _, _ = call_stack(to_dev(rec, np.float64), starts, radius, n_px, size, dz)
    assert np.all(np.isfinite(field)) and np.all(np.isfinite(sums))
    for b in range(K):
        sl = rec[:, starts[b]:starts[b + 1]]
        nb = sl.shape[1]
        if not nb:
            assert not field[:, b].any() and not sums[:, b].any(), "a band without a record gives zeros"
            continue
        a, kappa = sl[5].astype(LD), sl[4].astype(LD)
        for z in range(Z):
            re, im, bound, A, A2, _ = pc.truth(sl, radius, n_px, size, dz[z])
            within(np.append(field[z, b, 0], sums[z, b, 0]), re, bound, f"Re U, plane {z} band {b}")
            within(np.append(field[z, b, 1], sums[z, b, 1]), im, bound, f"Im U, plane {z} band {b}")
            within(sums[z, b, 2], A, (nb + 40) * EPS * A, "sum a")
            within(sums[z, b, 3], A2, (nb + 40) * EPS * A2, "sum a^2")
            within(sums[z, b, 4], (a * a * kappa).sum(), (nb + 40) * EPS * (a * a * kappa).sum(), "sum a^2 kappa")
    return field, sums


# ---- 1. the hot sum on grouped synthetic records -----------------------------------------------------------------------------------
STACK_CASES = [(n, n_px, K, Z) for n in (1, 63, 65, 257) for n_px in (1, 2, 33, 64) for K, Z in ((1, 1), (2, 3), (5, 2))] + [(70001, 8, 3, 2)]


@pytest.mark.parametrize("n,n_px,K,Z", STACK_CASES)
def test_stack_of_synthetic_records(n, n_px, K, Z):
    """The shapes of `test_gpu_psf.test_sum_of_synthetic_records` with bands and planes: lane, wave, tile and chunk edges, band
    boundaries inside chunks, an empty band and one of a single record, both signs of R."""
    radius = 100.0 if (n + n_px) % 2 else -60.0
    size = 1.0 if n in (63, 257) else 0.02
    rec = pc.synthetic_records(n, 1000 * n + n_px + K, radius)
    check_stack(rec, band_starts(n, K), radius, n_px, size, [0.05, 0.0, -0.03][:Z])


# ---- 2., 3. bits ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,n_px", [(257, 64), (70001, 8), (140001, 4)])
def test_one_band_one_plane_is_ot_psf_sum_bit_for_bit(n, n_px):
    """(257, 64): five tiles; (140001, 4): 1024 chunks of 137 rays aimed at, of which 1022 hold a ray."""
    rec = to_dev(pc.synthetic_records(n, n, -80.0), np.float64)
    field, sums, _, _ = call_stack(rec, [0, n], -80.0, n_px, 0.03, [0.04])
    f1, centre = call_sum(rec, -80.0, n_px, 0.03, 0.04)
    assert np.array_equal(field[0, 0], f1.reshape(2, n_px * n_px)) and np.array_equal(sums[0, 0, :4], centre)


@pytest.mark.parametrize("n,n_px", [(257, 33), (5000, 8)])
def test_planes_do_not_depend_on_each_other(n, n_px):
    """A call for three planes against three calls for one plane each with the same starts, plane by plane, bit for bit; and the
    same call twice.  The chunk length is part of what fixes the bits, and the workgroups aimed at are divided among the planes:
    the two routes share it as long as 128 rays per chunk is what limits the chunks, ceil(n / 128) <= 1024 / (tiles x planes), as
    here (3 chunks of 86, 40 of 125); beyond that the planes of a stack agree with single calls to the truth's bound only."""
    K = 5
    starts, dz = band_starts(n, K), [0.05, 0.0, -0.03]
    assert -(-n // 128) <= 1024 // (3 * -(-(n_px * n_px + 1) // 1024))
    rec = to_dev(pc.synthetic_records(n, 7 * n, 100.0), np.float64)
    field, sums, _, _ = call_stack(rec, starts, 100.0, n_px, 0.02, dz)
    again = call_stack(rec, starts, 100.0, n_px, 0.02, dz)
    assert np.array_equal(field, again[0]) and np.array_equal(sums, again[1]), "two calls, different bits"
    for z in range(3):
        f1, s1, _, _ = call_stack(rec, starts, 100.0, n_px, 0.02, dz[z:z + 1])
        assert np.array_equal(field[z], f1[0]) and np.array_equal(sums[z], s1[0]), f"plane {z}"


# ---- 4. the combine step ------------------------------------------------------------------------------------------------------------------
def combine_by_definition(field, sums, xp=np.float64):
    """DESIGN.md "Polychromatic through-focus PSF" on field (Z, K, 2, px) and sums (Z, K, 5), bands ascending with the device's
    association.  -> (intensity (Z, px), band_strehl (Z, K), strehl (Z,), g (K,), noise_floor)"""
    Z, K = sums.shape[:2]
    field, sums = field.astype(xp), sums.astype(xp)
    inten, bs, s = np.zeros((Z, field.shape[3]), dtype=xp), np.full((Z, K), np.nan, dtype=xp), np.zeros(Z, dtype=xp)
    for z in range(Z):
        A, W, S4 = sums[z, :, 2], sums[z, :, 3], sums[z, :, 4]
        live = [b for b in range(K) if W[b] > 0]
        T = xp(0)
        for b in live:
            kb = S4[b] / W[b]
            T = T + W[b] * (kb * kb)
        g, floor = np.zeros(K, dtype=xp), xp(0)
        for b in live:
            kb = S4[b] / W[b]
            g[b] = W[b] * (kb * kb) / T
            inten[z] = inten[z] + g[b] * ((field[z, b, 0] * field[z, b, 0] + field[z, b, 1] * field[z, b, 1]) / (A[b] * A[b]))
            bs[z, b] = (sums[z, b, 0] * sums[z, b, 0] + sums[z, b, 1] * sums[z, b, 1]) / (A[b] * A[b])
            s[z] = s[z] + g[b] * bs[z, b]
            floor = floor + g[b] * (W[b] / (A[b] * A[b]))
        if z == 0:
            g0, floor0 = g, floor
    return inten, bs, s, g0, floor0


@pytest.mark.parametrize("n,n_px,K,Z", [(257, 33, 5, 2), (65, 2, 2, 3), (63, 1, 1, 1)])
def test_combine_against_the_definition(n, n_px, K, Z):
    """`ot_psf_combine` against the formulas in float64 NumPy on the device's own field and sums.  Every figure is a sum of K positive
    terms; a term passes through 10 roundings at the most (kappa_mean, its square, W kappa^2, the quotient g; two squares and a
    sum, A^2, the quotient; g times it), the sum T of the weights through K and the sum of the terms through K more: (10 + 2 K)
    eps relative.  (With IEEE division and no contraction on both sides the two agree bit for bit; the test does not ask for it.)"""
    rec = pc.synthetic_records(n, 31 * n, 100.0)
    starts = band_starts(n, K)
    field, sums, field_d, sums_d = call_stack(to_dev(rec, np.float64), starts, 100.0, n_px, 0.02, [0.0, 0.04, -0.02][:Z])
    inten, bs, s, g, floor = call_combine(field_d, sums_d, K, Z, n_px)
    w_i, w_bs, w_s, w_g, w_floor = combine_by_definition(field, sums)
    tol = (10 + 2 * K) * EPS
    print("bit for bit:", np.array_equal(inten, w_i), np.array_equal(s, w_s), np.array_equal(g, w_g), floor == w_floor)
    within(inten, w_i, tol * w_i, "intensity")
    within(s, w_s, tol * w_s, "strehl")
    within(g, w_g, tol * w_g, "g")
    within(floor, w_floor, tol * w_floor, "noise floor")
    empty = sums[0, :, 3] == 0  # (no record, or dead records alone)
    assert empty[np.diff(starts) == 0].all()
    assert np.all(np.isnan(bs[:, empty])) and np.all(g[empty] == 0)
    within(bs[:, ~empty], w_bs[:, ~empty], tol * w_bs[:, ~empty], "band strehl")
    assert g.sum() == pytest.approx(1, abs=K * EPS)
    # strehl is sum g_b band_strehl, formed the same way
    for z in range(Z):
        t = 0.0
        for b in np.nonzero(~empty)[0]:
            t = t + g[b] * bs[z, b]
        assert s[z] == t


# ---- 5. end to end: a singlet with colour ----------------------------------------------------------------------------------------------
F_LINE, C_LINE = spectral_lines.F, spectral_lines.C


def singlet(spectrum=None):
    """A biconvex singlet of R = +-50 mm and n_d = 1.5, V = 30 (f = 50 mm at d), lit along the axis by a collimated bundle of
    radius 1 mm -- a point far on the axis behind an aperture of 1 mm --: NA 0.02."""
    RT = ot.Raytracer(outline=[-3, 3, -3, 3, -1, 70], no_pol=True, seed=5)
    spectrum = spectrum or ot.LightSpectrum("Lines", lines=[F_LINE, C_LINE], line_vals=[1, 1])
    RT.add(ot.RaySource(ot.CircularSurface(r=1), divergence="None", spectrum=spectrum, pos=[0, 0, 0]))
    RT.add(ot.Lens(ot.SphericalSurface(r=2, R=50), ot.SphericalSurface(r=2, R=-50), n=ot.RefractionIndex("Abbe", n=1.5, V=30),
                   pos=[0, 0, 5], d=0.4))
    return RT


def stack_truth(rec_g, starts, radius, n_px, size, dz, points):
    """The definition in longdouble on grouped host records at the points `points` of plane dz.
    -> (value, bound) per point: sum_b g_b |U_b|^2 / A_b^2 and, per band, |d |U|^2| <= 2 (|Re| + |Im|) beta + 2 beta^2 carried through
    the same sum, plus 8 (n + 40) eps of the value for A, W and the weights; and the per-band values."""
    K, n = len(starts) - 1, rec_g.shape[1]
    t, per_band, per_bound = np.zeros(K, dtype=LD), [], []
    for b in range(K):
        sl = rec_g[:, starts[b]:starts[b + 1]]
        a, kappa = sl[5].astype(LD), sl[4].astype(LD)
        W = (a * a).sum()
        t[b] = W * ((a * a * kappa).sum() / W) ** 2
        re, im, beta, A, _, _ = pc.truth(sl, radius, n_px, size, dz, points=points)
        per_band.append((re * re + im * im) / (A * A))
        per_bound.append((2 * (np.abs(re) + np.abs(im)) * beta + 2 * beta * beta) / (A * A))
    g = t / t.sum()
    value = sum(g[b] * per_band[b] for b in range(K))
    bound = sum(g[b] * per_bound[b] for b in range(K)) + 8 * (n + 40) * EPS * value
    return value, bound, np.array(per_band), np.array(per_bound), g


def test_singlet_with_two_lines_through_focus():
    """20 000 rays of the F and C lines, 31 planes across +-1.5 mm about the default focus, 16 x 16 points.  The axis point (strehl,
    band_strehl) is held to the longdouble definition on every plane; the image on the middle plane at every point, and on every
    plane at eight points of the diagonal, which keeps the truth to about 1e7 longdouble ray-points.  Then the colour: the F band
    focuses before the C band, as far apart as the paraxial images of the two lines."""
    RT = singlet()
    with ot.global_options.no_warnings():
        RT.trace(20000)
    dz = np.linspace(-1.5, 1.5, 31)
    n_px = 16
    with warnings.catch_warnings():
        warnings.simplefilter("error", category=OptraceWarning)  # (huygens_stack never gives the monochromatic warning)
        st = RT.huygens_stack(0, n_px=n_px, dz=dz)
        again = RT.huygens_stack(0, n_px=n_px, dz=dz)
    assert isinstance(st, ot.HuygensStack) and st.N == 20000 and st.n_missed == 0 and st.n_out_of_band == 0 and st.section == 2
    assert np.array_equal(st.intensity, again.intensity) and np.array_equal(st.band_strehl, again.band_strehl)
    assert st.band_edges is None and np.array_equal(st.band_wavelength, np.float32([F_LINE, C_LINE]).astype(np.float64))
    assert st.band_N.sum() == st.N and np.all(st.band_N > 9000) and st.band_power.sum() == pytest.approx(st.power, rel=1e-12)
    assert st.intensity.shape == (31, 16, 16) and st.strehl.shape == (31,) and st.band_strehl.shape == (31, 2)
    assert st.band_weight.sum() == pytest.approx(1, abs=1e-15) and st.band_weight[0] > st.band_weight[1], "(n / lambda)^2 favours F"

    # the device's own records and band assignment
    rays = RT.rays
    rec, rec_d, _, mom = check_records(rays, 0, 20000, st.section, st.focus, st.radius)
    assert st.size == hp.default_size(mom)
    key, K, table = hp.assign_bands(rays._dev["wl"][:20000], rec_d[5 * 20000:] != 0, "lines")
    grouped, starts, table, order = hp.group_records(rec_d, 20000, key, K, table)
    K, starts, _ = hp.settle_bands("lines", K, starts, table)
    assert K == 2 and np.array_equal(np.diff(starts), st.band_N)
    rec_g = grouped.cpu().numpy().reshape(6, 20000)
    assert np.array_equal(rec_g, rec[:, order.cpu().numpy()]) and np.all(np.diff(order.cpu().numpy()[:starts[1]]) > 0)
    axis = n_px * n_px
    diag = np.arange(0, n_px, 2) * (n_px + 1)
    for z in range(31):
        pts = np.append(np.arange(axis) if z == 15 else diag, axis)
        value, bound, per_band, per_bound, g = stack_truth(rec_g, starts, st.radius, n_px, st.size, dz[z], pts)
        within(st.intensity[z].ravel()[pts[:-1]], value[:-1], bound[:-1], f"intensity, plane {z}")
        within(st.strehl[z], value[-1], bound[-1], f"strehl, plane {z}")
        within(st.band_strehl[z], per_band[:, -1], per_bound[:, -1] + 8 * (20000 + 40) * EPS * per_band[:, -1], f"band strehl, plane {z}")
    within(st.band_weight, g, 8 * (20000 + 40) * EPS * g, "band weights")
    assert np.array_equal(st.peak, st.intensity.max(axis=(1, 2))) and st.best_focus == dz[np.argmax(st.strehl)]

    # colour: F focuses first; the distance of the best planes is that of the paraxial images, to two plane spacings
    zF, zC = dz[np.argmax(st.band_strehl[:, 0])], dz[np.argmax(st.band_strehl[:, 1])]
    parax = RT.tma(C_LINE).image_position(-np.inf) - RT.tma(F_LINE).image_position(-np.inf)
    print(f"best planes: F {zF:+.3f} mm, C {zC:+.3f} mm, apart {zC - zF:.3f} mm; paraxial images apart {parax:.4f} mm; "
          f"band strehl there {st.band_strehl[:, 0].max():.4f}, {st.band_strehl[:, 1].max():.4f}; strehl {st.strehl.max():.4f} at {st.best_focus:+.2f}")
    assert zF < zC and -1.5 < zF and zC < 1.5
    assert abs((zC - zF) - parax) <= 2 * (dz[1] - dz[0])


# ---- 6. one wavelength, and the warnings ----------------------------------------------------------------------------------------------------
def test_monochromatic_stack_is_huygens_psf_plane_by_plane(monkeypatch):
    """`huygens_stack(dz=[0, d])` against `huygens_psf(dz=0)` and `huygens_psf(dz=d)`: each route lies within its bound of the
    definition on the device's records (the bound of `test_gpu_psf.check_against_own_records`), so the two differ by the sum."""
    monkeypatch.setattr(ot.global_options, "show_warnings", True)
    RT = mono_tracer()
    with ot.global_options.no_warnings():
        RT.trace(20000)
    d, n_px, n = 0.03, 8, 20000
    with warnings.catch_warnings():
        warnings.simplefilter("error", category=OptraceWarning)
        st = RT.huygens_stack(0, n_px=n_px, dz=[0.0, d])
        singles = [RT.huygens_psf(0, n_px=n_px, dz=0.0), RT.huygens_psf(0, n_px=n_px, dz=d)]
        by_count = RT.huygens_stack(0, n_px=n_px, dz=[0.0, d], bands=4)  # (one wavelength: one band, whatever the count)
    assert st.band_N.tolist() == [n] and st.band_weight.tolist() == [1] and st.band_wavelength[0] == pytest.approx(550, rel=1e-6)
    assert by_count.band_N.tolist() == [n] and by_count.band_edges.shape == (2,) and by_count.band_edges[0] == by_count.band_edges[1]
    assert np.array_equal(by_count.intensity, st.intensity)
    rec, _, _, _ = check_records(RT.rays, 0, n, st.section, st.focus, st.radius)
    for z, one in enumerate(singles):
        assert np.array_equal(one.focus, st.focus) and one.radius == st.radius and one.size == st.size and one.N == st.N
        re, im, bound, A, A2, _ = pc.truth(rec, st.radius, n_px, st.size, st.dz[z])
        I = (re * re + im * im) / (A * A)
        b_I = (2 * np.sqrt(LD(2)) * np.sqrt(re * re + im * im) * bound + 2 * bound * bound) / (A * A) + (4 * (n + 40) + 8) * EPS * I
        within(st.intensity[z].ravel(), one.intensity.ravel(), 2 * b_I[:-1], f"plane {z}, the two routes")
        within(st.strehl[z], one.strehl, 2 * b_I[-1], f"strehl of plane {z}, the two routes")
        within(st.intensity[z].ravel(), I[:-1], b_I[:-1], f"plane {z} against the definition")
        assert st.noise_floor == pytest.approx(one.noise_floor, rel=1e-12) and st.psf(z).peak == st.peak[z]


def test_two_lines_warn_in_huygens_psf_alone(monkeypatch):
    monkeypatch.setattr(ot.global_options, "show_warnings", True)
    RT = singlet()
    with ot.global_options.no_warnings():
        RT.trace(3000)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        RT.huygens_psf(0, n_px=4)
    mine = [x for x in seen if issubclass(x.category, OptraceWarning)]
    assert len(mine) == 1 and "monochromatic" in str(mine[0].message)
    with warnings.catch_warnings():
        warnings.simplefilter("error", category=OptraceWarning)
        st = RT.huygens_stack(0, n_px=4)
    assert st.band_N.sum() == 3000 and st.dz.tolist() == [0]


# ---- 7. bands by count and by edges, storage edges, refusals ------------------------------------------------------------------------------
def test_bands_by_count_and_by_edges():
    """The source of `lens_tracer`: lines at 486 and 656 nm, weights 1 : 2."""
    RT = lens_tracer()
    with ot.global_options.no_warnings():
        RT.trace(6000)
        lines = RT.huygens_stack(0, n_px=4)
        two = RT.huygens_stack(0, n_px=4, bands=2)
        four = RT.huygens_stack(0, n_px=4, bands=4, focus=lines.focus, radius=lines.radius, size=lines.size)
        blue = RT.huygens_stack(0, n_px=4, bands=[400.0, 486.0, 600.0], dz=[0.0, 0.01])
        edge = RT.huygens_stack(0, n_px=4, bands=[400.0, 486.0])  # (the last band is closed above)
        none = RT.huygens_stack(0, n_px=4, bands=[700.0, 800.0], dz=[0.0, 0.1, 0.2])
    nF, nC = lines.band_N
    assert lines.band_wavelength.tolist() == [486, 656] and nF + nC == 6000 and 1500 < nF < 2500
    assert two.band_edges.tolist() == [486, 571, 656] and two.band_N.tolist() == [nF, nC] and two.n_out_of_band == 0
    assert np.array_equal(two.intensity, lines.intensity) and np.array_equal(two.band_strehl, lines.band_strehl)
    assert two.band_wavelength == pytest.approx([486, 656], rel=1e-12)
    assert four.band_N.tolist() == [nF, 0, 0, nC] and np.all(np.isnan(four.band_strehl[:, 1:3])) and four.band_weight[1:3].tolist() == [0, 0]
    assert np.array_equal(four.band_strehl[:, [0, 3]], lines.band_strehl) and np.array_equal(four.strehl, lines.strehl)
    assert np.all(np.isnan(four.band_wavelength[1:3])) and four.band_power[1:3].tolist() == [0, 0]
    assert blue.band_N.tolist() == [0, nF] and blue.N == nF and blue.n_out_of_band == nC and blue.band_weight.tolist() == [0, 1]
    assert np.array_equal(blue.strehl, blue.band_strehl[:, 1]) and blue.wavelength == pytest.approx(486, rel=1e-12)
    assert edge.band_N.tolist() == [nF] and edge.n_out_of_band == nC
    # every used ray out of band: the empty result, which keeps what the call fixed and counts what it left out
    assert none.N == 0 and none.power == 0 and none.n_out_of_band == 6000 and none.intensity.shape == (3, 4, 4) and np.all(np.isnan(none.intensity))
    assert np.all(np.isnan(none.strehl)) and np.isnan(none.best_focus) and none.band_edges.tolist() == [700, 800] and none.band_N.tolist() == [0]
    assert np.array_equal(none.focus, lines.focus) and none.radius == lines.radius


def test_all_absorbed_bundle_gives_the_empty_result():
    RT = lens_tracer(aim_at_aperture=True)
    with ot.global_options.no_warnings():
        RT.trace(1000)
        st = RT.huygens_stack(0, n_px=6, dz=[0.0, 0.1])
    assert st.N == 0 and st.n_out_of_band == 0 and st.intensity.shape == (2, 6, 6) and np.all(np.isnan(st.intensity)) and np.isnan(st.size)
    pc.check_empty(st.psf(1), 6)


def test_padded_storage_and_stale_index_plane(monkeypatch):
    """A generated trace of 4099 rays in planes 4224 apart, its index plane still unwritten when the stack is asked for."""
    monkeypatch.setattr(RayStorage, "PAD_FROM", 512)
    RT = lens_tracer()
    with ot.global_options.no_warnings():
        RT.trace(4099)
        assert RT.rays._Np == 4224 and RT.rays._n_stale, "nothing here may have read the plane through the hook"
        st = RT.huygens_stack(0, n_px=8, dz=[0.0, 0.02])
    assert not RT.rays._n_stale and st.N == 4099 and st.band_N.sum() == 4099 and st.band_wavelength.tolist() == [486, 656]
    rec, rec_d, _, _ = check_records(RT.rays, 0, 4099, 2, st.focus, st.radius)
    assert np.array_equal(np.unique(np.round(rec[4])), [1524, 2058]), "kappa = 1 / lambda of the two lines, in air"
    key, K, table = hp.assign_bands(RT.rays._dev["wl"][:4099], rec_d[5 * 4099:] != 0, "lines")
    grouped, starts, table, _ = hp.group_records(rec_d, 4099, key, K, table)
    K, starts, _ = hp.settle_bands("lines", K, starts, table)
    rec_g = grouped.cpu().numpy().reshape(6, 4099)
    for z in range(2):
        value, bound, per_band, per_bound, g = stack_truth(rec_g, starts, st.radius, 8, st.size, st.dz[z], np.arange(65))
        within(st.intensity[z].ravel(), value[:-1], bound[:-1], f"intensity, plane {z}")
        within(st.strehl[z], value[-1], bound[-1], f"strehl, plane {z}")


def test_over_the_cap_is_refused_without_a_launch():
    lib = _capi.load_library()
    rec = to_dev(pc.synthetic_records(65, 3, 50.0), np.float64)
    out = torch.full((16,), -3.0, dtype=torch.float64, device=dev())
    starts = (C.c_int64 * 33)(*([0] * 32 + [65]))
    dz = (C.c_double * 64)()
    assert _capi.psf_stack_ws(65, 32, 1024, 64) + 64 * 32 * 2 * 1024 * 1024 > _capi.PSF_STACK_CAP
    rc = lib.ot_psf_stack(65, ptr(rec), 32, starts, 50.0, 1024, 0.1, 64, dz, ptr(out), ptr(out), ptr(out), stream_ptr())
    assert rc == _capi.ERR_UNSUPPORTED and b"ot_psf_stack: workspace and field" in lib.ot_last_error()
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.full(16, -3.0))
    RT = mono_tracer()
    with ot.global_options.no_warnings():
        RT.trace(1000)
    with pytest.raises(RuntimeError, match="fewer planes, bands or image points"):
        RT.huygens_stack(0, n_px=1024, dz=np.zeros(64), bands=32)
