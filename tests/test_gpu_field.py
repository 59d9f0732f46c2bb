"""Raytracer.field_analysis and the `ot_field_*` entry points on the GPU.

Truth is NumPy longdouble following the definition (tests/field_cases.py): on synthetic storages handed to the entry points through
ctypes, and on the device's own ray storage read back for traced scenes.

Bounds, as stated with the feature: the ray counts (slots 1 and 7) equal the truth; every sum is within (n + 40) eps sum |terms|
(`chromatic_cases.sum_bound`), n the cell's ray count, the second-pass sums about the means the device forms from its own record,
which are an input of that pass; two calls return the same bits; a field's records do not depend on the other fields of the call;
slots 0, 1 and 6 added over the fields are slots 0, 1 and 4 of `ot_chromatic_plane` on the same rays, each side within its bound."""
import ctypes as C
import functools

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

pytestmark = pytest.mark.gpu

EPS, LD, M, NONE = fc.EPS, fc.LD, fc.M, fc.NO_BAND
CAP = 1024  # OT_FIELD_BLOCKS: most workgroups of 256 per field
F64 = lambda a: np.asarray(a).astype(np.float64)


def dev():
    return torch.device("cuda", torch.cuda.current_device())


# ---- synthetic storages ----------------------------------------------------------------------------------------------------------
class Storage:
    """Host arrays p (N, nt, 3), w (N, nt), wl (N,) in the layout of the reference and their planes on the device behind an `ot_rays`."""

    def __init__(self, p, w, wl):
        self.p, self.w, self.wl = p, w, wl
        self.N, self.nt = w.shape
        self.d_p = to_dev(np.ascontiguousarray(p.transpose(2, 1, 0)), np.float64)  # r + N * (i + nt * c)
        self.d_w = to_dev(np.ascontiguousarray(w.T), np.float32)
        self.d_wl = to_dev(wl, np.float32)
        self.rays = _capi.Rays()
        self.rays.N, self.rays.nt = self.N, self.nt
        self.rays.p, self.rays.w, self.rays.wl = self.d_p.data_ptr(), self.d_w.data_ptr(), self.d_wl.data_ptr()


FAR_END = [-1e30, -2e30, -3e30]  # (from 1e30 in all three: a section of some length that crosses a plane z = const far away)


def build(counts, nt, k, first, K, seed, gaps=None, behind=37, keys=None, far=True):
    """-> (Storage, fields [(first, count), ...], key, key_first).  Field f owns `counts[f]` rays, `gaps[f]` rays after it belong to
    no field.  Random planes: four rays in five live in section k, the dead ones hold NaN positions and weight 0; of the living,
    some have a section of no length (not used) and some run within a plane z = const (used, d_z == 0).  Keys are drawn from
    0 .. K - 1 and 255 unless `keys` gives them.  far: in every field of 8 rays or more one living ray in no band, and in the last
    such field one of band K - 1, lies 1e30 away with a weight of 1e30: a leak between bands or fields shows.  The rays outside the
    fields -- `first` in front, the gaps, `behind` after the last -- hold used rays of 1e30 with the key 0, every other one of a gap
    NaN positions and a weight of 1: a read beyond a field's range would bring them in.  key_first lies 3 before the first field."""
    rng = np.random.default_rng(seed)
    gaps = [0] * len(counts) if gaps is None else gaps
    N = first + sum(counts) + sum(gaps) + behind
    p = np.full((N, nt, 3), 1e30)
    p[:, 1::2] = FAR_END  # (outside the fields every section has a length)
    w = np.full((N, nt), 1e30, dtype=np.float32)
    wl = np.full(N, 1e30, dtype=np.float32)
    key_first = max(first - 3, 0)
    key = np.zeros(N - key_first, dtype=np.uint8)
    fields, at, big = [], first, [f for f, n in enumerate(counts) if n >= 8]
    for f, (count, gap) in enumerate(zip(counts, gaps)):
        fields.append((at, count))
        alive = rng.uniform(size=count) < 0.8
        q = rng.normal(size=(count, nt, 3)) * [3.0, 2.0, 1.0] + [0.5 + 0.1 * f, -0.25, 10.0]
        kind = rng.uniform(size=count)
        q[kind < 0.03, k + 1] = q[kind < 0.03, k]          # no length: not used
        flat = (kind >= 0.03) & (kind < 0.08)
        q[flat, k + 1, 2] = q[flat, k, 2]                  # d_z == 0
        q[~alive] = np.nan
        wr = np.where(alive[:, None], rng.uniform(0.1, 1.0, size=(count, nt)), 0.0)
        kf = rng.choice(np.arange(K + 1), size=count) if keys is None else np.array(keys[f])
        kf = np.where(kf >= K, NONE, kf).astype(np.uint8)
        if far and count >= 8:
            spots = [count // 3] + ([2 * count // 3] if K > 1 and f == big[-1] else [])
            q[spots], wr[spots] = 1e30, 1e30
            q[spots, k + 1] = FAR_END
            kf[spots[0]] = NONE
            if len(spots) > 1:
                kf[spots[1]] = K - 1
        p[at:at + count], w[at:at + count] = q, wr.astype(np.float32)
        wl[at:at + count] = rng.uniform(400, 700, size=count).astype(np.float32)
        key[at - key_first:at - key_first + count] = kf
        p[at + count:at + count + gap:2] = np.nan
        w[at + count:at + count + gap:2] = 1.0
        at += count + gap
    return Storage(p, w, wl), fields, key, key_first


def flat_ranges(fields):
    return (C.c_int64 * (2 * len(fields)))(*[int(v) for pair in fields for v in pair])


def call_sums(S, fields, k, key, key_first, K, origin):
    lib = _capi.load_library()
    F = len(fields)
    n_ws = lib.ot_field_workspace(flat_ranges(fields), F, K)
    longest = max(1, max(min(-(-n // 256), CAP) for _, n in fields))
    assert n_ws == K * (F * longest * 10 + F * M)
    ws = torch.full((n_ws,), np.nan, dtype=torch.float64, device=dev())  # (a partial read before it is written shows)
    rec = torch.full((F * K * M,), -7.0, dtype=torch.float64, device=dev())
    d_key = to_dev(key, np.uint8)
    _capi.check(lib.ot_field_sums(C.byref(S.rays), flat_ranges(fields), F, k, ptr(d_key), key_first, K, (C.c_double * 3)(*origin),
                                  ptr(ws), ptr(rec), stream_ptr()))
    return rec.cpu().numpy().reshape(F, K, M)


def call_plane(S, first, count, k, key, K, z0):
    lib = _capi.load_library()
    ws = torch.full((lib.ot_chromatic_workspace(count, K),), np.nan, dtype=torch.float64, device=dev())
    rec = torch.full((K * cc.M,), -7.0, dtype=torch.float64, device=dev())
    d_key = to_dev(key, np.uint8)
    _capi.check(lib.ot_chromatic_plane(C.byref(S.rays), first, count, k, ptr(d_key), K, z0, ptr(ws), ptr(rec), stream_ptr()))
    return rec.cpu().numpy().reshape(K, cc.M)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a).view(np.uint64), np.ascontiguousarray(b).view(np.uint64))


def check_entry_point(S, fields, k, key, key_first, K, what, origin=(0.25, -0.5, 9.5), alone=True):
    """-> records of the device, checked against the oracle; twice the same bits; every field alone gives the bits it has among
    the others."""
    rec = call_sums(S, fields, k, key, key_first, K, origin)
    assert same_bits(rec, call_sums(S, fields, k, key, key_first, K, origin)), f"{what}: two calls, different bits"
    val, mag = fc.records(S.p, S.w, S.wl, fields, k, key, key_first, K, origin, means=fc.record_means(rec))
    fc.check_records(rec, val, mag, what)
    if alone and len(fields) > 1:
        for f, one in enumerate(fields):
            if one[1]:
                assert same_bits(rec[f], call_sums(S, [one], k, key, key_first, K, origin)[0]), f"{what}: field {f} alone differs"
    return rec


@pytest.mark.parametrize("counts,gaps,nt,k,first,K", [
    ([1], None, 2, 0, 5, 1), ([63, 64], None, 5, 3, 5, 3), ([65, 255, 256], [0, 7, 0], 2, 0, 33, 32),  # around a wave and a workgroup
    ([257, 0, 3000], [5, 0, 11], 5, 3, 7, 3),                   # a field of no rays between two, gaps of rays of no field
    ([3000, 1, 64], [1, 1, 1], 5, 0, 3, 32),                    # a field of one ray
    ([256 * CAP + 1, 65], [3, 0], 2, 0, 7, 3),                  # one ray more than a field's launch has lanes
    ([3000], None, 5, 3, 64, 1),
])
def test_entry_point_on_random_planes(counts, gaps, nt, k, first, K):
    seed = sum(counts) + 7 * nt + K
    S, fields, key, key_first = build(counts, nt, k, first, K, seed, gaps=gaps)
    check_entry_point(S, fields, k, key, key_first, K, f"fields of {counts} rays, nt {nt}, section {k}, {K} bands")


def test_sixty_four_fields_and_the_last_ends_with_the_storage():
    counts = [(37 * f) % 131 + (f % 3 == 0) for f in range(64)]
    assert 0 in counts or min(counts) <= 1
    S, fields, key, key_first = build(counts, 4, 2, 13, 3, 8, gaps=[(f + 1) % 2 for f in range(64)], behind=0)
    assert fields[-1][0] + fields[-1][1] == S.N and any(a % 16 for a, _ in fields)
    rec = check_entry_point(S, fields, 2, key, key_first, 3, "64 fields", alone=False)
    # three of the fields alone: the bits they have among the 64
    for f in (1, 17, 63):
        assert same_bits(rec[f], call_sums(S, [fields[f]], 2, key, key_first, 3, (0.25, -0.5, 9.5))[0])


def test_waves_of_one_band_and_of_all_bands_and_bands_without_a_ray():
    """Two fields of 640 rays, 32 bands: the first wave of field 0 holds rays of band 5 alone, its second wave all 32 bands, two
    rays each; the rest of field 0 lies in band 1.  Field 1: every ray in band 30."""
    count, K = 640, 32
    k0 = np.ones(count, dtype=np.int64)
    k0[:64], k0[64:128] = 5, np.arange(64) % 32
    S, fields, key, key_first = build([count, count], 3, 1, 11, K, 21, keys=[k0, np.full(count, 30)], far=False)
    # (the two waves alive, of some length and not in a plane, whatever was drawn)
    rng = np.random.default_rng(3)
    r = np.arange(11, 11 + 128)
    S.p[r] = rng.normal(size=(128, 3, 3)) + [0, 0, 10]
    S.p[r, 2, 2] += 5
    S.w[r] = 0.5
    S = Storage(S.p, S.w, S.wl)
    rec = check_entry_point(S, fields, 1, key, key_first, K, "special waves")
    n = rec[0, :, 1]
    assert n[5] == 66 and n[1] > 300 and np.all(n[[0, 2, 3, 4] + list(range(6, 32))] == 2)
    assert np.all(rec[1, :30, :8] == 0) and np.all(rec[1, 31, :8] == 0) and rec[1, 30, 1] > 400 and rec[1, 30, 7] > 5
    assert np.all(np.isnan(rec[1, :30, 8:]))


def test_fields_add_up_to_the_chromatic_plane():
    """Three adjacent fields: slots 0, 1 and 6 added over the fields against slots 0, 1 and 4 of `ot_chromatic_plane` on the whole range."""
    counts, K, k = [700, 300, 1000], 3, 1
    S, fields, key, key_first = build(counts, 3, k, 16, K, 5, far=False)
    rec = check_entry_point(S, fields, k, key, key_first, K, "three adjacent fields")
    first, count = fields[0][0], sum(counts)
    whole = call_plane(S, first, count, k, key[first - key_first:first - key_first + count], K, 9.0)
    val, mag = fc.records(S.p, S.w, S.wl, fields, k, key, key_first, K, (0.25, -0.5, 9.5))
    cval, cmag = cc.records(S.p, S.w, S.wl, first, count, k, key[first - key_first:first - key_first + count], K, 9.0)
    assert np.array_equal(rec[:, :, 1].sum(axis=0), whole[:, 1]) and np.array_equal(rec[:, :, 7].sum(axis=0), whole[:, 9])
    for mine, theirs in ((0, 0), (6, 4)):
        bound = cc.sum_bound(F64(val[:, :, 1]), F64(mag[:, :, mine])).sum(axis=0) + cc.sum_bound(F64(cval[:, 1]), F64(cmag[:, theirs]))
        apart = np.abs(rec[:, :, mine].astype(LD).sum(axis=0) - whole[:, theirs].astype(LD)).astype(np.float64)
        assert np.all(apart <= bound), f"slot {mine}: {apart} above {bound}"


def test_no_ray_in_any_field_launches_nothing():
    S, fields, key, key_first = build([10], 3, 0, 0, 2, 2)
    lib = _capi.load_library()
    rec = torch.full((2 * 2 * M,), -7.0, dtype=torch.float64, device=dev())
    ws = torch.zeros(256, dtype=torch.float64, device=dev())
    d_key = to_dev(key, np.uint8)
    _capi.check(lib.ot_field_sums(C.byref(S.rays), flat_ranges([(10, 0), (3, 0)]), 2, 0, ptr(d_key), 0, 2, (C.c_double * 3)(0, 0, 0),
                                  ptr(ws), ptr(rec), stream_ptr()))
    assert np.all(rec.cpu().numpy() == -7.0) and np.all(ws.cpu().numpy() == 0)


# ---- Raytracer.field_analysis on traced rays -----------------------------------------------------------------------------------------
def ideal_scene():
    """An ideal lens of f = 15 mm images three point sources at z = -30, heights 0, 1 and 2 mm, one to one onto z = 30."""
    RT = ot.Raytracer(outline=[-10, 10, -10, 10, -40, 60])
    for h in (0.0, 1.0, 2.0):
        RT.add(ot.RaySource(ot.Point(), divergence="Isotropic", div_angle=3, pos=[0, h, -30], s=[0, 0, 1],
                            spectrum=ot.LightSpectrum("Monochromatic", wl=550.)))
    RT.add(ot.IdealLens(r=5, D=1000 / 15, pos=[0, 0, 0]))
    RT.add(ot.Detector(ot.RectangularSurface(dim=[8, 8]), pos=[0, 0, 30]))
    return RT


def test_an_ideal_lens_images_every_field_point_where_the_paraxial_analysis_says():
    with ot.global_options.no_warnings():
        RT = ideal_scene()
        RT.trace(6000)
    image_z = RT.tma(550.0).image_position(-30.0)
    assert image_z == pytest.approx(30.0, rel=1e-12)
    fa = RT.field_analysis()
    assert fa.n_fields == 3 and fa.n_bands == 1 and fa.sources.tolist() == [0, 1, 2] and np.all(fa.band_N[:, 0] == 2000)
    rel = lambda got, want: np.max(np.abs(got - want)) / np.max(np.abs(want))
    print(f"foci t {fa.focus_t[:, 0]}, s {fa.focus_s[:, 0]}, z {fa.z}, centroid {fa.centroid[:, 0]}, paraxial {fa.paraxial[:, 0]}, "
          f"distortion {fa.distortion[:, 0]}")
    assert rel(fa.focus_t[:, 0], image_z) <= 1e-9 and rel(fa.focus_s[:, 0], image_z) <= 1e-9 and rel(fa.focus_rms[:, 0], image_z) <= 1e-9
    assert abs(fa.z - image_z) <= 1e-9 * image_z
    assert np.allclose(fa.paraxial[:, 0], [[0, 0], [0, -1], [0, -2]], rtol=0, atol=1e-12)
    assert np.all(np.abs(fa.centroid[:, 0] - fa.paraxial[:, 0]) <= 1e-9 * 2.0)
    assert np.isnan(fa.distortion[0, 0]) and np.all(np.abs(fa.distortion[1:, 0]) <= 1e-9)
    assert np.allclose(fa.field, [[0, 0], [0, 1], [0, 2]]) and np.allclose(fa.t, [[0, 1]] * 3)
    # (the smallest spot is what is left of the quadratic A + 2 zeta C + zeta^2 V where its terms cancel: rounding of the spot at the
    # origin's plane, 1.6 mm wide on the lens, squared: sqrt(64 eps) of that width allowed)
    assert np.all(fa.rms_radius_best[:, 0] < np.sqrt(64 * EPS) * 1.6) and np.all(np.abs(fa.astigmatism[:, 0]) <= 2e-9 * image_z)
    assert fa.relative_illumination.tolist() == [1, 1, 1] and "RS0, RS1, RS2" in fa.long_desc
    # no paraxial analysis asked for: NaN, and nothing else changes
    fb = RT.field_analysis(paraxial=None)
    assert np.all(np.isnan(fb.paraxial)) and np.all(np.isnan(fb.distortion)) and same_bits(fa.records, fb.records)


@functools.lru_cache(maxsize=None)
def double_gauss():
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=7)
        RT.trace(20000)
    return RT


def quotient_tolerance(C_val, V_val, dC, dV):
    """How far -C / V from sums within their bounds dC, dV may lie from that of the true sums: to first order
    dC / |V| + |C| dV / V^2, doubled for the higher orders, plus 4 eps for the quotient and the difference from the origin."""
    return 2 * (dC / abs(V_val) + abs(C_val) * dV / V_val ** 2)


def check_analysis(RT, fa, sources, section, bands, what):
    """The records and the foci of `fa` against the truth formed from the storage read back."""
    p, w, wl = RT.rays.p_list, RT.rays.w_list, RT.rays.wl_list
    nt = w.shape[1]
    k = nt - 2 if section is None else section
    fields = [(int(RT.rays.B_list[s]), int(RT.rays.B_list[s + 1] - RT.rays.B_list[s])) for s in sources]
    origin = np.array(SectionTable(RT).origin(k, None), dtype=np.float64)
    # the bands: over the used rays of all chosen fields together
    used = np.zeros(w.shape[0], dtype=bool)
    for first, count in fields:
        used[first:first + count] = cc.used_rays(p, w, first, count, k)[0]
    key, K, edges = cc.band_keys(wl, used, bands)
    assert fa.n_bands == K and fa.section == k and fa.n_fields == len(sources) and fa.sources.tolist() == list(sources)
    assert np.array_equal(fa.origin, origin) and (fa.band_edges is None if edges is None else np.array_equal(fa.band_edges, edges))
    rec = fa.records
    val, mag = fc.records(p, w, wl, fields, k, key, 0, K, origin, means=fc.record_means(rec))
    fc.check_records(rec, val, mag, what)
    S = Storage(p, w, wl)
    assert same_bits(rec, call_sums(S, fields, k, key.astype(np.uint8), 0, K, origin)), f"{what}: the records are the entry point's"
    # the foci against those of the true sums, within the first-order bound of their quotients
    v, b = F64(val), cc.sum_bound(F64(val[:, :, 1:2]), F64(mag))
    for f in range(len(sources)):
        tx, ty = fa.t[f]
        for (ux, uy), got in (((tx, ty), fa.focus_t), ((-ty, tx), fa.focus_s)):
            for band in range(K):
                if v[f, band, 1] < 2:
                    continue
                c = [ux * ux, ux * uy, ux * uy, uy * uy]
                Cv, dC = np.dot(c, v[f, band, 11:15]), np.dot(np.abs(c), b[f, band, 11:15])
                q = [ux * ux, 2 * ux * uy, uy * uy]
                Vv, dV = np.dot(q, v[f, band, 15:18]), np.dot(np.abs(q), b[f, band, 15:18])
                want = origin[2] - Cv / Vv
                tol = quotient_tolerance(Cv, Vv, dC, dV) + 8 * EPS * (abs(want) + abs(origin[2]))
                assert abs(got[f, band] - want) <= tol, f"{what}: focus of field {f}, band {band}: {got[f, band]} against {want}, {tol:.2e}"
    return fields, key, K


def test_double_gauss_three_fields_three_lines():
    RT = double_gauss()
    fa = RT.field_analysis(sources=[0, 1, 2])
    fields, key, K = check_analysis(RT, fa, [0, 1, 2], None, "lines", "double Gauss, sources 0 1 2")
    assert K == 3 and fa.reference_band == 1 and fa.reference_field == 0 and fa.z == fa.focus_rms[0, 1]
    lines = np.array(ot.presets.spectral_lines.FdC, dtype=np.float32).astype(np.float64)
    assert np.allclose(fa.wavelengths, [486.1327, 589.2938, 656.272], rtol=1e-6)
    # the sources converge onto the lens: no constant orientation, no paraxial image
    assert np.all(np.isnan(fa.paraxial)) and np.all(np.isnan(fa.distortion))
    # (... and the source on the axis no direction: its field is no number, its tangential direction (0, 1))
    assert np.allclose(fa.t, [[0, 1], [0, -1], [0, -1]]) and np.all(np.isnan(fa.field[0])) and fa.field[1, 0] == 0 > fa.field[1, 1]
    # relative illumination: the ratio of two field points' total transmission
    fp = [RT.footprints(source_index=s).total_transmission for s in (0, 1, 2)]
    print(f"relative illumination {fa.relative_illumination}, footprints {np.array(fp) / fp[0]}")
    assert np.allclose(fa.relative_illumination, np.array(fp) / fp[0], rtol=1e-12, atol=0)
    # the order of the sources is the order of the result
    fb = RT.field_analysis(sources=[2, 0], z=fa.z)
    assert fb.sources.tolist() == [2, 0] and same_bits(fb.records[0], fa.records[2]) and same_bits(fb.records[1], fa.records[0])
    assert same_bits(fb.focus_t[0], fa.focus_t[2]) and np.array_equal(fb.field, fa.field[[2, 0]], equal_nan=True)
    assert np.array_equal(fb.field_curvature_t, fb.focus_t - fb.focus_rms[0][None, :])
    fc_ = RT.field_analysis(sources=[2, 0], z=fa.z, reference_field=1)
    assert np.array_equal(fc_.field_curvature_t[0], fa.field_curvature_t[2]) and fc_.relative_illumination[1] == 1
    # an earlier section, bands as edges
    fe = RT.field_analysis(sources=[1, 3], section=3, bands=np.array([450.0, 550, 600, 700]), z=0.0)
    check_analysis(RT, fe, [1, 3], 3, np.array([450.0, 550, 600, 700]), "double Gauss, section 3, edges")


def test_one_band_against_the_chromatic_analysis_of_every_source():
    RT = double_gauss()
    fa = RT.field_analysis(sources=[0, 1, 2], bands=1)
    assert fa.n_bands == 1
    p, w, wl = RT.rays.p_list, RT.rays.w_list, RT.rays.wl_list
    k = w.shape[1] - 2
    zeta = fa.z - fa.origin[2]
    for f, s in enumerate((0, 1, 2)):
        ca = RT.chromatic_analysis(source_index=s, bands=1, z=fa.z)
        first, count = int(RT.rays.B_list[s]), int(RT.rays.B_list[s + 1] - RT.rays.B_list[s])
        key = np.zeros(count, dtype=np.uint8)
        cval, cmag = cc.records(p, w, wl, first, count, k, key, 1, fa.z, centroid=cc.record_centroid(ca.records))
        val, mag = fc.records(p, w, wl, [(first, count)], k, key, first, 1, fa.origin, means=fc.record_means(fa.records[f:f + 1]))
        n, W = float(val[0, 0, 1]), float(val[0, 0, 0])
        assert fa.band_N[f, 0] == ca.band_N[0] == n and fa.band_power[f, 0] == pytest.approx(ca.band_power[0], rel=(n + 40) * EPS * 2)
        bc, bm = cc.sum_bound(n, F64(cmag[0])), cc.sum_bound(n, F64(mag[0, 0]))
        for c in range(2):
            tol = (bc[2 + c] + bm[2 + c] + abs(zeta) * bm[4 + c]) / W + 8 * EPS * (abs(fa.centroid[f, 0, c]) + abs(fa.origin[c]))
            assert abs(fa.centroid[f, 0, c] - ca.centroid[0, c]) <= tol, f"centroid {c} of source {s}"
        var = bc[5] + bc[6] + bm[8] + bm[10] + 2 * abs(zeta) * (bm[11] + bm[14]) + zeta ** 2 * (bm[15] + bm[17])
        tol = var / W / (2 * ca.rms_radius[0]) + 8 * EPS * ca.rms_radius[0]
        print(f"source {s}: rms radius {fa.rms_radius[f, 0]} against {ca.rms_radius[0]}, allowed {tol:.3e}")
        assert abs(fa.rms_radius[f, 0] - ca.rms_radius[0]) <= tol, f"rms radius of source {s}"


def test_deferred_planes_are_neither_read_nor_filled():
    """A trace that generates its rays on the device leaves the index plane and the polarisation planes unwritten.  The field
    figures of such a storage, its unwritten planes poisoned, are those of the storage once it is complete, bit for bit, and asking
    for them fills nothing."""
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=11)
        RT.trace(20000)
    r = RT.rays
    assert r._pol_stale is not None and r._n_stale
    raw = lambda key: dict.__getitem__(r._dev, key)
    raw("n").fill_(float("nan"))
    raw("pol").fill_(float("nan"))
    before = RT.field_analysis(sources=[0, 2, 4])
    assert r._pol_stale is not None and r._n_stale, "the field analysis filled a deferred plane"
    r._dev["n"], r._dev["pol"]  # (through the hook: the storage is complete now)
    assert r._pol_stale is None and not r._n_stale
    after = RT.field_analysis(sources=[0, 2, 4])
    assert same_bits(before.records, after.records) and before.z == after.z and before.n_bands == 3
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
    fa = RT.field_analysis()
    assert fa.band_N[:, 0].tolist() == [N, 0] and np.isfinite(fa.focus_rms[0, 0]) and np.all(np.isnan(fa.records[1, 0, 8:]))
    assert np.isnan(fa.focus_t[1, 0]) and np.all(np.isnan(fa.centroid[1])) and fa.relative_illumination[1] == 0
    assert 5 < fa.z < 12 and np.allclose(fa.paraxial[0, 0], [0, 0], atol=1e-12)
    # the reference field has no ray: no default plane
    with pytest.raises(RuntimeError, match="pass `z`"):
        RT.field_analysis(reference_field=1)
    # no chosen ray at all: the empty result, what the caller fixed stays
    e = RT.field_analysis(sources=[1], bands=np.array([400.0, 500, 600]), z=3.0)
    assert e.n_bands == 2 and e.z == 3.0 and e.reference_band == -1 and e.band_N.tolist() == [[0, 0]] and e.sources.tolist() == [1]
    assert np.all(np.isnan(e.focus_t)) and np.all(np.isnan(e.centroid))
    e = RT.field_analysis(sources=[1])
    assert e.n_bands == 1 and np.isnan(e.z) and e.band_edges is None
    # rays outside every band: the empty result too
    assert RT.field_analysis(bands=np.array([600.0, 700]), z=5.0).band_N.sum() == 0
