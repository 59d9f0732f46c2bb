"""Raytracer.wavefront_field and the `ot_wavefield_*` entry points on the GPU.

Truth is NumPy longdouble following the definition (tests/wavefront_field_cases.py): on synthetic storages handed to the entry
points through ctypes, and on the device's own ray storage read back for traced scenes.

Bounds, as stated with the feature: counts equal the truth; u, v, opl and w_out of every ray are the bits `ot_wavefront_paths`
writes for it with the sphere of its cell; every sum is within (n + 40) eps sum |terms| (`chromatic_cases.sum_bound`), n the cell's
count, the moments and the normal equations taken over the device's own planes, means and pupil, which are inputs of those passes;
two calls return the same bits; a field's outputs do not depend on the other fields of the call."""
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
import wavefront_cases as wc
import wavefront_field_cases as wfc
import scenes

pytestmark = pytest.mark.gpu

EPS, LD, NONE = wfc.EPS, wfc.LD, wfc.NO_BAND
F64 = lambda a: np.asarray(a).astype(np.float64)
ORIGIN = (0.25, -0.5, 0.5)


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def flat_ranges(fields):
    return (C.c_int64 * (2 * len(fields)))(*[int(v) for pair in fields for v in pair])


# ---- synthetic storages ----------------------------------------------------------------------------------------------------------
class Storage:
    """Host arrays p (N, nt, 3), n (N, nt), w (N, nt), wl (N,) in the layout of the reference and their planes on the device."""

    def __init__(self, p, n, w, wl):
        self.p, self.n, self.w, self.wl = p, n, w, wl
        self.N, self.nt = w.shape
        self.d_p = to_dev(np.ascontiguousarray(p.transpose(2, 1, 0)), np.float64)  # r + N * (i + nt * c)
        self.d_n = to_dev(np.ascontiguousarray(n.T), np.float64)
        self.d_w = to_dev(np.ascontiguousarray(w.T), np.float32)
        self.d_wl = to_dev(wl, np.float32)
        self.rays = _capi.Rays()
        self.rays.N, self.rays.nt = self.N, self.nt
        self.rays.p, self.rays.w, self.rays.wl, self.rays.n = (t.data_ptr() for t in (self.d_p, self.d_w, self.d_wl, self.d_n))


FAR_END = [-1e30, -2e30, -3e30]
FOCUS = np.array([0.3, -0.2, 20.0])


def build(counts, nt, k, first, K, seed, gaps=None, behind=37, keys=None, far=True):
    """-> (Storage, fields, key, key_first).  Field f owns `counts[f]` rays, `gaps[f]` rays after it belong to no field.  Section k
    of a living ray runs from a plane near z = 0 towards a point near FOCUS + (0.2 f, 0, 0), with an aberration of some hundredths;
    the sections before it are a random chain with indices between 1 and 1.7.  Four rays in five live in section k, the dead ones
    hold NaN positions and weight 0; some of the living have a section of no length.  Keys are drawn from 0 .. K - 1 and 255 unless
    `keys` gives them.  far: in every field of 8 rays or more one living ray in no band lies 1e30 away with a weight of 1e30.  The
    rays outside the fields hold used rays of 1e30 with the key 0, every other one of a gap NaN positions and a weight of 1.
    key_first lies 3 before the first field."""
    rng = np.random.default_rng(seed)
    gaps = [0] * len(counts) if gaps is None else gaps
    N = first + sum(counts) + sum(gaps) + behind
    p = np.full((N, nt, 3), 1e30)
    p[:, 1::2] = FAR_END
    n = np.full((N, nt), 1e30)
    w = np.full((N, nt), 1e30, dtype=np.float32)
    wl = np.full(N, 1e30, dtype=np.float32)
    key_first = max(first - 3, 0)
    key = np.zeros(N - key_first, dtype=np.uint8)
    fields, at = [], first
    for f, (count, gap) in enumerate(zip(counts, gaps)):
        fields.append((at, count))
        alive = rng.uniform(size=count) < 0.8
        q = np.cumsum(rng.uniform(0.5, 2.0, size=(count, nt, 3)) * [0.3, 0.3, 1.0], axis=1) - [0.0, 0.0, 2.0 * (k + 1)]
        q[:, :, :2] += rng.normal(size=(count, 1, 2)) * 2.0
        aim = FOCUS + [0.2 * f, 0.0, 0.0] + rng.normal(size=(count, 3)) * 0.03
        q[:, k + 1] = q[:, k] + (aim - q[:, k]) * rng.uniform(0.2, 0.6, size=(count, 1))
        kind = rng.uniform(size=count)
        q[kind < 0.03, k + 1] = q[kind < 0.03, k]  # no length: not used
        q[~alive] = np.nan
        wr = np.where(alive[:, None], rng.uniform(0.1, 1.0, size=(count, nt)), 0.0)
        kf = rng.choice(np.arange(K + 1), size=count) if keys is None else np.array(keys[f])
        kf = np.where(kf >= K, NONE, kf).astype(np.uint8)
        if far and count >= 8:
            spot = count // 3
            q[spot], wr[spot] = 1e30, 1e30
            q[spot, k + 1] = FAR_END
            kf[spot] = NONE
        p[at:at + count], w[at:at + count] = q, wr.astype(np.float32)
        n[at:at + count] = rng.uniform(1.0, 1.7, size=(count, nt))
        wl[at:at + count] = rng.uniform(400, 700, size=count).astype(np.float32)
        key[at - key_first:at - key_first + count] = kf
        p[at + count:at + count + gap:2] = np.nan
        w[at + count:at + count + gap:2] = 1.0
        at += count + gap
    return Storage(p, n, w, wl), fields, key, key_first


def sphere_choice(F, K, seed):
    """A sphere table: most cells a sphere about the field's focus of radius 12 to 16, converging; every fifth cell none (NaN);
    every seventh a sphere of radius 0.04 a little off the focus, which part of the lines miss; one diverging."""
    rng = np.random.default_rng(seed)
    sph = np.zeros((F, K, 4))
    for f in range(F):
        for b in range(K):
            c = FOCUS + [0.2 * f, 0.0, 0.0] + rng.normal(size=3) * 0.01
            sph[f, b] = [*c, rng.uniform(12, 16)]
            if (f * K + b) % 7 == 3:
                sph[f, b] = [c[0] + 0.03, c[1], c[2], 0.04]
            if (f * K + b) % 5 == 4:
                sph[f, b] = np.nan
            if (f * K + b) % 11 == 6:
                sph[f, b, 3] = -sph[f, b, 3]
    return sph


class Call:
    """The entry points on one storage: every output read back."""

    def __init__(self, S, fields, k, key, key_first, K, J):
        self.S, self.fields, self.k, self.key, self.key_first, self.K, self.J = S, fields, k, key, key_first, K, J
        self.F, self.lib, self.flat = len(fields), _capi.load_library(), flat_ranges(fields)
        self.d_key = to_dev(key, np.uint8)
        self.span = len(key)
        n_ws = self.lib.ot_wavefield_workspace(self.flat, self.F, K, J)
        assert n_ws > 0
        self.ws = torch.full((n_ws,), np.nan, dtype=torch.float64, device=dev())  # (a partial read before it is written shows)

    def focus(self, origin=ORIGIN):
        sums = torch.full((self.F * self.K * 17,), -7.0, dtype=torch.float64, device=dev())
        _capi.check(self.lib.ot_wavefield_focus(C.byref(self.S.rays), self.flat, self.F, self.k, ptr(self.d_key), self.key_first, self.K,
                                                (C.c_double * 3)(*origin), ptr(self.ws), ptr(sums), stream_ptr()))
        return sums.cpu().numpy().reshape(self.F, self.K, 17)

    def paths(self, spheres):
        span = self.span
        self.planes = torch.full((3 * span,), -7.0, dtype=torch.float64, device=dev())
        self.w_out = torch.full((span,), -7.0, dtype=torch.float32, device=dev())
        counts = torch.full((self.F * self.K * 2,), -7, dtype=torch.int64, device=dev())
        d_sph = to_dev(np.ascontiguousarray(spheres).reshape(-1), np.float64)
        self.uvl = [self.planes[i * span:(i + 1) * span] for i in range(3)]
        _capi.check(self.lib.ot_wavefield_paths(C.byref(self.S.rays), self.flat, self.F, self.k, ptr(self.d_key), self.key_first, self.K,
                                                ptr(d_sph), *(ptr(t) for t in self.uvl), ptr(self.w_out), ptr(counts), stream_ptr()))
        u, v, opl = (t.cpu().numpy() for t in self.uvl)
        return u, v, opl, self.w_out.cpu().numpy(), counts.cpu().numpy().reshape(self.F, self.K, 2)

    def d_wl(self):
        """wavelengths of the entries of the planes: the storage's from key_first on"""
        return self.S.d_wl[self.key_first:]

    def moments(self):
        mom = torch.full((self.F * self.K * 9,), -7.0, dtype=torch.float64, device=dev())
        pupil = torch.full((self.F * 4,), -7.0, dtype=torch.float64, device=dev())
        _capi.check(self.lib.ot_wavefield_moments(self.flat, self.F, *(ptr(t) for t in self.uvl), ptr(self.w_out), ptr(self.d_wl()),
                                                  ptr(self.d_key), self.key_first, self.K, ptr(self.ws), ptr(mom), ptr(pupil), stream_ptr()))
        self.d_mom, self.d_pupil = mom, pupil
        return mom.cpu().numpy().reshape(self.F, self.K, 9), pupil.cpu().numpy().reshape(self.F, 4)

    def zernike(self, pupil_radius=None):
        J = self.J
        out = torch.full((self.F * self.K * (J * (J + 1) // 2 + J),), -7.0, dtype=torch.float64, device=dev())
        _capi.check(self.lib.ot_wavefield_zernike(self.flat, self.F, *(ptr(t) for t in self.uvl), ptr(self.w_out), ptr(self.d_key),
                                                  self.key_first, self.K, ptr(self.d_mom), ptr(self.d_pupil),
                                                  np.nan if pupil_radius is None else pupil_radius, J, ptr(self.ws), ptr(out), stream_ptr()))
        return out.cpu().numpy().reshape(self.F, self.K, -1)

    def everything(self, spheres, pupil_radius=None):
        u, v, opl, w_out, counts = self.paths(spheres)
        mom, pupil = self.moments()
        return dict(u=u, v=v, opl=opl, w=w_out, counts=counts, mom=mom, pupil=pupil, normal=self.zernike(pupil_radius))


def single_paths(S, first, count, k, sphere):
    """`ot_wavefront_paths` on the rays [first, first + count) with one sphere -> (u, v, opl, w_out, missed, device tensors)"""
    lib = _capi.load_library()
    planes = torch.full((3 * count,), -7.0, dtype=torch.float64, device=dev())
    w_out = torch.full((count,), -7.0, dtype=torch.float32, device=dev())
    missed = torch.zeros(1, dtype=torch.int64, device=dev())
    uvl = [planes[i * count:(i + 1) * count] for i in range(3)]
    _capi.check(lib.ot_wavefront_paths(C.byref(S.rays), first, count, k, (C.c_double * 3)(*sphere[:3]), float(sphere[3]),
                                       *(ptr(t) for t in uvl), ptr(w_out), ptr(missed), stream_ptr()))
    return [t.cpu().numpy() for t in uvl] + [w_out.cpu().numpy(), int(missed.cpu()[0]), uvl + [w_out]]


def check_bits_of_single_paths(S, fields, k, key, key_first, K, spheres, got, what):
    """u, v, opl and w_out of every used ray of a cell with a sphere: the bits of `ot_wavefront_paths` with that sphere."""
    for f, (first, count) in enumerate(fields):
        kf = wfc.band_of(key, key_first, first, count)
        for b in range(K):
            sel = np.nonzero(kf == b)[0]
            if not sel.shape[0] or not wfc.has_sphere(spheres[f, b]):
                continue
            u, v, opl, w_out, _, _ = single_paths(S, first, count, k, spheres[f, b])
            at = first - key_first + sel
            for name, one in (("u", u), ("v", v), ("opl", opl), ("w", w_out)):
                assert same_bits(got[name][at], one[sel]), f"{what}: {name} of cell ({f}, {b}) is not ot_wavefront_paths'"


def check_entry_points(S, fields, k, key, key_first, K, J, spheres, what, alone=True, pupil_radius=None):
    """-> outputs of the device, checked against the oracle; twice the same bits; every field alone gives the bits it has among the
    others."""
    call = Call(S, fields, k, key, key_first, K, J)
    F = len(fields)
    sums = call.focus()
    assert same_bits(sums, call.focus()), f"{what}: two focus calls, different bits"
    val, mag = wfc.focus_sums(S.p, S.w, fields, k, key, key_first, K, ORIGIN)
    shares = [cc.check_focus_sums(sums[f], val[f], mag[f], f"{what}, field {f}") for f in range(F) if fields[f][1]]
    got = call.everything(spheres, pupil_radius)
    again = call.everything(spheres, pupil_radius)
    for name in got:
        assert same_bits(got[name], again[name]), f"{what}: two calls, different bits in {name}"
    truth = wfc.paths(S.p, S.n, S.w, fields, k, key, key_first, K, spheres, call.span)
    assert np.array_equal(got["counts"][:, :, 0], truth["n_missed"]) and np.array_equal(got["counts"][:, :, 1], truth["n_no_sphere"]), \
        f"{what}: counts {got['counts'].tolist()} against {truth['n_missed'].tolist()}, {truth['n_no_sphere'].tolist()}"
    wfc.check_planes(got["u"], got["v"], got["opl"], got["w"], truth, what)
    outside = ~truth["inside"]
    assert np.all(got["w"][outside] == -7.0) and np.all(got["opl"][outside] == -7.0), f"{what}: entries of no field were written"
    check_bits_of_single_paths(S, fields, k, key, key_first, K, spheres, got, what)
    wl = S.wl[key_first:]
    mval, mmag, tpupil = wfc.moments(got["u"], got["v"], got["opl"], got["w"], wl, fields, key, key_first, K,
                                     means=wfc.record_means(got["mom"]), centre=got["pupil"][:, :2])
    wfc.check_moments(got["mom"], got["pupil"], mval, mmag, tpupil, what)
    centre, cbound = wfc.centre_bound(mval, mmag)
    some = mval[..., 1].sum(axis=1) > 0
    off = np.abs(got["pupil"][some][:, :2].astype(LD) - centre[some]).astype(np.float64)
    assert np.all(off <= cbound[some]), f"{what}: pupil centre off by {off} against {cbound[some]}"
    neq = wfc.normal_equations(got["u"], got["v"], got["opl"], got["w"], fields, key, key_first, K, got["mom"], got["pupil"],
                               pupil_radius, J)
    wfc.check_normal(got["normal"], neq, F, K, J, what)
    if alone and F > 1:
        for f, one in enumerate(fields):
            if one[1]:
                check_alone(S, fields, f, k, key, key_first, K, J, spheres, sums, got, what, pupil_radius)
    return sums, got


def check_alone(S, fields, f, k, key, key_first, K, J, spheres, sums, got, what, pupil_radius=None):
    one = Call(S, [fields[f]], k, key, key_first, K, J)
    assert same_bits(sums[f], one.focus()[0]), f"{what}: field {f} alone, focus sums differ"
    alone = one.everything(spheres[f:f + 1], pupil_radius)
    first, count = fields[f]
    at = slice(first - key_first, first - key_first + count)
    for name in ("u", "v", "opl", "w"):
        assert same_bits(got[name][at], alone[name][at]), f"{what}: field {f} alone, plane {name} differs"
    for name in ("counts", "mom", "pupil", "normal"):
        assert same_bits(got[name][f], alone[name][0]), f"{what}: field {f} alone, {name} differs"


@pytest.mark.parametrize("counts,gaps,nt,k,first,K,J", [
    ([1], None, 2, 0, 5, 1, 1), ([63, 64], None, 5, 3, 5, 3, 15), ([65, 255, 256], [0, 7, 0], 2, 0, 33, 32, 16),
    ([257, 0, 3000], [5, 0, 11], 5, 3, 7, 3, 36),                # a field of no rays between two, gaps of rays of no field
    ([3000, 1, 64], [1, 1, 1], 5, 0, 3, 32, 15),                 # a field of one ray
    ([256 * 1024 + 1, 65], [3, 0], 2, 0, 7, 3, 15),              # one ray more than a field's launch has lanes
    ([3000], None, 5, 3, 64, 1, 36),
])
def test_entry_points_on_random_planes(counts, gaps, nt, k, first, K, J):
    seed = sum(counts) + 7 * nt + K
    S, fields, key, key_first = build(counts, nt, k, first, K, seed, gaps=gaps)
    check_entry_points(S, fields, k, key, key_first, K, J, sphere_choice(len(counts), K, seed),
                       f"fields of {counts} rays, nt {nt}, section {k}, {K} bands, {J} polynomials")


def test_a_given_pupil_radius_leaves_entries_out_of_the_normal_equations_only():
    S, fields, key, key_first = build([700, 300], 3, 1, 16, 3, 5, far=False)
    sph = sphere_choice(2, 3, 1)
    _, free = check_entry_points(S, fields, 1, key, key_first, 3, 6, sph, "two fields, the moments' pupil", alone=False)
    pr = 0.6 * free["pupil"][0, 3]
    _, cut = check_entry_points(S, fields, 1, key, key_first, 3, 6, sph, "two fields, a given pupil radius", pupil_radius=pr)
    assert same_bits(free["mom"], cut["mom"]) and same_bits(free["pupil"], cut["pupil"])
    assert not same_bits(free["normal"], cut["normal"])


def test_sixty_four_fields_and_the_last_ends_with_the_storage():
    counts = [(37 * f) % 131 + (f % 3 == 0) for f in range(64)]
    assert 0 in counts or min(counts) <= 1
    S, fields, key, key_first = build(counts, 4, 2, 13, 3, 8, gaps=[(f + 1) % 2 for f in range(64)], behind=0)
    assert fields[-1][0] + fields[-1][1] == S.N and any(a % 16 for a, _ in fields)
    sph = sphere_choice(64, 3, 8)
    sums, got = check_entry_points(S, fields, 2, key, key_first, 3, 15, sph, "64 fields", alone=False)
    for f in (1, 17, 63):  # three of the fields alone: the bits they have among the 64
        check_alone(S, fields, f, 2, key, key_first, 3, 15, sph, sums, got, "64 fields")


def test_waves_of_one_band_and_of_all_bands_and_bands_without_a_ray():
    """Two fields of 640 rays, 32 bands: the first wave of field 0 holds rays of band 5 alone, its second wave all 32 bands, two
    rays each; the rest of field 0 lies in band 1.  Field 1: every ray in band 30."""
    count, K = 640, 32
    k0 = np.ones(count, dtype=np.int64)
    k0[:64], k0[64:128] = 5, np.arange(64) % 32
    S, fields, key, key_first = build([count, count], 3, 1, 11, K, 21, keys=[k0, np.full(count, 30)], far=False)
    sph = sphere_choice(2, K, 21)
    sph[0, 5], sph[0, 1], sph[1, 30] = [*FOCUS, 14.0], [*FOCUS, 13.0], [*(FOCUS + [0.2, 0, 0]), 15.0]
    sums, got = check_entry_points(S, fields, 1, key, key_first, K, 15, sph, "special waves")
    assert np.all(sums[1, :30, :] == 0) and np.all(sums[1, 31, :] == 0) and sums[1, 30, 1] > 400
    assert np.all(got["mom"][1, :30, :8] == 0) and np.all(np.isnan(got["mom"][1, :30, 8])) and got["mom"][1, 30, 1] > 400


def test_cells_of_one_sphere_add_up_to_the_single_bundle_moments():
    """One field, three bands, one common sphere: slots 0, 1 and 5 of the moments added over the cells against `ot_wavefront_moments`
    on the planes of `ot_wavefront_paths` with that sphere, each side within its bound."""
    K, k = 3, 1
    S, fields, key, key_first = build([2000], 3, k, 16, K, 5, far=False, keys=[np.arange(2000) % 3])
    sph = np.tile([*FOCUS, 14.0], (1, K, 1))
    _, got = check_entry_points(S, fields, k, key, key_first, K, 15, sph, "one field, one sphere")
    first, count = fields[0]
    u, v, opl, w_out, missed, d = single_paths(S, first, count, k, sph[0, 0])
    lib = _capi.load_library()
    ws = torch.empty(_capi.WF_WS, dtype=torch.float64, device=dev())
    mom = torch.zeros(_capi.WF_M, dtype=torch.float64, device=dev())
    _capi.check(lib.ot_wavefront_moments(count, *(ptr(t) for t in d), ptr(S.d_wl[first:first + count]), ptr(ws), ptr(mom), stream_ptr()))
    whole = mom.cpu().numpy()
    assert missed == got["counts"][0, :, 0].sum() and whole[1] == got["mom"][0, :, 1].sum()
    tval, tmag = wc.first_moments(u, v, opl, w_out, S.wl[first:first + count])
    mval, mmag, _ = wfc.moments(got["u"], got["v"], got["opl"], got["w"], S.wl[key_first:], fields, key, key_first, K)
    for s in (0, 5):
        bound = cc.sum_bound(F64(mval[0, :, 1]), F64(mmag[0, :, s])).sum() + wc.sum_bound(float(tval[1]), float(tmag[s]))
        apart = float(abs(got["mom"][0, :, s].astype(LD).sum() - LD(whole[s])))
        assert apart <= bound, f"slot {s}: {apart} above {bound}"


def test_no_ray_in_any_field_launches_nothing():
    S, fields, key, key_first = build([10], 3, 0, 0, 2, 2)
    call = Call(S, [(10, 0), (3, 0)], 0, key, 0, 2, 15)
    call.ws.fill_(0.0)
    assert np.all(call.focus() == -7.0)
    got = call.everything(sphere_choice(2, 2, 0))
    assert all(np.all(a == -7) for a in got.values()) and np.all(call.ws.cpu().numpy() == 0)


# ---- Raytracer.wavefront_field on traced rays ----------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def double_gauss():
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=7)
        RT.trace(20000)
    return RT


def storage_of(RT):
    r = RT.rays
    return Storage(r.p_list, r.n_list, r.w_list, r.wl_list)


def fields_of(RT, sources):
    return [(int(RT.rays.B_list[s]), int(RT.rays.B_list[s + 1] - RT.rays.B_list[s])) for s in sources]


def check_analysis(RT, wf, sources, section, bands, what, pupil_radius=None):
    """Every cell of `wf` against the oracle on the storage read back: the records are the entry points' on that storage with the
    result's spheres, and those are held to the oracle."""
    S = storage_of(RT)
    k = S.nt - 2 if section is None else section
    fields = fields_of(RT, sources)
    used = np.zeros(S.N, dtype=bool)
    for first, count in fields:
        used[first:first + count] = cc.used_rays(S.p, S.w, first, count, k)[0]
    key, K, edges = cc.band_keys(S.wl, used, bands)
    assert wf.n_bands == K and wf.section == k and wf.n_fields == len(sources) and wf.sources.tolist() == list(sources)
    assert wf.band_edges is None if edges is None else np.array_equal(wf.band_edges, edges)
    spheres = np.concatenate([wf.focus, wf.radius[:, :, None]], axis=2)
    lo = min(a for a, c in fields if c)
    hi = max(a + c for a, c in fields if c)
    key8 = key.astype(np.uint8)[lo:hi]
    sums, got = check_entry_points(S, fields, k, key8, lo, K, wf.n_zernike, spheres, what, alone=False, pupil_radius=pupil_radius)
    assert same_bits(wf.moments, got["mom"]) and same_bits(wf.normal, got["normal"]) and same_bits(wf.pupil, got["pupil"]), \
        f"{what}: the records are not the entry points'"
    assert np.array_equal(wf.n_missed, got["counts"][:, :, 0]) and np.array_equal(wf.n_no_sphere, got["counts"][:, :, 1])
    return S, fields, key8, lo, K, sums, got


def test_double_gauss_three_fields_three_lines():
    RT = double_gauss()
    wf = RT.wavefront_field(sources=[0, 1, 2])
    S, fields, key8, lo, K, sums, got = check_analysis(RT, wf, [0, 1, 2], None, "lines", "double Gauss, sources 0 1 2")
    assert K == 3 and wf.reference_band == 1 and wf.sphere == "field" and wf.zernike.shape == (3, 3, 15)
    assert np.allclose(wf.wavelengths, [486.1327, 589.2938, 656.272], rtol=1e-6)
    # one sphere per field: that of the reference band, formed by the host from the device's focus sums
    origin = np.array(SectionTable(RT).origin(S.nt - 2, None), dtype=np.float64)
    from optrace_amd.wavefront_field import sphere_table
    assert same_bits(sphere_table(Call(S, fields, S.nt - 2, key8, lo, K, 15).focus(origin), origin, "field", 1),
                     np.concatenate([wf.focus, wf.radius[:, :, None]], axis=2))
    assert np.all(wf.focus == wf.focus[:, 1:2]) and np.all(wf.radius == wf.radius[:, 1:2]) and np.all(np.isfinite(wf.zernike))
    # the coefficients against a longdouble solve of the true normal equations: within the first-order bound of the solve
    neq = wfc.normal_equations(got["u"], got["v"], got["opl"], got["w"], fields, key8, lo, K, got["mom"], got["pupil"], None, 15)
    for (f, b), (tG, aG, tg, ag, n) in neq.items():
        check_solution(wf.zernike[f, b], tG, tg, cc.sum_bound(n, F64(aG)), cc.sum_bound(n, F64(ag)), f"cell ({f}, {b})")
    # sphere="field" against "band" at the reference band: the same sphere, so equal bits in everything that is the cell's own --
    # the counts, the moments and the figures from them.  (The normal equations are not: they live on the field's pupil, whose
    # centre and radius are common to the bands and move with the other bands' spheres.)
    wb = RT.wavefront_field(sources=[0, 1, 2], sphere="band")
    for name in ("moments", "focus", "radius", "n_missed", "band_N", "opl_mean", "opd_rms", "opd_pv", "rms_waves", "strehl"):
        assert same_bits(getattr(wb, name)[:, 1], getattr(wf, name)[:, 1]), f"sphere='band' at the reference band: {name} differs"
    assert not same_bits(wb.focus[:, 0], wf.focus[:, 0]) and not same_bits(wb.moments[:, 0], wf.moments[:, 0])
    # ... and with one band there is no other band: the two are one, normal equations and coefficients too
    one_f, one_b = (RT.wavefront_field(sources=[0, 2], bands=1, sphere=s) for s in ("field", "band"))
    assert same_bits(one_f.normal, one_b.normal) and same_bits(one_f.zernike, one_b.zernike) and same_bits(one_f.pupil, one_b.pupil)
    check_analysis(RT, wb, [0, 1, 2], None, "lines", "double Gauss, a sphere per band")
    # the order of the sources is the order of the result
    wr = RT.wavefront_field(sources=[2, 0])
    for name in ("moments", "normal", "pupil", "zernike", "focus", "radius", "n_missed", "rms_waves", "strehl_all"):
        a, b = getattr(wr, name), getattr(wf, name)
        assert same_bits(a[0], b[2]) and same_bits(a[1], b[0]), f"sources [2, 0]: {name} is not the rows of [0, 2] swapped"
    # an earlier section, bands as edges
    edges = np.array([450.0, 550, 600, 700])
    we = RT.wavefront_field(sources=[1, 3], section=3, bands=edges, n_zernike=6)
    check_analysis(RT, we, [1, 3], 3, edges, "double Gauss, section 3, edges")


def check_solution(a, G, g, dG, dg, what, extra=0.0):
    """Coefficients `a` of a float64 solve against the longdouble solution of G x = g, G and g known within dG and dg: to first
    order |da| <= cond(G) (|dG| / |G| + |dg| / |g|) |a| in the 2-norm; the solve's own backward error, J eps |G| by the usual bound
    of an elimination with pivoting, counts as a part of dG."""
    J = len(a)
    x = wfc.solve_ld(G, g)
    G64 = F64(G)
    cond = np.linalg.cond(G64)
    rel = (np.linalg.norm(dG) + extra) / np.linalg.norm(G64) + J * EPS + np.linalg.norm(dg) / np.linalg.norm(F64(g))
    err = np.linalg.norm(F64(a.astype(LD) - x))
    print(f"{what}: cond(G) {cond:.3g}, coefficients off by {err:.3g}, allowed {cond * rel * np.linalg.norm(F64(x)):.3g}")
    assert err <= cond * rel * np.linalg.norm(F64(x)), what


def test_one_band_against_the_wavefront_analysis_of_every_source():
    RT = double_gauss()
    S = storage_of(RT)
    k, J, lib = S.nt - 2, 15, _capi.load_library()
    for f in (0, 1, 2):
        wf = RT.wavefront_field(sources=[f], bands=1, sphere="band")
        wa = RT.wavefront_analysis(source_index=f, focus=wf.focus[0, 0], radius=float(wf.radius[0, 0]))
        assert wf.band_N[0, 0] == wa.N and wf.n_missed[0, 0] == wa.n_missed and wf.n_no_sphere[0, 0] == 0
        print(f"source {f}: pupil radius {wf.pupil_radius[0]!r} against {wa.pupil_radius!r}, rms {wf.opd_rms[0, 0]!r} against {wa.rms!r}")
        assert wf.pupil_radius[0] == wa.pupil_radius
        # G and g of the single bundle through its entry points, on the same storage
        first, count = fields_of(RT, [f])[0]
        sphere = [*wf.focus[0, 0], wf.radius[0, 0]]
        u, v, opl, w_out, missed, d = single_paths(S, first, count, k, sphere)
        ws = torch.empty(_capi.WF_WS, dtype=torch.float64, device=dev())
        res = torch.zeros(_capi.WF_M + J * (J + 1) // 2 + J, dtype=torch.float64, device=dev())
        _capi.check(lib.ot_wavefront_moments(count, *(ptr(t) for t in d), ptr(S.d_wl[first:first + count]), ptr(ws), ptr(res), stream_ptr()))
        _capi.check(lib.ot_wavefront_zernike(count, *(ptr(t) for t in d), ptr(res), np.nan, J, ptr(ws), ptr(res[_capi.WF_M:]), stream_ptr()))
        h = res.cpu().numpy()
        mom1, packed1 = h[:_capi.WF_M], h[_capi.WF_M:]
        tG1, aG1, tg1, ag1, n1 = wc.normal_equations(u, v, opl, w_out.astype(np.float64), mom1, None, J)
        key = np.zeros(count, dtype=np.uint8)
        neq = wfc.normal_equations(u, v, opl, w_out, [(first, count)], key, first, 1, wf.moments, wf.pupil, None, J)
        tG, aG, tg, ag, n = neq[0, 0]
        assert n == n1 == wa.N
        G, g = wfc.unpack(wf.normal[0, 0], J)
        G1, g1 = wfc.unpack(packed1, J)
        # (both sides sum the same rays, each about its own means and pupil: the truths differ by that, the sums by their bounds)
        dG = cc.sum_bound(n, F64(aG)) + cc.sum_bound(n1, F64(aG1)) + np.abs(F64(tG - tG1))
        dg = cc.sum_bound(n, F64(ag)) + cc.sum_bound(n1, F64(ag1)) + np.abs(F64(tg - tg1))
        assert np.all(np.abs(G - G1) <= dG) and np.all(np.abs(g - g1) <= dg), f"source {f}: normal equations apart"
        check_solution(wf.zernike[0, 0], tG1, tg1, dG, dg, f"source {f} against the single bundle")


def test_deferred_planes_are_filled_on_demand_and_the_polarisation_left_alone():
    """A trace that generates its rays on the device leaves the index plane and the polarisation planes unwritten.  The paths read
    the index plane, so the analysis fills it, and leaves the polarisation alone; the figures are those of the complete storage,
    bit for bit."""
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=11)
        RT.trace(20000)
    r = RT.rays
    assert r._pol_stale is not None and r._n_stale
    raw = lambda key: dict.__getitem__(r._dev, key)
    raw("n").fill_(float("nan"))
    raw("pol").fill_(float("nan"))
    before = RT.wavefront_field(sources=[0, 2, 4])
    assert r._pol_stale is not None and not r._n_stale, "the polarisation planes were filled, or the index plane was not"
    r._dev["pol"]
    after = RT.wavefront_field(sources=[0, 2, 4])
    assert same_bits(before.moments, after.moments) and same_bits(before.normal, after.normal) and before.n_bands == 3
    assert np.all(np.isfinite(before.opd_rms))
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
    wf = RT.wavefront_field(n_zernike=11)
    assert wf.band_N[:, 0].tolist() == [N, 0] and np.isfinite(wf.opd_rms[0, 0]) and np.isnan(wf.opd_rms[1, 0])
    assert np.all(np.isnan(wf.zernike[1])) and np.all(np.isfinite(wf.zernike[0])) and np.all(np.isnan(wf.pupil_centre[1]))
    assert wf.n_no_sphere.tolist() == [[0], [0]] and 5 < wf.focus[0, 0, 2] < 12 and wf.radius[0, 0] > 0
    assert wf.named()["spherical"][0, 0] != 0 and np.isnan(wf.strehl_all[1])
    # the section in front of the lens is collimated: no sphere, every used ray counted
    wc_ = RT.wavefront_field(section=0)
    assert wc_.n_no_sphere.tolist() == [[N], [0]] and wc_.band_N.sum() == 0 and np.all(np.isnan(wc_.focus))
    # ... unless the caller gives one
    wg = RT.wavefront_field(section=0, focus=[[0, 0, 50.0], [0, 0, 50.0]], radius=40.0, n_zernike=4)
    assert wg.band_N[:, 0].tolist() == [N, 0] and wg.n_no_sphere.sum() == 0 and np.all(wg.focus[0, 0] == [0, 0, 50.0])
    # no chosen ray at all: the empty result, what the caller fixed stays
    e = RT.wavefront_field(sources=[1], bands=np.array([400.0, 500, 600]), n_zernike=3)
    assert e.n_bands == 2 and e.reference_band == -1 and e.band_N.tolist() == [[0, 0]] and e.sources.tolist() == [1]
    assert e.zernike.shape == (1, 2, 3) and np.all(np.isnan(e.zernike)) and np.all(np.isnan(e.opd_rms))
    e = RT.wavefront_field(sources=[1])
    assert e.n_bands == 1 and e.band_edges is None
    assert RT.wavefront_field(bands=np.array([600.0, 700])).band_N.sum() == 0
