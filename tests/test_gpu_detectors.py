"""The detector stage on the device (csrc/ot_detector.hpp, ot_detector_fused.hpp, ot_render_tiles.hpp, the routing in
raytracer.py / detector.py) against the reference for every detector kind at every placement, and against the oracle.

tests/golden/detectors.npz holds two traced scenes of the reference and, per (kind, placement, projection), its detector
hits and images; tests/test_oracle_detectors.py pins the oracle to the same records on the CPU.  The recorded rays are
injected, traced on the device, and every record is compared: hit lists, images through every binning route, batches of
requests, compact lists, sub-ranges of the rays, rays that died inside a detector's z-range.  Then the device against the
oracle on random systems, and render-only chunks against the stored path.  The generator keeps every recorded ray off the
decision thresholds of the search: nothing is excluded.  Reference: raytracer.py:881-1098, 1134-1279."""
import ctypes as C

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi, detector as _detector

import oracle_bridge as ob
import scenes
from detector_fixture import fixture, records, record_id
from helpers import assert_close
from test_gpu_fused_detector import same_image

pytestmark = pytest.mark.gpu

_traced = {}


def traced(name):
    """The fixture scene `name` with one detector per kind, the recorded rays injected and traced.  -> (RT, kind -> index)"""
    if name not in _traced:
        builder, N, rt_args = scenes.DETECTOR_SCENES[name]
        sc = fixture().scene(name)
        with ot.global_options.no_warnings():
            RT = builder(ot, **rt_args)
            idx = scenes.add_detectors(ot, RT)
            RT.trace(N, _initial_rays=(sc["p0"], sc["s0"], sc["pol0"], sc["w0"], sc["wl"]), _N_list=sc["N_list"])
        assert not RT.geometry_error and RT.rays.p_list.shape == sc["p_list"].shape
        _traced[name] = (RT, idx)
    return _traced[name]


def placed(rec):
    """-> (RT, detector index, fixture record) with the detector moved to where the record's stood"""
    name, kind, place, proj = rec
    RT, idx = traced(name)
    g = fixture().record(record_id(rec))
    RT.detectors[idx[kind]].move_to(g["pos"])
    return RT, idx[kind], g


def host_hits(RT, di, proj, **kw):
    ph, hw, wl, ext, projection, ill = RT._hit_detector("x", di, kw.get("source_index"), kw.get("extent"), proj)
    n = hw.shape[0]
    return ph.cpu().numpy().reshape(3, n).T, hw.cpu().numpy(), wl.cpu().numpy(), np.asarray(ext), ill


def fused_kind(kind, proj) -> bool:
    """the routing rule, stated per kind: closed-form hit and no sphere projection with a transcendental"""
    return kind in scenes.DETECTOR_CLOSED and proj in (None, "Orthographic")


def image_on_device(im):
    """the fixture's image as a device tensor"""
    return torch.from_numpy(im["dense"]).cuda()


def check_image(img, im, what):
    """power to 1e-6, image norm (sum |a - b| / sum |b| per channel) below 1e-4, like test_detector_image_matches_reference;
    formed on the device where the image still lives there"""
    assert_close(img.extent, im["extent"], rtol=1e-9, atol=1e-11, what=f"{what}: image extent")
    pw = im["power"]
    a = img._dev if img._dev is not None else torch.from_numpy(img._data).cuda()
    b = image_on_device(im)
    assert tuple(a.shape) == tuple(b.shape), what
    power = float(a[..., 3].sum())
    print(f"{what}: power {power!r} against {pw!r}")
    assert abs(power - pw) <= 1e-6 * max(pw, 1e-300), what
    if pw > 0:
        err = ((a - b).abs().sum(dim=(0, 1)) / b.abs().sum(dim=(0, 1)).clamp_min(1e-300)).cpu().numpy()
        print(f"{what}: image norm {err}")
        assert np.all(err < 1e-4), (what, err)


# ---- hit lists and images ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("rec", records(), ids=record_id)
def test_hits_match_reference(rec):
    RT, di, g = placed(rec)
    name, kind, place, proj = rec
    with ot.global_options.no_warnings():
        ph, hw, wl, ext, ill = host_hits(RT, di, proj)
    assert np.isfinite(ph).all() and np.isfinite(hw).all() and np.isfinite(ext).all(), "no NaN leaves the hit kernel"
    sel = hw > 0
    assert np.count_nonzero(sel) == g["w"].shape[0], "number of detector hits must be exact"
    assert not ph[~sel].any(), "rays without a valid hit: zeros"
    if sel.any():
        print("largest weight difference", np.abs(hw[sel].astype(np.float64) - g["w"]).max())
    assert np.array_equal(hw[sel], g["w"])  # (no float32 exp, no tabulated spectrum in these scenes: bit for bit)
    assert np.array_equal(wl[sel], g["wl"])
    assert_close(ph[sel], g["ph"], rtol=1e-9, atol=1e-11, what="ph")
    assert ill == g["ill"]
    if sel.any():
        assert_close(ext, g["extent"], rtol=1e-9, atol=1e-11, what="auto extent")
    else:
        assert np.array_equal(ext, g["extent"]), "without a hit: the detector's centre"


ROUTES = [(None, None), ("direct", None), ("tiles", None), ("tiles", "0")]


@pytest.fixture(params=ROUTES, ids=["probe", "direct", "tiles", "tiles, plain tile kernel"])
def binning_route(request, monkeypatch):
    path, linebuf = request.param
    for key, val in (("OT_RENDER_PATH", path), ("OT_TILE_LINEBUF", linebuf)):
        if val is None:
            monkeypatch.delenv(key, raising=False)
        else:
            monkeypatch.setenv(key, val)
    return request.param


class calls:
    """counts the calls of the detector stage's entry points (optrace_amd.detector) made inside"""
    NAMES = ("detector_hits_multi", "detector_images", "detector_extent_sample", "AutoImage")

    def __init__(self, monkeypatch):
        self.n = dict.fromkeys(self.NAMES, 0)
        for name in self.NAMES:
            monkeypatch.setattr(_detector, name, self._wrap(name, getattr(_detector, name)))

    def _wrap(self, name, orig):
        def spy(*a, **k):
            self.n[name] += 1
            return orig(*a, **k)
        return spy


@pytest.mark.parametrize("rec", records(), ids=record_id)
def test_images_match_reference(rec, binning_route, monkeypatch):
    """detector_image with the automatic extent (at this size: the hit-list chain for every kind) and with a user extent and
    the last source alone (`ot_detector_images`: the fused kernels for closed-form detectors without a projection, the chain
    inside the library otherwise), each against the reference's image."""
    RT, di, g = placed(rec)
    name, kind, place, proj = rec
    fx = fixture()
    seen = calls(monkeypatch)
    with ot.global_options.no_warnings():
        img = RT.detector_image(detector_index=di, projection_method=proj)
    assert seen.n == dict(detector_hits_multi=1, detector_images=0, detector_extent_sample=0, AutoImage=0)
    check_image(img, fx.image(record_id(rec)), f"{record_id(rec)} automatic extent {binning_route}")
    if proj in (None, scenes.SPHERE_PROJECTIONS[0]):
        im = fx.image(f"{name}/{kind}/{place}/user")
        with ot.global_options.no_warnings():
            img = RT.detector_image(detector_index=di, extent=list(im["uext"]), projection_method=proj,
                                    source_index=len(RT.ray_sources) - 1)
        assert seen.n == dict(detector_hits_multi=1, detector_images=1, detector_extent_sample=0, AutoImage=0)
        check_image(img, im, f"{record_id(rec)} user extent {binning_route}")


ONE_PASS = {}  # (kind, projection) -> records where the one-pass form applied


@pytest.mark.parametrize("linebuf", [None, "0"], ids=["line buffers", "plain tile kernel"])
@pytest.mark.parametrize("rec", records(), ids=record_id)
def test_one_pass_route_per_kind(rec, linebuf, monkeypatch):
    """With the one-pass form switched on for every bundle size: detectors with a closed-form hit and no projection are
    offered to it (sample pass, then `AutoImage` or, where the sample says no, the chain); numeric and projected detectors
    never are -- they take the hit-list chain.  Either way the reference's image comes out."""
    RT, di, g = placed(rec)
    name, kind, place, proj = rec
    monkeypatch.setattr(ot.Raytracer, "AUTO_ONE_PASS_FROM", 1)
    if linebuf is None:
        monkeypatch.delenv("OT_TILE_LINEBUF", raising=False)
    else:
        monkeypatch.setenv("OT_TILE_LINEBUF", linebuf)
    assert _capi.fused_ok(RT.detectors[di].surface._desc(), _capi.PROJECTIONS[proj]) == fused_kind(kind, proj)
    assert _capi.numeric_hit(RT.detectors[di].surface._desc()) == (kind in scenes.DETECTOR_NUMERIC)
    seen = calls(monkeypatch)
    with ot.global_options.no_warnings():
        img = RT.detector_image(detector_index=di, projection_method=proj)
    if fused_kind(kind, proj):
        assert seen.n["detector_extent_sample"] == 1
        assert seen.n["AutoImage"] + seen.n["detector_hits_multi"] >= 1
        if seen.n["AutoImage"] and not seen.n["detector_hits_multi"]:
            ONE_PASS.setdefault((kind, proj), []).append(place)
    else:
        assert seen.n == dict(detector_hits_multi=1, detector_images=0, detector_extent_sample=0, AutoImage=0)
    check_image(img, fixture().image(record_id(rec)), f"{record_id(rec)} one pass")


def test_one_pass_form_served_every_closed_form_kind():
    """(after the test above) every kind the one-pass form is meant for has been rendered by it somewhere"""
    want = {(k, p) for _, k, _, p in records() if fused_kind(k, p)}
    print({k: sorted(set(v)) for k, v in ONE_PASS.items()})
    assert set(ONE_PASS) == want


# ---- batches, spectra, ray counts ---------------------------------------------------------------------------------
def record(surf, proj, **kw):
    """a request over ray ranges given with the call, without a crop: the hits' extent comes back"""
    return _detector.DetectorRequest(0, None, surf, proj, None, 0, None, "", **kw)


def request(RT, di, proj, **kw):
    return record(RT.detectors[di].surface._desc(), proj, **kw)


def compact_rows(res, count):
    """rows (x, y, w, wl) of a compact hit list, sorted"""
    ph, hw, ext, ill, wl, fill = res
    plen = int(_capi.load_library().ot_hit_piece_len(int(count)))
    cap = _capi.HIT_PIECES * plen
    ph, hw, wl, fill = ph.cpu().numpy(), hw.cpu().numpy(), wl.cpu().numpy(), fill.cpu().numpy()
    rows = [np.column_stack((ph[i * plen:i * plen + f], ph[cap + i * plen:cap + i * plen + f], hw[i * plen:i * plen + f],
                             wl[i * plen:i * plen + f])) for i, f in enumerate(fill) if f]
    rows = np.vstack(rows) if rows else np.zeros((0, 4))
    return rows[np.lexsort(rows.T[::-1])]


BATCH = [("ring", "between", None), ("tilted_steep", "stop", None), ("sphere_neg", "inside", "Equidistant"),
         ("conic_k2", "behind", None), ("tilted", "lateral", None), ("slit", "source", None),
         ("sphere_pos", "stop", "Orthographic"), ("tilted_y", "inside", None)]


@pytest.mark.parametrize("n", [2, 5, 8])
def test_batches_equal_single_requests(n):
    """`ot_detector_hits_multi` with closed-form and numeric detectors in one batch (the numeric instantiation of
    `detector_multi_kernel` then serves them all), dense and compact: every request equals its single call bit for bit."""
    RT, idx = traced("objective")
    N = RT.rays.N
    fx = fixture()
    dets = []
    for kind, place, proj in BATCH[:n]:  # one detector object per request (a kind may stand at one place at a time)
        surf = scenes.detector_kinds(ot)[kind]
        surf.move_to(fx.record(f"objective/{kind}/{place}/{proj}")["pos"])
        dets.append((surf._desc(), proj))
    mk = lambda j, **kw: record(*dets[j], **kw)  # noqa: E731
    single = [_detector.detector_hits_multi(RT.rays, 0, N, [mk(j, want_z=True)])[0] for j in range(n)]
    dense = _detector.detector_hits_multi(RT.rays, 0, N, [mk(j, want_z=True) for j in range(n)])
    compact = _detector.detector_hits_multi(RT.rays, 0, N, [mk(j, compact=True) for j in range(n)])
    wl = RT.rays._dev["wl"][:N].cpu().numpy()
    for j, (kind, place, proj) in enumerate(BATCH[:n]):
        g = fx.record(f"objective/{kind}/{place}/{proj}")
        a, b = single[j], dense[j]
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]), (kind, place)
        assert np.array_equal(a[2], b[2]) and a[3] == b[3] == g["ill"]
        hw = a[1].cpu().numpy()
        sel = hw > 0
        assert np.count_nonzero(sel) == g["w"].shape[0]
        ph = a[0].cpu().numpy().reshape(3, N)
        want = np.column_stack((ph[0][sel], ph[1][sel], hw[sel], wl[sel]))
        want = want[np.lexsort(want.T[::-1])]
        assert np.array_equal(compact_rows(compact[j], N), want), (kind, place, "compact list")
        assert np.array_equal(compact[j][2], a[2]) and compact[j][3] == a[3]


@pytest.mark.parametrize("kind,place", [("tilted_steep", "stop"), ("ring", "between")])
def test_spectrum_through_the_compact_list(kind, place, monkeypatch):
    """detector_spectrum over a compact list of weights and wavelengths against the dense list: the same bins; sums of the
    same at most 440 float32 weights in f64 in another order (1e-12 covers that by far)."""
    RT, di, g = placed(("objective", kind, place, None))
    with ot.global_options.no_warnings():
        monkeypatch.setattr(ot.Raytracer, "COMPACT_HITS_FROM", 1 << 60)
        dense = RT.detector_spectrum(detector_index=di)
        monkeypatch.setattr(ot.Raytracer, "COMPACT_HITS_FROM", 1)
        compact = RT.detector_spectrum(detector_index=di)
    assert np.array_equal(dense._wls, compact._wls)
    assert dense._vals.sum() > 0
    assert_close(compact._vals, dense._vals, rtol=1e-12, atol=1e-12 * dense._vals.max(), what="spectrum")


@pytest.mark.parametrize("kind,place,proj", [("ring", "inside", None), ("conic_hyp", "stop", None),
                                             ("sphere_neg", "between", "Stereographic"), ("tilted_steep", "stop", None)])
@pytest.mark.parametrize("first,count", [(0, 1), (5, 1), (0, 63), (101, 63), (0, 65), (130, 65), (0, 257), (183, 257), (0, None)])
def test_sub_ranges_of_the_rays(kind, place, proj, first, count):
    """Ray counts 1, 63, 65, 257 and all (a lane, a wave less one, a wave and one, a workgroup and one): the hits of a
    sub-range are the same entries of the whole list, its extent is theirs."""
    RT, di, g = placed(("objective", kind, place, proj))
    N = RT.rays.N
    count = N if count is None else count
    whole = _detector.detector_hits_multi(RT.rays, 0, N, [request(RT, di, proj, want_z=True)])[0]
    part = _detector.detector_hits_multi(RT.rays, first, count, [request(RT, di, proj, want_z=True)])[0]
    pw, pp = whole[0].cpu().numpy().reshape(3, N)[:, first:first + count], part[0].cpu().numpy().reshape(3, count)
    assert np.array_equal(pw, pp)
    hw = part[1].cpu().numpy()
    assert np.array_equal(whole[1].cpu().numpy()[first:first + count], hw)
    sel = hw > 0
    if sel.any():
        assert np.array_equal(part[2], [pp[0][sel].min(), pp[0][sel].max(), pp[1][sel].min(), pp[1][sel].max()])
    else:
        assert np.array_equal(part[2], [np.inf, -np.inf, np.inf, -np.inf])
    if count == N:
        assert np.count_nonzero(sel) == g["w"].shape[0] and part[3] == g["ill"]


# ---- rays that died inside the detector's z-range -------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["tilted_steep", "tilted", "conic_k2", "conic_hyp", "sphere_pos", "sphere_neg"])
def test_dead_rays_inside_the_z_range_contribute_nothing(kind):
    """The stop lies inside the detector's z-range: rays it absorbed end there, their later sections have no length (the
    reference normalises those to NaN and drops them by weight).  Every hit must come from a section that carries power: the
    section whose z-span holds the hit, with that section's weight; no NaN; the ill-conditioned count of the fixture."""
    rec = ("objective", kind, "stop", "Orthographic" if kind.startswith("sphere") else None)
    RT, di, g = placed(rec)
    surf = RT.detectors[di].surface
    with ot.global_options.no_warnings():
        ph, hw, wl, ext, ill = host_hits(RT, di, rec[3])
    p, w = RT.rays.p_list, RT.rays.w_list
    z_stop = RT.apertures[0].pos[2]
    assert surf.z_min < z_stop < surf.z_max
    died = (w[:, 2] > 0) & (w[:, 3] == 0)
    assert np.count_nonzero(died) > 20 and np.all(p[died, 3, 2] == p[died, 4, 2]), "rays that ended at the stop"
    assert np.isfinite(ph).all() and np.isfinite(hw).all() and np.isfinite(ext).all()
    assert ill == g["ill"]
    sel = np.nonzero(hw > 0)[0]
    assert sel.size == g["w"].shape[0] and sel.size > 50
    for r in sel:
        # the first section whose end lies at / behind the hit (C_EPS: raytracer.py:985)
        k = int(np.argmax(p[r, 1:, 2] + surf.C_EPS >= ph[r, 2]))
        assert w[r, k] > 0 and hw[r] == w[r, k], f"ray {r}: hit from section {k} with weight {w[r, k]}"
    assert not hw[died & (p[:, 3, 2] < ph[:, 2] - surf.C_EPS)].any(), "no hit behind the place a ray died at"


# ---- device against oracle -------------------------------------------------------------------------------------------
ORACLE_SEEDS = [4000, 4001, 4002, 4003, 4004, 4005, 4006, 4007, 4008, 4009, 4010, 4011, 4012, 4013, 4014, 4015, 4016, 4017, 4018, 4019, 4020, 4021, 4022, 4023]
"""24 random systems none of which collides (a skip here is a failure); the first half runs without HURB, the second with"""


def random_detector(RT, rng):
    """a detector kind, projection and position drawn by `rng`: behind the last surface, between two surfaces, around a
    surface (its plane in the middle of the detector's z-range), in the source plane, displaced"""
    kinds = scenes.detector_kinds(ot)
    kind = [k for k in kinds if k != "tilted_ill"][rng.integers(0, len(kinds) - 1)]
    surf = kinds[kind]
    proj = scenes.SPHERE_PROJECTIONS[rng.integers(0, 4)] if kind.startswith("sphere") else None
    ts = RT.tracing_surfaces
    j = int(rng.integers(0, len(ts) - 1))
    where = ["behind", "between", "around", "source", "lateral"][rng.integers(0, 5)]
    z_last = max(s.z_max for s in ts[:-1])
    lo, hi = surf.z_min - surf.pos[2], surf.z_max - surf.pos[2]
    pos = dict(behind=[0, 0, z_last + 6.0], between=[0, 0, 0.5 * (ts[j].pos[2] + ts[j + 1].pos[2])],
               around=[0, 0, ts[j].pos[2] - 0.5 * (lo + hi) + 1e-3], source=[0, 0, RT.ray_sources[0].pos[2]],
               lateral=[1.7, -0.8, z_last + 6.0])[where]
    return kind, where, proj, surf, pos


@pytest.mark.parametrize("scene_seed", ORACLE_SEEDS)
def test_random_systems_against_the_oracle(scene_seed):
    """3000 rays through a random system, then one detector drawn by the seed: the device's hit search against
    `orc_detector_hits` on the device's own stored sections.  Valid mask and weights bit for bit, both counters, positions
    and extent to 1e-11 (the same operations in another order; the extent is a min / max of those positions)."""
    hurb = ORACLE_SEEDS.index(scene_seed) >= len(ORACLE_SEEDS) // 2
    with ot.global_options.no_warnings():
        RT = scenes.random_scene(ot, scene_seed, seed=scene_seed, use_hurb=hurb)
        kind, where, proj, surf, pos = random_detector(RT, np.random.default_rng(scene_seed + 1))
        RT.add(ot.Detector(surf, pos=[0, 0, RT.outline[5] - 10]))
        RT.trace(3000)
        assert not RT.geometry_error, "the seed list holds systems that do not collide"
        RT.detectors[0].move_to(pos)
        ph, hw, wl, ext, ill = host_hits(RT, 0, proj)  # (a timeout of the numeric search raises here)
    rays = ob.HostRays.from_lists(RT.rays.p_list, RT.rays.w_list, RT.rays.wl_list)
    ph_o, hw_o, ext_o, ill_o, st = ob.detector_hits(rays, 0, rays.N, RT.detectors[0].surface._desc(), _capi.PROJECTIONS[proj])
    print(scene_seed, kind, where, proj, "hits", np.count_nonzero(hw_o > 0), "ill", ill_o)
    assert st == 0
    assert np.array_equal(hw > 0, hw_o > 0), "valid mask"
    assert np.array_equal(hw, hw_o), "weights"
    assert_close(ph, ph_o, rtol=1e-11, atol=1e-11, what="ph")
    assert ill == ill_o
    if np.any(hw_o > 0):
        assert_close(ext, ext_o, rtol=1e-11, atol=1e-11, what="extent")
    else:
        assert np.array_equal(ext, np.repeat(np.asarray(pos[:2], dtype=np.float64), 2))


# ---- render-only chunks ------------------------------------------------------------------------------------------------
class settings:
    def __init__(self, **kw):
        self.kw = kw

    def __enter__(self):
        self.old = {k: getattr(ot.Raytracer, k) for k in self.kw}
        for k, v in self.kw.items():
            setattr(ot.Raytracer, k, v)

    def __exit__(self, *a):
        for k, v in self.old.items():
            setattr(ot.Raytracer, k, v)


def chunked_render(kind, place, proj, render_only):
    """three chunks of 40 000 rays of the objective onto one detector; -> (image, per trace: went to the tail storage?)"""
    with ot.global_options.no_warnings():
        RT = scenes.detector_objective(ot, seed=13)
        surf = scenes.detector_kinds(ot)[kind]
        RT.add(ot.Detector(surf, pos=scenes.detector_position(RT, surf, place)))
        tails = []
        orig = RT.trace
        RT.trace = lambda N, **kw: (tails.append(kw.get("_tail") is not None), orig(N, **kw))[1]
        with settings(ITER_RAYS_STEP=40_000, ITER_RENDER_ONLY=render_only, ITER_EXTENT_RAYS=1 << 60):
            img = RT.iterative_render(120_000, projection_method=proj, extent=[-3., 3., -2.5, 2.5])[0]
        del RT.trace
    return img, tails


@pytest.mark.parametrize("kind", ["ring", "circle", "conic_k2", "conic_hyp", "sphere_pos", "sphere_neg"])
def test_render_only_chunks_equal_the_stored_path(kind):
    """Detectors with a closed-form hit behind the last surface: the chunks of an iterative render go through the tail
    storage (`detector_hit_pair`, `detector_hit_last`) and give the stored path's image (the stored last chunk joins the
    tail after one more float32 rounding of its weights: 1e-7, as in tests/test_gpu_render_only.py)."""
    tail, t_tails = chunked_render(kind, "behind", None, True)
    stored, s_tails = chunked_render(kind, "behind", None, False)
    assert t_tails.count(True) == 2 and not any(s_tails)
    same_image(tail, stored, tol=1e-7)


@pytest.mark.parametrize("kind,place", [("ring", "inside"), ("tilted", "between")])
def test_detectors_in_front_of_the_last_surface_take_the_ray_storage(kind, place):
    """A detector inside the objective needs sections a render-only trace does not keep: every chunk is stored."""
    img, tails = chunked_render(kind, place, None, True)
    stored, _ = chunked_render(kind, place, None, False)
    assert not any(tails)
    same_image(img, stored, tol=1e-11)


def test_numeric_detector_behind_the_last_surface():
    """A tilted detector behind the last surface: the numeric hit search on whatever storage the render picks (the
    two-section tail storage serves it like any other: `detector_hit` with nt = 2) gives the stored path's image."""
    img, tails = chunked_render("tilted", "behind", None, True)
    stored, _ = chunked_render("tilted", "behind", None, False)
    same_image(img, stored, tol=1e-7)
