"""Position and weight of the sections before the last two are written on demand: the tracer's scenes defer them
(`ot_scene_set_deferred_planes`, bit `OT_DEFER_SECTIONS`), a trace that generates its rays on the device stores `p` and `w` of
sections nt - 2 and nt - 1 only, and the first read of `RayStorage._dev["p"]` / `["w"]` -- or of `_rays_struct()` -- repeats the
trace with the stores of the other sections (`ot_rays_fill_sections`).

The yardstick is the storing kernel itself with complete stores (`ot_scene_set_index_store(handle, 1)` clears the whole mask),
read past the hook of `_dev`: the replay runs the same kernel on the same Philox streams, so the planes must be equal bit for
bit, NaN and frozen positions of absorbed rays included -- there is no tolerance.  Detector images are sums of f64 atomics in
no fixed order: same lit pixels, sums to 1e-13 relative.
"""
import ctypes as C

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi

import scenes

gpu = pytest.mark.gpu

COUNTS = (1, 63, 64, 65, 70001)  # one lane, the edges of a wave, 274 workgroups with range borders inside waves
P_SENTINEL, W_SENTINEL = -12345.678, -7.0


def raw(RT, key):
    """The device tensor without the hook of `_dev` (no fill)."""
    return dict.__getitem__(RT.rays._dev, key)


def second_source(RT, **kw):
    """Every scene here has two sources at least, so that a wave straddles a range border."""
    RT.add(ot.RaySource(ot.CircularSurface(r=0.02), divergence="None", s=[0, 0, 1],
                        spectrum=ot.LightSpectrum("Monochromatic", wl=600.), **kw))
    return RT


def one_surface(**kw):
    """nt = 3: one deferred section.  A ring aperture that most rays pass."""
    RT = ot.Raytracer(outline=[-5, 5, -5, 5, -5, 40], **kw)
    RT.add(ot.RaySource(ot.CircularSurface(r=1.5), divergence="Isotropic", div_angle=2, pos=[0, 0, -3],
                        spectrum=ot.LightSpectrum("Monochromatic", wl=550.)))
    second_source(RT, pos=[0.3, 0, -2])
    RT.add(ot.Aperture(ot.RingSurface(r=3, ri=1), pos=[0, 0, 5]))
    RT.add(ot.Detector(ot.RectangularSurface(dim=[8, 8]), pos=[0, 0, 20]))
    return RT


def no_surface(**kw):
    """nt = 2: nothing is deferred, the fill is a no-op."""
    RT = ot.Raytracer(outline=[-5, 5, -5, 5, -5, 40], **kw)
    RT.add(ot.RaySource(ot.CircularSurface(r=1.5), divergence="Isotropic", div_angle=2, pos=[0, 0, -3],
                        spectrum=ot.LightSpectrum("Monochromatic", wl=550.)))
    second_source(RT, pos=[0.3, 0, -2])
    RT.add(ot.Detector(ot.RectangularSurface(dim=[8, 8]), pos=[0, 0, 20]))
    return RT


def clipping(**kw):
    """A diverging source in a narrow outline: rays that miss the lens leave the box on their way (OUTLINE_INTERSECTION)."""
    RT = ot.Raytracer(outline=[-3, 3, -3, 3, -5, 40], **kw)
    RT.add(ot.RaySource(ot.CircularSurface(r=0.5), divergence="Isotropic", div_angle=25, pos=[0, 0, -4],
                        spectrum=ot.LightSpectrum("Monochromatic", wl=550.)))
    second_source(RT, pos=[0.3, 0, -2])
    RT.add(ot.Lens(ot.SphericalSurface(r=1.2, R=18), ot.SphericalSurface(r=1.2, R=-18), de=0.1,
                   n=ot.RefractionIndex("Constant", n=1.5), pos=[0, 0, 12]))
    RT.add(ot.Detector(ot.RectangularSurface(dim=[5.5, 5.5]), pos=[0, 0, 30]))
    return RT


# name -> (builder, index of a detector behind the stack or None)
CASES = {
    "double_gauss": (lambda: scenes.double_gauss(ot, seed=5), 0),                            # level 0, lines: the bench kernel
    "mixed_geometry": (lambda: scenes.mixed_geometry(ot, seed=6), None),                     # filter, ideal lens, tabulated media
    "double_gauss_aspheric": (lambda: scenes.double_gauss(ot, aspheric=True, seed=7), 0),
    "hurb_slit_lens": (lambda: second_source(scenes.hurb_slit_lens(ot, seed=8), pos=[0, 0.5, -3]), 0),   # Philox HURB deviates
    "freeform": (lambda: second_source(scenes.freeform_scene(ot, seed=9), pos=[0.5, 0, 1]), 1),          # spline level
    "double_gauss_no_pol": (lambda: scenes.double_gauss(ot, seed=10, no_pol=True), 0),
    "one_surface": (lambda: one_surface(seed=11), 0),
    "no_surface": (lambda: no_surface(seed=12), 0),
}


def traced(make, N: int, complete: bool, timing: bool = False):
    """A seeded tracer after two traces of N rays: the first compiles the scene, then `p` and `w` get a sentinel and the second,
    which repeats the first ray for ray, writes over it what it writes.  `complete`: with the scene's mask cleared."""
    lib = _capi.load_library()
    with ot.global_options.no_warnings():
        RT = make()
        RT.trace(N)
        if complete:
            _capi.check(lib.ot_scene_set_index_store(RT._scene_handle, 1))
        if timing:
            _capi.check(lib.ot_scene_set_timing(RT._scene_handle, 1))
        raw(RT, "p").fill_(P_SENTINEL)
        raw(RT, "w").fill_(W_SENTINEL)
        RT.trace(N)
    return RT


def host_planes(RT, N: int) -> dict:
    """p (3, nt, N), w (nt, N), s (3, N), wl (N) as they lie in the buffers: past the hook, no fill."""
    r = RT.rays
    Np, nt = r._Np, r._nt
    return {"p": raw(RT, "p").view(3, nt, Np)[..., :N].cpu().numpy(), "w": raw(RT, "w").view(nt, Np)[:, :N].cpu().numpy(),
            "s": r._dev["s"].view(3, Np)[:, :N].cpu().numpy(), "wl": r._dev["wl"][:N].cpu().numpy()}


_complete = {}


def complete_run(name: str, N: int):
    """(planes, counters, tracer) of the complete-store trace of a case: computed once, shared, left unchanged."""
    if (name, N) not in _complete:
        RT = traced(CASES[name][0], N, True)
        _complete[name, N] = (host_planes(RT, N), RT._msgs.copy(), RT)
    return _complete[name, N]


def bits(a: np.ndarray) -> np.ndarray:
    return a.view(np.uint64 if a.dtype == np.float64 else np.uint32)


def last_trace_ms(RT) -> float:
    ms = C.c_double()
    _capi.check(_capi.load_library().ot_scene_last_trace_ms(RT._scene_handle, C.byref(ms)))
    return ms.value


def image_of(RT, **kw) -> np.ndarray:
    with ot.global_options.no_warnings():
        img = RT.detector_image(**kw)
    return np.array(img._data, dtype=np.float64), np.array(img.extent, dtype=np.float64)


def assert_images_equal(got, ref, need_light: bool = True) -> None:
    (a, ea), (b, eb) = got, ref
    assert np.array_equal(ea, eb), "the automatic extents differ"
    assert a.shape == b.shape and np.array_equal(a != 0, b != 0), "other pixels are lit"
    assert b.any() or not need_light, "no ray reached the detector: the case shows nothing"
    assert np.abs(a - b).max() <= 1e-13 * np.abs(b).max()


@gpu
@pytest.mark.parametrize("N", COUNTS)
@pytest.mark.parametrize("name", list(CASES))
def test_deferred_sections_are_left_out_and_replayed_bit_for_bit(name, N):
    make, behind = CASES[name]
    ref, ref_msgs, ST = complete_run(name, N)
    nt = ST.rays._nt
    assert not (ref["p"] == P_SENTINEL).any() and not (ref["w"] == W_SENTINEL).any(), "the yardstick stored every entry"
    RT = traced(make, N, False, timing=True)
    r = RT.rays
    assert r._nt == nt and len(r.N_list) >= 2
    assert (r._sections_stale is not None) == (nt >= 3)
    if N == COUNTS[-1]:  # some source range starts in the middle of a wave
        assert any(int(q.first) % 64 for q in r._source_ranges())

    # before any fill: the last two sections, s, wl and the counters are the complete trace's; the rest is untouched
    got = host_planes(RT, N)
    k = max(nt - 2, 0)
    for key in ("s", "wl"):
        assert np.array_equal(bits(got[key]), bits(ref[key])), key
    assert np.array_equal(bits(got["p"][:, k:]), bits(ref["p"][:, k:]))
    assert np.array_equal(bits(got["w"][k:]), bits(ref["w"][k:]))
    assert np.array_equal(RT._msgs, ref_msgs)
    assert (got["p"][:, :k] == P_SENTINEL).all() and (got["w"][:k] == W_SENTINEL).all(), "the trace stored a deferred section"

    # a detector behind the stack is served from the last two sections: same image, no fill
    if behind is not None:
        # (a single ray may well be vignetted; from a wave on some ray reaches every one of these detectors)
        assert_images_equal(image_of(RT, detector_index=behind), image_of(ST, detector_index=behind), need_light=N > 1)
        # (unless a ray was clipped at the outline, where the HURB scene bends some: then the rule asks for the fill)
        clipped = bool(RT._msgs[RT.INFOS.OUTLINE_INTERSECTION].any())
        assert not clipped or name not in ("double_gauss", "double_gauss_no_pol", "one_surface")
        assert (r._sections_stale is not None) == (nt >= 3 and not clipped), "the detector stage did not follow its rule"
        assert clipped or (host_planes(RT, N)["p"][:, :k] == P_SENTINEL).all()

    # the first read through the hook completes the storage; counters, slot tables and the trace's timing do not notice
    msgs, ms = RT._msgs.copy(), last_trace_ms(RT)
    assert ms > 0
    r._dev["p"]
    assert r._sections_stale is None
    got = host_planes(RT, N)
    for key in ("p", "w", "s", "wl"):
        a, b = got[key], ref[key]
        assert np.array_equal(bits(a), bits(b)), \
            f"plane {key} differs in {np.count_nonzero(bits(a) != bits(b))} entries after the fill"
    assert np.isnan(got["p"]).sum() == np.isnan(ref["p"]).sum()
    assert np.array_equal(RT._msgs, msgs) and last_trace_ms(RT) == ms
    with ot.global_options.no_warnings():
        RT.trace(N)  # counters the fill had left in the scene's slot tables would be added to this trace's
    assert np.array_equal(RT._msgs, msgs)


@gpu
def test_absorbed_and_reflected_rays_replay_their_frozen_and_nan_positions():
    """Total internal reflection and rays that miss a surface: the cases the bit-for-bit claim is about."""
    def tir(**kw):
        RT = ot.Raytracer(outline=[-6, 6, -6, 6, -5, 40], **kw)
        RT.add(ot.RaySource(ot.CircularSurface(r=3.4), divergence="None", s=[0, 0, 1], pos=[0, 0, -3],
                            spectrum=ot.LightSpectrum("Monochromatic", wl=550.), polarization="x"))
        second_source(RT, pos=[0.3, 0, -2])
        RT.add(ot.Lens(ot.CircularSurface(r=3), ot.SphericalSurface(r=2.9, R=-3), de=0.2, pos=[0, 0, 2],
                       n=ot.RefractionIndex("Constant", n=1.8)))
        RT.add(ot.Lens(ot.SphericalSurface(r=4, R=20), ot.SphericalSurface(r=4, R=-20), de=0.2, pos=[0, 0, 15],
                       n=ot.RefractionIndex("Constant", n=1.5)))
        return RT

    N = 4097
    ST = traced(lambda: tir(seed=12), N, True)
    ref = host_planes(ST, N)
    assert ST._msgs[ST.INFOS.TIR].sum() > 0 and ST._msgs[ST.INFOS.ABSORB_MISSING].sum() > 0
    RT = traced(lambda: tir(seed=12), N, False)
    RT.rays._dev["w"]
    got = host_planes(RT, N)
    assert np.array_equal(bits(got["p"]), bits(ref["p"])) and np.array_equal(bits(got["w"]), bits(ref["w"]))
    dead = ref["w"][-2] == 0
    assert dead.any() and (ref["p"][:, 1:-1, dead] == ref["p"][:, 2:, dead]).any(), "no ray rests where it was absorbed"


@gpu
def test_detector_inside_the_stack_fills_first():
    N = COUNTS[-1]
    make = lambda: scenes.double_gauss(ot, seed=21)
    ST, RT = traced(make, N, True), traced(make, N, False)
    z = float(RT.lenses[3].front.pos[2]) - 5.0  # between the stop and the fourth lens
    for T in (ST, RT):
        T.detectors[0].move_to([0, 0, z])
    assert RT.rays._sections_stale is not None
    assert_images_equal(image_of(RT), image_of(ST))
    assert RT.rays._sections_stale is None, "early sections were read unfilled"


@gpu
def test_clipped_rays_fill_first():
    N = COUNTS[-1]
    ST, RT = traced(lambda: clipping(seed=22), N, True), traced(lambda: clipping(seed=22), N, False)
    assert RT._msgs[RT.INFOS.OUTLINE_INTERSECTION].sum() > 0
    assert RT.rays._sections_stale is not None and RT.rays._tail_z is None
    assert_images_equal(image_of(RT), image_of(ST))
    assert RT.rays._sections_stale is None
    assert_images_equal(image_of(RT, extent=[-2, 2, -2, 2]), image_of(ST, extent=[-2, 2, -2, 2]))


@gpu
def test_a_second_trace_replaces_the_mark():
    N = 1000
    ref2 = host_planes(traced(lambda: scenes.double_gauss(ot, seed=32), N, True), N)
    RT = traced(lambda: scenes.double_gauss(ot, seed=31), N, False)
    RT.seed = 32
    with ot.global_options.no_warnings():
        RT.trace(N)
    assert RT.rays._sections_stale is not None
    RT.rays._dev["p"]
    got = host_planes(RT, N)
    assert np.array_equal(bits(got["p"]), bits(ref2["p"])) and np.array_equal(bits(got["w"]), bits(ref2["w"]))


@gpu
def test_the_fill_uses_the_scene_that_traced_the_rays():
    N = 1000
    make = lambda: scenes.double_gauss(ot, seed=33)
    ref = host_planes(traced(make, N, True), N)
    RT = traced(make, N, False)
    RT.lenses[0].n = ot.RefractionIndex("Constant", n=1.31)
    with ot.global_options.no_warnings():
        RT._compile(RT._geometry_key())  # the tracer lets go of the scene that traced; the storage keeps it
    assert RT.rays._sections_stale is not None and RT.rays._sections_stale[0] is not RT._scene_ref
    RT.rays._dev["p"]
    got = host_planes(RT, N)
    assert np.array_equal(bits(got["p"]), bits(ref["p"])) and np.array_equal(bits(got["w"]), bits(ref["w"]))


class _Counted:
    """Wraps the `ot_rays_fill_sections` binding of the loaded library and counts its calls."""

    def __init__(self, monkeypatch):
        lib = _capi.load_library()
        self.calls, inner = 0, lib.ot_rays_fill_sections

        def wrapper(*a):
            self.calls += 1
            return inner(*a)
        monkeypatch.setattr(lib, "ot_rays_fill_sections", wrapper)


@gpu
def test_set_initial_rays_never_launches_a_fill(monkeypatch):
    N = 500
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=34)
        RT.trace(N)
        assert RT.rays._sections_stale is not None
        p0, w0, wl = RT.rays.p_list[:, 0].copy(), RT.rays.w_list[:, 0].copy(), RT.rays.wl_list.copy()
        pol0 = RT.rays.pol_list[:, 0].copy()
        d = RT.rays.p_list[:, 1] - p0
        s0 = d / np.linalg.norm(d, axis=1)[:, None]
        N_list = RT.rays.N_list.copy()
        RT.trace(N)  # same shape: the buffers are kept and carry a mark again
        assert RT.rays._sections_stale is not None
        counted = _Counted(monkeypatch)
        RT.trace(N, _initial_rays=(p0, s0, pol0, w0, wl), _N_list=N_list)
    assert counted.calls == 0 and RT.rays._sections_stale is None
    assert np.isfinite(RT.rays.p_list[RT.rays.w_list[:, -2] > 0]).all() and counted.calls == 0


@gpu
def test_accessors_return_filled_data():
    N = 1000
    make = lambda: scenes.double_gauss(ot, seed=35)
    ref = host_planes(traced(make, N, True), N)
    p_ref, w_ref = ref["p"].transpose(2, 1, 0), ref["w"].T  # (N, nt, 3), (N, nt)
    A = traced(make, N, False)
    assert np.array_equal(bits(np.ascontiguousarray(A.rays.p_list)), bits(np.ascontiguousarray(p_ref)))
    assert A.rays._sections_stale is None
    B = traced(make, N, False)
    assert np.array_equal(bits(np.ascontiguousarray(B.rays.w_list)), bits(np.ascontiguousarray(w_ref)))
    assert B.rays._sections_stale is None
    S = traced(make, N, False)
    ind = np.arange(0, N, 7)
    got = S.rays._select("p", ind, slice(None))
    assert S.rays._sections_stale is None and "p" not in S.rays._host
    assert np.array_equal(bits(np.ascontiguousarray(got)), bits(np.ascontiguousarray(p_ref[ind])))


@gpu
def test_sections_and_polarisation_fill_independently():
    N = 1000
    make = lambda: scenes.double_gauss(ot, seed=36)
    ST = traced(make, N, True)
    ref = host_planes(ST, N)
    pol_ref = raw(ST, "pol").view(3, ST.rays._nt, ST.rays._Np)[..., :N].cpu().numpy().transpose(2, 1, 0)
    n_ref = raw(ST, "n").view(ST.rays._nt, ST.rays._Np)[:, :N].cpu().numpy().T
    for first in ("pol", "p"):
        RT = traced(make, N, False)
        r = RT.rays
        assert r._sections_stale is not None and r._pol_stale is not None and r._n_stale
        if first == "pol":
            pol, n = r.pol_list, r.n_list
            assert r._sections_stale is not None and r._pol_stale is None, "the polarisation fill is its own"
            assert (host_planes(RT, N)["p"][:, :-2] == P_SENTINEL).all()
            r._dev["p"]
        else:
            r._dev["p"]
            assert r._sections_stale is None and r._pol_stale is not None, "the sections fill is its own"
            pol, n = r.pol_list, r.n_list
        assert np.array_equal(pol, pol_ref, equal_nan=True) and np.array_equal(n, n_ref)
        got = host_planes(RT, N)
        assert np.array_equal(bits(got["p"]), bits(ref["p"])) and np.array_equal(bits(got["w"]), bits(ref["w"]))


@gpu
def test_back_to_back_traces_launch_no_fill(monkeypatch):
    """`init()` asks the kept buffers for their device past the hook: otherwise every trace would repeat the one before."""
    counted = _Counted(monkeypatch)
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=37)
        for _ in range(30):
            RT.trace(1000)
        img = RT.detector_image()
    assert counted.calls == 0 and RT.rays._sections_stale is not None and img.power() > 0
    RT.rays._dev["p"]
    assert counted.calls == 1
    RT.rays._dev["w"], RT.rays._rays_struct()
    assert counted.calls == 1


@gpu
def test_the_mark_holds_scene_table_and_ranges():
    import gc
    import weakref
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=38)
        RT.trace(1000)
    rays = RT.rays
    scene, table, ranges, seed, count = rays._sections_stale
    refs = weakref.ref(scene), weakref.ref(table)
    assert count == 1000 and len(ranges) >= 5
    del scene, table, ranges
    RT._release_scene()
    RT._source_cache = RT._record = None
    rays.__dict__["_pol_stale"], rays.__dict__["_n_scene"] = None, None
    gc.collect()
    assert all(r() is not None for r in refs), "the mark must keep what its fill needs"
    rays._dev["p"]
    gc.collect()
    assert rays._sections_stale is None and all(r() is None for r in refs), "a filled storage lets go"


@gpu
def test_mismatched_arguments_are_refused():
    lib = _capi.load_library()
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=39)
        RT.trace(1000)
    scene, tab, rng, seed, count = RT.rays._sections_stale
    rays = RT.rays._rays_struct(tail_only=True)

    def call(r, first=0, n=count):
        return lib.ot_rays_fill_sections(scene.handle, tab.handle, rng, len(rng), seed, C.byref(r), first, n, None)

    def variant(**kw):
        r = _capi.Rays()
        C.memmove(C.byref(r), C.byref(rays), C.sizeof(r))
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    for bad, word in ((variant(p=None), b"needs p, w"), (variant(w=None), b"needs p, w"), (variant(nt=rays.nt - 1), b"sections")):
        assert call(bad) == -1 and b"ot_rays_fill_sections" in lib.ot_last_error() and word in lib.ot_last_error()
    for first, n in ((-1, 1), (0, rays.N + 1), (rays.N, 1)):
        assert call(rays, first, n) == -1 and b"ot_rays_fill_sections: range outside the storage" in lib.ot_last_error()
    assert RT.rays._sections_stale is not None  # nothing above went through the storage
    # the bit through the C-ABI: every mask of the three bits is taken, a fourth bit is not, and "complete storage" clears all
    for mask in range(8):
        assert lib.ot_scene_set_deferred_planes(scene.handle, mask) == 0
    assert lib.ot_scene_set_deferred_planes(scene.handle, 8) == -1 and b"unknown bit" in lib.ot_last_error()
    assert lib.ot_scene_set_deferred_planes(scene.handle, _capi.OT_DEFER_SECTIONS) == 0
    raw(RT, "p").fill_(P_SENTINEL)
    with ot.global_options.no_warnings():
        RT.trace(1000)
    assert (host_planes(RT, 1000)["p"][:, :-2] == P_SENTINEL).all(), "OT_DEFER_SECTIONS alone defers the sections"
    assert lib.ot_scene_set_deferred_planes(scene.handle, 7) == 0 and lib.ot_scene_set_index_store(scene.handle, 1) == 0
    with ot.global_options.no_warnings():
        RT.trace(1000)
    assert not (host_planes(RT, 1000)["p"] == P_SENTINEL).any(), "ot_scene_set_index_store(handle, 1) is complete storage"
