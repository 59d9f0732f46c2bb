"""The step loop of the trace kernels after two changes to how it is compiled, neither of which may move a bit: the plane
bases of the section stores are formed where a store happens (no running bases), and the head of a step's hot record is read
as one group at the top of the step.  (The cases also cover lanes whose hit point is replaced next to lanes that go on to the
normal, which is where a hand-over from the hit search to the normal would show.)

Yardstick of every case: the same scene with every step compiled as OT_HOT_OTHER (`ot_scene_set_hot_steps(handle, 0)`: hit
search and normal read the surface records) and complete storage (`ot_scene_set_index_store(handle,
1)`: every plane of every section written by the one launch).  Every plane -- p, s, w, n, pol, wl -- and the counters are
compared bit for bit; there is no tolerance.  Handed-in rays are compared with the C oracle as well, with the bars of
tests/test_gpu_hot_step.py.

Every buffer is filled with a sentinel before the launch that is looked at: a plane (or a section, or the padding behind
the last ray) that a store mode does not write must still hold it afterwards, and what the mode writes must not.  A plane
base formed wrongly shows up as a sentinel overwritten or a plane left unwritten.
"""
import ctypes as C

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd._device import stream_ptr
from optrace_amd.ray_storage import RayStorage, TailStorage
from optrace_amd.scene import CompiledScene

import oracle_bridge as ob
import scenes
from helpers import assert_close

pytestmark = pytest.mark.gpu

COUNTS = (1, 63, 65, 1000, 70001)  # one lane, either side of a wave, four workgroups, 274 workgroups with a partial last wave
SENTINEL = {"p": -12345.678, "w": -7.0, "n": -3.25, "pol": -9.5, "s": -2.125, "wl": -11.0}
LINES = dict(lines=[486.1327, 587.5618, 656.272], line_vals=[1., 2., 1.])
COMPLETE, DEFERRED = "complete", "deferred"


# ---- scenes: the smallest in which the loop can go wrong ---------------------------------------------------------------------
def small(name: str, **rt_args):
    RT = ot.Raytracer(outline=[-6, 6, -6, 6, -12, 40], **rt_args)
    RT.add(ot.RaySource(ot.CircularSurface(r=2.8), divergence="Isotropic", div_angle=4, pos=[0.1, -0.05, -10],
                        spectrum=ot.LightSpectrum("Lines", **LINES), polarization="Uniform"))
    RT.add(ot.RaySource(ot.CircularSurface(r=0.02), divergence="None", s=[0, 0, 1], pos=[0.3, 0, -8],
                        spectrum=ot.LightSpectrum("Lines", **LINES)))  # (a second range: its border lies inside a wave)
    glass = ot.RefractionIndex("Abbe", n=1.62, V=36.)
    sph, disc = ot.SphericalSurface, ot.CircularSurface
    if name == "one_step":  # nt = 3: the step in front of the tracer's end aperture; its neighbour's record is the last one
        RT.add(ot.Aperture(ot.RingSurface(r=3., ri=1.9), pos=[0.2, 0.1, 3]))
    elif name == "two_steps":  # a decentred lens: px, py != 0 in the head of the record
        RT.add(ot.Lens(sph(r=2.5, R=7.), sph(r=2.5, R=-9.), de=0.2, pos=[0.45, -0.35, 0], n=glass))
    elif name == "plates_ring":  # disc and ring forms
        RT.add(ot.Lens(disc(r=2.2), disc(r=2.2), de=0.5, pos=[0, 0, 0], n=glass))
        RT.add(ot.Aperture(ot.RingSurface(r=3., ri=1.5), pos=[0.2, 0.1, 3]))
        RT.add(ot.Lens(disc(r=2.4), disc(r=2.4), de=0.4, pos=[0, 0, 5], n=glass))
    elif name == "three_forms":  # plain sphere, flat sphere (|R| > 4096), conic
        RT.add(ot.Lens(sph(r=2.5, R=20.), sph(r=2.5, R=-5000.), de=0.3, pos=[0, 0, 0], n=glass))
        RT.add(ot.Lens(ot.ConicSurface(r=2.5, R=8., k=-0.6), ot.ConicSurface(r=2.5, R=-10., k=-2.5), de=0.1, pos=[0, 0, 6],
                       n=ot.RefractionIndex("Cauchy", coeff=[1.49, 0.00354, 0, 0])))
    else:
        raise KeyError(name)
    return RT


def gauss(spectrum: str, **rt_args):
    if spectrum == "lines":
        return scenes.double_gauss(ot, **rt_args)
    RT = scenes.double_gauss(ot, spectrum=ot.LightSpectrum("Gaussian", mu=550., sig=40.), **rt_args)
    if spectrum == "tables":  # a tabulated medium: the kernels with per-lane loads in the loop
        RT.lenses[2].n = ot.RefractionIndex("Data", wls=np.linspace(380., 780., 41), vals=1.6 + 0.1 * np.exp(-np.linspace(0, 3, 41)))
    return RT


SCENES = {
    "one_step": lambda: small("one_step", seed=3),
    "two_steps": lambda: small("two_steps", seed=4),
    "plates_ring": lambda: small("plates_ring", seed=5),
    "three_forms": lambda: small("three_forms", seed=6),
    "gauss_lines": lambda: gauss("lines", seed=7),
    "gauss_lines_no_pol": lambda: gauss("lines", seed=7, no_pol=True),
    "gauss_formulas": lambda: gauss("formulas", seed=8),
    "gauss_formulas_no_pol": lambda: gauss("formulas", seed=8, no_pol=True),
    "gauss_tables": lambda: gauss("tables", seed=9),
    "gauss_tables_no_pol": lambda: gauss("tables", seed=9, no_pol=True),
}


# ---- launches behind a sentinel ------------------------------------------------------------------------------------------------
def raw(RT, key):
    """The device tensor without the hook of `_dev` (no fill)."""
    return dict.__getitem__(RT.rays._dev, key)


def keys_of(RT) -> tuple:
    return ("p", "w", "n", "s", "wl") + (() if RT.no_pol else ("pol",))


def paint(RT, keys) -> None:
    for k in keys:
        raw(RT, k).fill_(SENTINEL[k])


def planes(RT, N: int) -> dict:
    """p, pol (3, nt, N), w, n (nt, N), s (3, N), wl (N) as they lie in the buffers, past the hook; `pad`: everything behind
    ray N - 1 of every plane; the counters."""
    r = RT.rays
    Np, nt = r._Np, r._nt
    shape = {"p": (3, nt, Np), "pol": (3, nt, Np), "w": (nt, Np), "n": (nt, Np), "s": (3, Np), "wl": (Np,)}
    out, pad = {}, {}
    for k in keys_of(RT):
        a = raw(RT, k).view(*shape[k]).cpu().numpy()
        out[k], pad[k] = np.ascontiguousarray(a[..., :N]), a[..., N:]
    out["msgs"] = RT._msgs.copy()
    return out, pad


def bits(a: np.ndarray) -> np.ndarray:
    return a.view({8: np.uint64, 4: np.uint32}[a.dtype.itemsize])


def assert_bits(got: dict, ref: dict, what: str, keys=None) -> None:
    for k in keys or ref.keys():
        a, b = got[k], ref[k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{what}: {k}"
        assert np.array_equal(bits(a), bits(b)), f"{what}: {k} differs in {np.count_nonzero(bits(a) != bits(b))} of {a.size} entries"


def untouched(a: np.ndarray, key: str) -> bool:
    return bool((a == SENTINEL[key]).all())


def written(a: np.ndarray, key: str) -> bool:
    return not (a == SENTINEL[key]).any()


def switches(RT, mode: str, hot: int) -> None:
    lib = _capi.load_library()
    if mode == COMPLETE:
        _capi.check(lib.ot_scene_set_index_store(RT._scene_handle, 1))
    _capi.check(lib.ot_scene_set_hot_steps(RT._scene_handle, hot))


def generated(make, N: int, mode: str, hot: int):
    """A seeded tracer after two traces of N rays: the first compiles the scene and allocates, then the switches are set, every
    buffer is painted, and the second -- ray for ray the first -- writes what its store mode writes."""
    with ot.global_options.no_warnings():
        RT = make()
        RT.trace(N)
        assert not RT.geometry_error
        switches(RT, mode, hot)
        paint(RT, keys_of(RT))
        RT.trace(N)
    return RT


_yardstick = {}


def yardstick(name: str, N: int) -> dict:
    """The planes of (scene, N) with every step on the surface records and complete stores: computed once, shared, unchanged."""
    if (name, N) not in _yardstick:
        RT = generated(SCENES[name], N, COMPLETE, 0)
        ref, pad = planes(RT, N)
        for k in keys_of(RT):
            assert written(ref[k], k), f"the yardstick left {k} unwritten"
            assert untouched(pad[k], k)
        for a in ref.values():
            a.flags.writeable = False
        _yardstick[name, N] = ref
    return _yardstick[name, N]


def check_complete_and_deferred(name: str, N: int) -> None:
    ref = yardstick(name, N)
    nt = ref["w"].shape[0]

    # everything stored by the one launch
    RT = generated(SCENES[name], N, COMPLETE, 1)
    got, pad = planes(RT, N)
    assert_bits(got, ref, f"{name}, {N} rays, complete stores")
    assert all(untouched(pad[k], k) for k in pad)

    # the tracer's own mode: p and w of the last two sections, s, wl, the counters; then the three fills, one after the other
    RT = generated(SCENES[name], N, DEFERRED, 1)
    r = RT.rays
    got, pad = planes(RT, N)
    k0 = nt - 2
    assert_bits(got, ref, "deferred trace", keys=("s", "wl", "msgs"))
    assert np.array_equal(bits(got["p"][:, k0:]), bits(ref["p"][:, k0:])) and np.array_equal(bits(got["w"][k0:]), bits(ref["w"][k0:]))
    assert untouched(got["p"][:, :k0], "p") and untouched(got["w"][:k0], "w"), "the trace stored a deferred section"
    assert untouched(got["n"], "n") and (RT.no_pol or untouched(got["pol"], "pol")), "the trace stored a deferred plane"
    r._dev["p"]  # ot_rays_fill_sections
    got, pad = planes(RT, N)
    assert_bits(got, ref, "after the section fill", keys=("p", "w", "s", "wl"))
    assert untouched(got["n"], "n") and (RT.no_pol or untouched(got["pol"], "pol")), "the section fill wrote another plane"
    if not RT.no_pol:
        r._dev["pol"]  # ot_rays_fill_pol
        got, pad = planes(RT, N)
        assert_bits(got, ref, "after the polarisation fill", keys=("p", "w", "s", "wl", "pol"))
        assert untouched(got["n"], "n"), "the polarisation fill wrote the index plane"
    r._dev["n"]  # ot_rays_fill_index
    got, pad = planes(RT, N)
    assert_bits(got, ref, f"{name}, {N} rays, deferred trace and its fills")
    assert all(untouched(pad[k], k) for k in pad)
    _capi.check(_capi.load_library().ot_scene_set_hot_steps(RT._scene_handle, 1))


@pytest.mark.parametrize("N", COUNTS)
@pytest.mark.parametrize("name", list(SCENES))
def test_stored_planes_equal_the_surface_record_path_bit_for_bit(name, N):
    check_complete_and_deferred(name, N)
    w = yardstick(name, N)["w"]
    if N >= 1000:
        assert (w[-2] > 0).any(), "no ray reaches the last section: the case shows nothing"


# ---- handed-in rays and render-only chunks -------------------------------------------------------------------------------------
def initial_rays(ref: dict) -> tuple:
    """Section 0 of a traced storage as the rays to hand in."""
    p0, p1 = ref["p"][:, 0].T, ref["p"][:, 1].T
    d = p1 - p0
    s0 = d / np.linalg.norm(d, axis=1)[:, None]
    return p0.copy(), s0, ref["pol"][:, 0].T.copy(), ref["w"][0].copy(), ref["wl"].copy()


def handed_in(make, init: tuple, hot: int):
    """(planes, padding, tracer) of `ot_trace` on rays handed in, with the tracer's deferral mask: such a launch stores every
    section of p, w and pol, and leaves the index plane alone."""
    N = len(init[3])
    with ot.global_options.no_warnings():
        RT = make()
        RT.trace(N, _initial_rays=init)
        switches(RT, DEFERRED, hot)
        paint(RT, keys_of(RT))
        RT.trace(N, _initial_rays=init)
    got, pad = planes(RT, N)
    return got, pad, RT


def check_handed_in(make, init: tuple, what: str) -> dict:
    on, pad, RT = handed_in(make, init, 1)
    off, _, _ = handed_in(make, init, 0)
    assert_bits(on, off, what)
    for k in ("p", "w", "pol", "s", "wl"):
        assert written(on[k], k), f"{what}: {k} has entries the launch did not write"
    assert untouched(on["n"], "n"), "the index plane is deferred for rays handed in as well"
    RT.rays._dev["n"]
    filled, _ = planes(RT, len(init[3]))
    assert written(filled["n"], "n") and np.array_equal(bits(filled["p"]), bits(on["p"]))
    # the C oracle on the same rays
    sc = CompiledScene(RT)
    host = ob.HostRays(len(init[3]), sc.nt, False)
    host.set_initial(*init)
    msgs, st = ob.trace(sc.desc, host, None)
    assert st == 0
    assert np.array_equal(msgs, on["msgs"]), f"counters differ:\n{msgs}\n{on['msgs']}"
    assert np.array_equal(host.w_list > 0, on["w"].T > 0), "alive masks per section must be bit-exact"
    assert_close(on["p"].transpose(2, 1, 0), host.p_list, rtol=1e-11, atol=1e-11, what="p_list")
    assert_close(on["w"].T, host.w_list, rtol=1e-6, atol=1e-15, what="w_list")
    return on


def tail_records(RT, N: int) -> np.ndarray:
    """The records of a render-only chunk, sorted: start and end of the last section, its weight, the wavelength."""
    tail = TailStorage()
    RT.trace(N, _tail=tail)
    cap, n = tail._cap, tail.N
    p = tail._dev["p"].view(3, 2, cap)[:, :, :n].cpu().numpy()
    tw = tail._dev["w"].view(2, cap)[:, :n].cpu().numpy()
    twl = tail._dev["wl"][:n].cpu().numpy()
    live = tw[0] > 0
    assert int(live.sum()) == tail.alive
    a = np.concatenate([p[:, 0, live].T, p[:, 1, live].T, tw[0, live, None].astype(np.float64),
                        twl[live, None].astype(np.float64)], axis=1)
    return a[np.lexsort(a.T[::-1])]


@pytest.mark.parametrize("name", ["gauss_lines", "one_step"])
def test_handed_in_rays_and_render_only_chunks(name):
    N = 1000
    ref = yardstick(name, N)
    check_handed_in(SCENES[name], initial_rays(ref), f"{name}, rays handed in")

    # a render-only chunk stores no section: the living rays' last section, which is the stored trace's
    nt = ref["w"].shape[0]
    live = ref["w"][nt - 2] > 0
    assert live.any()
    want = np.concatenate([ref["p"][:, nt - 2, live].T, ref["p"][:, nt - 1, live].T,
                           ref["w"][nt - 2, live, None].astype(np.float64), ref["wl"][live, None].astype(np.float64)], axis=1)
    want = want[np.lexsort(want.T[::-1])]
    with ot.global_options.no_warnings():
        RT = SCENES[name]()
        RT.trace(N)
        before, _ = planes(RT, N)
        for hot in (1, 0):
            _capi.check(_capi.load_library().ot_scene_set_hot_steps(RT._scene_handle, hot))
            got = tail_records(RT, N)
            assert got.shape == want.shape and np.array_equal(bits(got), bits(want)), f"render-only chunk, hot steps {hot}"
        _capi.check(_capi.load_library().ot_scene_set_hot_steps(RT._scene_handle, 1))
    after, _ = planes(RT, N)
    assert_bits(after, before, "a render-only chunk wrote into the ray storage")


@pytest.mark.parametrize("name", ["three_forms", "gauss_lines"])
def test_rays_that_miss_and_rays_behind_a_surface_sit_next_to_rays_that_hit(name):
    """Lanes whose hit point is replaced (no hit, a start behind the surface) beside lanes that go on to the normal: a bundle
    wider than the lenses, every fifth ray started behind the first vertex, every seventh behind the third
    surface, every eighth without power."""
    N = 1000
    with ot.global_options.no_warnings():
        RT = SCENES[name]()
    first, third = RT.lenses[0].front, RT.lenses[1].front
    r_lens, z0 = float(first.r), float(first.pos[2])
    rng = np.random.default_rng(11)
    rr, ph = 1.25 * r_lens * np.sqrt(rng.uniform(0, 1, N)), rng.uniform(0, 2 * np.pi, N)
    p0 = np.stack([rr * np.cos(ph), rr * np.sin(ph), np.full(N, z0 - 5.)], axis=1)
    p0[::5, 2] = float(first.z_max) + 0.01  # (inside the first lens: behind its front, z > z_max)
    p0[::7, 2] = float(third.z_max) + 0.01
    cone = 10 if name == "three_forms" else 2  # degrees: wide enough that rays which hit the first lens miss the second
    th, a = np.radians(cone) * np.sqrt(rng.uniform(0, 1, N)), rng.uniform(0, 2 * np.pi, N)
    s0 = np.stack([np.sin(th) * np.cos(a), np.sin(th) * np.sin(a), np.cos(th)], axis=1)
    pol = np.cross(s0, [0., 1., 0.])
    pol /= np.linalg.norm(pol, axis=1)[:, None]
    w0 = np.ones(N, dtype=np.float32)
    w0[3::8] = 0
    wl = rng.choice(np.array(LINES["lines"] if name == "three_forms" else [486.1327, 589.2938, 656.272], dtype=np.float32), N)
    on = check_handed_in(SCENES[name], (p0, s0, pol, w0, wl), f"{name}, wide bundle")
    w = on["w"]
    lit = w0 > 0
    assert (w[1, lit] == 0).any() and (w[1, lit] > 0).any(), "some rays miss the first surface, some hit it"
    assert (w[3] > 0).any() and (w[-2] > 0).any(), "rays of the wave go on through the later lenses"
    assert ((w[2] > 0) & (w[3] == 0)).any(), "no ray is lost at the second lens"
    assert on["msgs"].sum() > 0


# ---- a plane stride that is not the ray count ----------------------------------------------------------------------------------
def test_padded_plane_stride_equals_the_packed_layout(monkeypatch):
    """Just above 2^20 rays the planes of the storage are 128 entries apart at least (RayStorage.PAD_FROM): the same trace into
    packed planes (padding switched off) must give the same rays, and the padding must stay as it was."""
    N = (1 << 20) + 1
    make = SCENES["two_steps"]

    def run(mode):
        RT = generated(make, N, mode, 1)
        if mode == DEFERRED:
            for k in ("p", "pol", "n"):
                RT.rays._dev[k]
        return RT

    monkeypatch.setattr(RayStorage, "PAD_FROM", 1 << 40)
    RT = run(COMPLETE)
    assert RT.rays._Np == N
    ref, _ = planes(RT, N)
    del RT
    monkeypatch.undo()
    for mode in (COMPLETE, DEFERRED):
        RT = run(mode)
        assert RT.rays._Np == N + 127
        got, pad = planes(RT, N)
        assert_bits(got, ref, f"stride {RT.rays._Np}, {mode} stores")
        assert all(untouched(pad[k], k) for k in pad), "a store went into the padding behind the last ray"
        del RT, got, pad


# ---- the reciprocal of the refraction step -------------------------------------------------------------------------------------
def test_fast_reciprocal_is_as_accurate_as_its_comment_says():
    """`fast_rcp` (csrc/ot_device.hpp: the hardware seed and one Newton step) on 2^27 operands of the range `refract` hands
    it, measured by the library's self-test: its largest relative error is at or below OT_FAST_RCP_BOUND = 2^-48, the bound
    stated where it is defined -- a factor 2^24 inside the rounding of the float32 values it feeds.  The errors of the seed
    alone and of a second step are printed: they are what the comment there records (MI355X: 2^-24.36, 2^-48.67, 2^-53.00)."""
    lib = _capi.load_library()
    over, err = C.c_int64(-1), (C.c_double * 4)()
    _capi.check(lib.ot_selftest_arith(4, 4, 1 << 27, 20261, C.byref(over), err, stream_ptr()))
    print(f"v_rcp_f64 seed: 2^{np.log2(err[0]):.2f}   one Newton step: 2^{np.log2(err[1]):.2f}   two steps: 2^{np.log2(err[2]):.2f}"
          f"   fast_rcp: 2^{np.log2(err[3]):.2f}   operands over the bound: {over.value}")
    assert 0 < err[2] < err[1] < err[0] < 2.0 ** -8, "a Newton step did not improve on what it started from"
    assert over.value == 0 and 0 < err[3] <= 2.0 ** -48
    assert lib.ot_selftest_arith(4, 0, 16, 1, C.byref(over), err, stream_ptr()) == -1, "the case has one operand class"
