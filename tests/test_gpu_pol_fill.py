"""The polarisation planes pol[3, section, ray] are written on demand: the tracer's scenes defer them
(`ot_scene_set_deferred_planes`, bit `OT_DEFER_POL`), a trace that generates its rays on the device leaves
`RayStorage._dev["pol"]` alone and the first read of it repeats the trace with the polarisation stores as its only stores
(`ot_rays_fill_pol`).

The yardstick is the storing trace kernel itself with complete stores switched on (`ot_scene_set_index_store(handle, 1)` clears
the whole mask), its planes read past the hook of `_dev`: the replayed planes must equal the stored ones bit for bit, NaN
patterns after total internal reflection included -- the replay runs the same device functions on the same Philox streams, so
there is no tolerance --, and every other plane must not notice the switch.  Rays handed in are always stored by their trace;
that path is tied to the reference's golden vectors.
"""
import ctypes as C

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd.ray_storage import RayStorage

import scenes
from helpers import load, assert_close

gpu = pytest.mark.gpu

N_SMALL = 1000          # three full workgroups and a ragged last wave
N_RANGES = 64 * 1024 + 1  # `_source_ranges` cuts each source's share into power-of-two blocks and a ragged rest: borders inside waves
PLANES = (("n", 1), ("p", 3), ("s", 0), ("w", 1), ("wl", 0), ("pol", 3))  # name, planes per section (0: per ray)


@pytest.fixture
def padded(monkeypatch):
    """Planes padded from 512 rays on, so that the small cases run with a plane stride `_Np` > N."""
    monkeypatch.setattr(RayStorage, "PAD_FROM", 512)


def raw(RT, key):
    """The device tensor without the hook of `_dev` (no fill)."""
    return dict.__getitem__(RT.rays._dev, key)


def planes(RT, hook: bool, count: int) -> dict:
    """name -> (rows, count) host array of every plane; `hook`: read through `_dev[...]` (fills n and pol) or past it."""
    r = RT.rays
    Np, nt = r._Np, r._nt
    out = {}
    for key, per_section in PLANES:
        rows = per_section * nt if per_section else (3 if key == "s" else 1)
        t = r._dev[key] if hook else raw(RT, key)
        if t is not None:
            out[key] = t.view(rows, Np)[:, :count].cpu().numpy()
    return out


def stored_tracer(make, N, **kw):
    """A tracer whose kernel stored every plane itself (empty mask); nothing has gone through the hooks."""
    lib = _capi.load_library()
    with ot.global_options.no_warnings():
        RT = make()
        RT.trace(N, **kw)  # compiles the scene
        _capi.check(lib.ot_scene_set_index_store(RT._scene_handle, 1))
        if raw(RT, "pol") is not None:
            raw(RT, "pol").fill_(-3.0)
        RT.trace(N, **kw)  # a seeded tracer repeats itself call for call
    return RT


def store_on_run(make, N, **kw) -> dict:
    return planes(stored_tracer(make, N, **kw), False, N)


def filled_run(make, N, **kw):
    with ot.global_options.no_warnings():
        RT = make()
        RT.trace(N, **kw)
    assert RT.rays._pol_stale is not None
    return RT


def assert_planes_equal(got: dict, ref: dict) -> None:
    assert set(got) == set(ref) and "pol" in ref
    assert not (ref["pol"] == -3.0).any(), "the storing kernel must have written every polarisation entry"
    for key in ref:
        a, b = got[key], ref[key]
        same = np.array_equal(a, b, equal_nan=True)
        assert same, f"plane {key} differs in {np.count_nonzero(~((a == b) | (np.isnan(a) & np.isnan(b))))} entries"
    # bit for bit, the payload of a NaN included
    assert np.array_equal(got["pol"].view(np.uint32), ref["pol"].view(np.uint32))


def mixed_lines(**kw):
    RT = scenes.mixed_geometry(ot, **kw)
    RT.ray_sources[1].spectrum = ot.LightSpectrum("Lines", lines=[450., 550., 610., 680.], line_vals=[1, 2, 1, 0.5])
    return RT


def same_medium(**kw):
    """A lens whose medium behind (`n2`) is its own: the back surface refracts between equal indices."""
    RT = ot.Raytracer(outline=[-5, 5, -5, 5, -5, 40], **kw)
    RT.add(ot.RaySource(ot.CircularSurface(r=1.5), divergence="Isotropic", div_angle=4, pos=[0, 0, -3], s=[0, 0.02, 1],
                        spectrum=ot.LightSpectrum("Monochromatic", wl=550.), polarization="Uniform"))
    n = ot.RefractionIndex("Constant", n=1.6)
    RT.add(ot.Lens(ot.SphericalSurface(r=3, R=9), ot.SphericalSurface(r=3, R=-12), de=0.2, pos=[0, 0, 2], n=n, n2=n))
    RT.add(ot.Lens(ot.SphericalSurface(r=3, R=14), ot.SphericalSurface(r=3, R=-14), de=0.2, pos=[0, 0, 12],
                   n=ot.RefractionIndex("Constant", n=1.45)))
    return RT


def tir_scene(**kw):
    """A collimated beam into a flat-fronted lens with a nearly hemispherical back (R = -3, n = 1.8): rays further than
    R / n = 1.67 mm from the axis meet the back surface beyond the critical angle."""
    RT = ot.Raytracer(outline=[-6, 6, -6, 6, -5, 40], **kw)
    RT.add(ot.RaySource(ot.CircularSurface(r=2.5), divergence="None", s=[0, 0, 1], pos=[0, 0, -3],
                        spectrum=ot.LightSpectrum("Monochromatic", wl=550.), polarization="x"))
    RT.add(ot.Lens(ot.CircularSurface(r=3), ot.SphericalSurface(r=2.9, R=-3), de=0.2, pos=[0, 0, 2],
                   n=ot.RefractionIndex("Constant", n=1.8)))
    RT.add(ot.Lens(ot.SphericalSurface(r=4, R=20), ot.SphericalSurface(r=4, R=-20), de=0.2, pos=[0, 0, 15],
                   n=ot.RefractionIndex("Constant", n=1.5)))
    return RT


CASES = {
    "double_gauss": (lambda: scenes.double_gauss(ot, seed=5), N_SMALL),                         # SPEC 2, the bench kernel
    "double_gauss_ranges": (lambda: scenes.double_gauss(ot, seed=6), N_RANGES),                 # range borders inside waves
    "mixed_lines": (lambda: mixed_lines(seed=7), N_SMALL),          # SPEC 2: filter, ideal lens, Function index
    "c3_arizona_eye_rgb": (lambda: scenes.c3_arizona_eye_rgb(ot), N_SMALL),                     # continuous, image source
    "hurb_slit_lens": (lambda: scenes.hurb_slit_lens(ot, seed=8), N_SMALL),                     # Philox HURB deviates
    "double_gauss_aspheric": (lambda: scenes.double_gauss(ot, aspheric=True, seed=9), N_SMALL),
    "freeform": (lambda: scenes.freeform_scene(ot, seed=10), N_SMALL),                          # spline level
    "asphere_hurb": (lambda: scenes.asphere_scene(ot, use_hurb=True, seed=13), N_SMALL),        # feature level 3
    "freeform_hurb": (lambda: scenes.freeform_hurb_scene(ot, seed=14), N_SMALL),                # feature level 5
    "same_medium": (lambda: same_medium(seed=11), N_SMALL),
    "tir": (lambda: tir_scene(seed=12), N_SMALL),
}


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_replayed_planes_equal_stored_planes(padded, name):
    make, N = CASES[name]
    ST = stored_tracer(make, N)
    ref = planes(ST, False, N)
    RT = filled_run(make, N)
    assert RT.rays._Np > N
    if N == N_RANGES:  # some source range starts in the middle of a wave
        assert any(int(r.first) % 64 for r in RT.rays._source_ranges())
    if name == "tir":
        assert ST._msgs[ST.INFOS.TIR].sum() > 0 and RT._msgs[RT.INFOS.TIR].sum() > 0
        assert np.isnan(ref["pol"]).any(), "total internal reflection leaves NaN polarisation"
    msgs = RT._msgs.copy()
    got = planes(RT, True, N)
    assert RT.rays._pol_stale is None
    assert_planes_equal(got, ref)
    assert np.array_equal(RT._msgs, msgs) and np.array_equal(RT._msgs, ST._msgs)


@gpu
def test_pol_list_of_handed_in_rays_matches_golden():
    """Rays handed in (`ot_trace`): the trace stores the planes itself, no mark; the bar of
    test_gpu_parity.test_trace_matches_reference."""
    g = load("trace_double_gauss.npz")
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot)
        RT.trace(int(g["N"]), _initial_rays=(g["p0"], g["s0"], g["pol0"], g["w0"], g["wl"]), _N_list=g["N_list"])
    assert RT.rays._pol_stale is None
    assert RT.rays.pol_list.dtype == np.float32
    assert_close(RT.rays.pol_list, g["pol_list"], rtol=1e-5, atol=2e-7, what="pol_list")


@gpu
def test_handed_in_rays_after_a_generated_trace_clear_the_mark(padded):
    g = load("trace_double_gauss.npz")
    N = int(g["N"])
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=3)
        RT.trace(N)  # same shape: the buffers are reused and carry a mark
        assert RT.rays._pol_stale is not None
        RT.trace(N, _initial_rays=(g["p0"], g["s0"], g["pol0"], g["w0"], g["wl"]), _N_list=g["N_list"])
    assert RT.rays._pol_stale is None
    assert_close(RT.rays.pol_list, g["pol_list"], rtol=1e-5, atol=2e-7, what="pol_list")


@gpu
def test_planes_are_written_on_demand_only(padded):
    N = N_SMALL
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=25)
        RT.trace(N)
        raw(RT, "pol").fill_(-7.0)
        RT.trace(N)
        RT.trace(N)
        img = RT.detector_image()
    assert img.power() > 0
    assert RT.rays._pol_stale is not None
    assert bool((raw(RT, "pol") == -7.0).all()), "trace and detector image must leave the planes alone"
    pol = RT.rays.pol_list
    assert RT.rays._pol_stale is None and pol.shape == (N, RT.rays.Nt, 3) and pol.dtype == np.float32
    alive = RT.rays.w_list > 0
    assert np.isfinite(pol[alive]).all()
    assert np.abs(np.linalg.norm(pol[:, 0].astype(np.float64), axis=1) - 1).max() < 1e-6


@gpu
def test_every_trace_overwrites_the_mark(padded):
    make = lambda seed: (lambda: scenes.double_gauss(ot, seed=seed))
    N = N_SMALL
    ref1, ref2 = store_on_run(make(21), N), store_on_run(make(22), N)
    assert not np.array_equal(ref1["pol"], ref2["pol"])
    RT = filled_run(make(21), N)
    RT.seed = 22
    with ot.global_options.no_warnings():
        RT.trace(N)
    assert RT.rays._pol_stale is not None
    pol = RT.rays.pol_list  # (N, nt, 3) against rows (component, section)
    assert np.array_equal(pol.transpose(2, 1, 0).reshape(-1, N), ref2["pol"], equal_nan=True)


@gpu
def test_planes_describe_the_scene_that_traced_the_rays(padded):
    make = lambda: scenes.double_gauss(ot, seed=23)
    N = N_SMALL
    ref = store_on_run(make, N)
    RT = filled_run(make, N)
    RT.lenses[0].n = ot.RefractionIndex("Constant", n=1.31)
    with ot.global_options.no_warnings():
        RT._compile(RT._geometry_key())  # the tracer lets go of the scene that traced; the storage keeps it
    assert RT.rays._pol_stale is not None
    msgs = RT._msgs.copy()
    pol = RT.rays.pol_list
    assert np.array_equal(pol.transpose(2, 1, 0).reshape(-1, N), ref["pol"], equal_nan=True)
    assert np.array_equal(RT._msgs, msgs)
    with ot.global_options.no_warnings():
        RT.trace(N)
    assert not np.array_equal(RT.rays.pol_list, pol, equal_nan=True)


@gpu
def test_accessors_replay_the_planes(padded):
    make = lambda: scenes.double_gauss(ot, seed=24)
    N = N_SMALL
    A = stored_tracer(make, N)
    A.rays.__dict__["_pol_stale"] = None  # the kernel stored the planes: read them as they are
    ch = np.zeros(N, dtype=bool)
    ch[np.random.default_rng(3).choice(N, 100, replace=False)] = True
    ret = [0, 0, 1, 0, 0, 0, 0]
    pol_ref, src_ref = A.rays.rays_by_mask(ch, ret=ret)[2], A.rays.source_sections(1)[2]
    B = filled_run(make, N)
    got = B.rays.rays_by_mask(ch, ret=ret)[2]
    assert B.rays._pol_stale is None and "pol" not in B.rays._host  # replayed on the device, gathered there
    assert got.shape == (100, B.rays.Nt, 3) and np.array_equal(got, pol_ref, equal_nan=True)
    C_ = filled_run(make, N)
    assert "pol" not in C_.rays._host
    got = C_.rays.source_sections(1)[2]
    assert C_.rays._pol_stale is None and got.shape == (int(C_.rays.N_list[1]), 3) and np.array_equal(got, src_ref)


@gpu
def test_no_pol_tracer_has_no_planes_and_no_mark(padded):
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=5, no_pol=True)
        RT.trace(N_SMALL)
    assert raw(RT, "pol") is None and RT.rays._dev["pol"] is None and RT.rays._pol_stale is None
    assert np.isnan(RT.rays.pol_list).all()


# ---- CPU tier ----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_check_their_arguments():
    import pathlib
    header = (pathlib.Path(__file__).resolve().parent.parent / "include" / "optrace_amd.h").read_text()
    for name in ("ot_scene_set_deferred_planes", "ot_rays_fill_pol"):
        assert f"int {name}(" in header and name in _capi.SIGNATURES
    assert "#define OT_DEFER_INDEX 1u" in header and "#define OT_DEFER_POL 2u" in header
    assert (_capi.OT_DEFER_INDEX, _capi.OT_DEFER_POL) == (1, 2)
    lib = _capi.load_library()
    assert lib.ot_scene_set_deferred_planes(None, 3) == -1  # OT_ERR_INVALID
    assert b"ot_scene_set_deferred_planes" in lib.ot_last_error()
    rays, rng = _capi.Rays(), (_capi.SourceRange * 1)()
    assert lib.ot_rays_fill_pol(None, None, rng, 1, 0, C.byref(rays), 0, 0, None) == -1
    assert b"ot_rays_fill_pol" in lib.ot_last_error()
    assert lib.ot_rays_fill_pol(None, None, None, 0, 0, None, 0, 0, None) == -1
    assert b"ot_rays_fill_pol" in lib.ot_last_error()


@gpu
def test_mismatched_arguments_are_refused(padded):
    lib = _capi.load_library()
    RT = filled_run(lambda: scenes.double_gauss(ot, seed=5), N_SMALL)
    scene, tab, rng, seed, count = RT.rays._pol_stale
    rays = RT.rays._rays_struct()

    def call(r, first=0, n=count, sc=scene):
        return lib.ot_rays_fill_pol(sc.handle, tab.handle, rng, len(rng), seed, C.byref(r), first, n, None)

    def variant(**kw):
        r = _capi.Rays()
        C.memmove(C.byref(r), C.byref(rays), C.sizeof(r))
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    for bad in (variant(pol=None), variant(nt=rays.nt - 1)):
        assert call(bad) == -1 and b"ot_rays_fill_pol" in lib.ot_last_error()
    for first, n in ((-1, 1), (0, rays.N + 1), (rays.N, 1)):
        assert call(rays, first, n) == -1 and b"ot_rays_fill_pol" in lib.ot_last_error()
    with ot.global_options.no_warnings():
        NP = scenes.double_gauss(ot, seed=5, no_pol=True)
        NP.trace(N_SMALL)
    assert call(rays, sc=NP._scene_ref) == -1 and b"ot_rays_fill_pol" in lib.ot_last_error()
    assert RT.rays._pol_stale is not None  # nothing above went through the storage
