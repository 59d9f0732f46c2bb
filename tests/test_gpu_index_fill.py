"""The index plane n[section, ray] is written on demand: the tracer's scenes have their index store switched off
(`ot_scene_set_index_store`), a trace leaves `RayStorage._dev["n"]` alone and the first read of it runs `ot_rays_fill_index`.

The yardstick is the trace kernel itself with the switch ON (the default of the C-ABI): the filled plane must equal the
stored one bit for bit -- the fill evaluates the same device functions on the same wavelengths, so there is no tolerance --
and every other plane must not notice the switch.  One scene is tied to the reference's golden vectors as well.
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


@pytest.fixture
def padded(monkeypatch):
    """Planes padded from 512 rays on, so that the small cases run with a plane stride `_Np` > N."""
    monkeypatch.setattr(RayStorage, "PAD_FROM", 512)


def raw(RT, key):
    """The device tensor without the hook of `_dev` (no fill)."""
    return dict.__getitem__(RT.rays._dev, key)


def planes(RT, hook: bool, count: int) -> dict:
    """name -> (rows, count) host array of every plane; `hook`: read through `_dev[...]` (fills n) or past it."""
    r = RT.rays
    Np, nt = r._Np, r._nt
    out = {}
    for key, rows in (("n", nt), ("p", 3 * nt), ("s", 3), ("w", nt), ("wl", 1), ("pol", 3 * nt)):
        t = r._dev[key] if hook else raw(RT, key)
        if t is not None:
            out[key] = t.view(rows, Np)[:, :count].cpu().numpy()
    return out


def store_on_run(make, N, **kw) -> dict:
    """The planes of a trace whose kernel stored the index plane itself (switch on), never touched by the fill."""
    lib = _capi.load_library()
    with ot.global_options.no_warnings():
        RT = make()
        RT.trace(N, **kw)  # compiles the scene
        _capi.check(lib.ot_scene_set_index_store(RT._scene_handle, 1))
        raw(RT, "n").fill_(float("nan"))
        RT.trace(N, **kw)  # a seeded tracer repeats itself call for call
    assert RT.rays._n_stale, "nothing here may have read the plane through the hook"
    count = RT.rays._Np if "_initial_rays" in kw else N
    return planes(RT, False, count)


def filled_run(make, N, **kw):
    with ot.global_options.no_warnings():
        RT = make()
        RT.trace(N, **kw)
    assert RT.rays._n_stale
    return RT


def assert_planes_equal(got: dict, ref: dict, N: int) -> None:
    """`N`: the rays proper (the padding of handed-in rays carries wavelength 0 and whatever index that gives)."""
    assert set(got) == set(ref)
    assert np.isfinite(ref["n"]).all() and ref["n"][:, :N].min() >= 1.0, "the stored plane must be complete"
    assert np.array_equal(got["n"], ref["n"]), f"n differs in {np.count_nonzero(got['n'] != ref['n'])} entries"
    for key in ref:
        assert np.array_equal(got[key], ref[key], equal_nan=True), f"plane {key} differs"


def mixed_lines(**kw):
    RT = scenes.mixed_geometry(ot, **kw)
    RT.ray_sources[1].spectrum = ot.LightSpectrum("Lines", lines=[450., 550., 610., 680.], line_vals=[1, 2, 1, 0.5])
    return RT


CASES = {
    "double_gauss": (lambda: scenes.double_gauss(ot, seed=5), N_SMALL),                         # SPEC 2
    "double_gauss_nopol": (lambda: scenes.double_gauss(ot, seed=5, no_pol=True), N_SMALL),      # SPEC 2
    "double_gauss_ranges": (lambda: scenes.double_gauss(ot, seed=6), N_RANGES),                 # range borders inside waves
    "mixed_lines": (lambda: mixed_lines(seed=7), N_SMALL),          # SPEC 2: filter, ideal lens, Function index
    "c3_arizona_eye_rgb": (lambda: scenes.c3_arizona_eye_rgb(ot), N_SMALL),                     # SPEC 0 / 1, continuous
    "hurb_slit_lens": (lambda: scenes.hurb_slit_lens(ot, seed=8), N_SMALL),
    "double_gauss_aspheric": (lambda: scenes.double_gauss(ot, aspheric=True, seed=9), N_SMALL),
}


@gpu
@pytest.mark.parametrize("name", list(CASES))
def test_filled_plane_equals_stored_plane(padded, name):
    make, N = CASES[name]
    ref = store_on_run(make, N)
    RT = filled_run(make, N)
    assert RT.rays._Np > N
    if N == N_RANGES:  # some source range starts in the middle of a wave
        assert any(int(r.first) % 64 for r in RT.rays._source_ranges())
    got = planes(RT, True, N)
    assert not RT.rays._n_stale
    assert_planes_equal(got, ref, N)


def golden_inputs(name="double_gauss"):
    g = load(f"trace_{name}.npz")
    kw = dict(_initial_rays=(g["p0"], g["s0"], g["pol0"], g["w0"], g["wl"]), _N_list=g["N_list"])
    return g, int(g["N"]), kw


@gpu
def test_injected_rays(padded):
    """Rays handed in (GEN = false, the formula kernels even for a line spectrum): the whole stride is traced and filled."""
    g, N, kw = golden_inputs()
    make = lambda: scenes.double_gauss(ot)
    ref = store_on_run(make, N, **kw)
    RT = filled_run(make, N, **kw)
    assert RT.rays._Np > N
    assert_planes_equal(planes(RT, True, RT.rays._Np), ref, N)


@gpu
def test_n_list_matches_golden():
    """The filled plane against the reference's own n_list (bar of test_gpu_parity.test_trace_matches_reference)."""
    g, N, kw = golden_inputs()
    RT = filled_run(lambda: scenes.double_gauss(ot), N, **kw)
    assert_close(RT.rays.n_list, g["n_list"], rtol=1e-13, what="n_list")
    assert not RT.rays._n_stale


@gpu
def test_every_trace_marks_the_plane_stale(padded):
    make = lambda seed: (lambda: scenes.double_gauss(ot, seed=seed))
    N = N_SMALL
    ref1, ref2 = store_on_run(make(21), N), store_on_run(make(22), N)
    assert not np.array_equal(ref1["n"], ref2["n"])  # other wavelengths per ray
    RT = filled_run(make(21), N)
    assert np.array_equal(RT.rays.n_list, ref1["n"].T)
    RT.seed = 22
    with ot.global_options.no_warnings():
        RT.trace(N)
    assert RT.rays._n_stale
    assert np.array_equal(RT.rays.n_list, ref2["n"].T)


@gpu
def test_plane_describes_the_scene_that_traced_the_rays(padded):
    make = lambda: scenes.double_gauss(ot, seed=23)
    N = N_SMALL
    ref = store_on_run(make, N)
    RT = filled_run(make, N)
    RT.lenses[0].n = ot.RefractionIndex("Constant", n=1.31)
    assert np.array_equal(RT.rays.n_list, ref["n"].T)
    # and through a recompiled scene: the storage keeps the old one until the plane is filled or traced anew
    RT2 = filled_run(make, N)
    RT2.lenses[0].n = ot.RefractionIndex("Constant", n=1.31)
    with ot.global_options.no_warnings():
        RT2._compile(RT2._geometry_key())
    assert RT2.rays._n_stale
    assert np.array_equal(RT2.rays.n_list, ref["n"].T)
    with ot.global_options.no_warnings():
        RT2.trace(N)
    n_new = RT2.rays.n_list
    assert np.all(n_new[:, 1] == 1.31) and not np.array_equal(n_new, ref["n"].T)


@gpu
def test_accessors_fill_the_plane(padded):
    make = lambda: scenes.double_gauss(ot, seed=24)
    N = N_SMALL
    with ot.global_options.no_warnings():
        A = make()
        A.trace(N)
        _capi.check(_capi.load_library().ot_scene_set_index_store(A._scene_handle, 1))
        A.trace(N)
    A.rays.__dict__["_n_stale"] = False  # the kernel stored the plane: read it as it is
    ch = np.zeros(N, dtype=bool)
    ch[np.random.default_rng(3).choice(N, 100, replace=False)] = True
    ret = [0, 0, 0, 0, 0, 0, 1]
    opt_ref, n_ref = A.rays.optical_lengths(ch), A.rays.rays_by_mask(ch, ret=ret)[6]
    B = filled_run(make, N)
    assert np.array_equal(B.rays.optical_lengths(ch), opt_ref, equal_nan=True)
    assert not B.rays._n_stale and "n" not in B.rays._host  # filled on the device, gathered there
    C_ = filled_run(make, N)
    got = C_.rays.rays_by_mask(ch, ret=ret)[6]
    assert got.shape == (100, C_.rays.Nt) and np.array_equal(got, n_ref)


@gpu
def test_plane_is_written_on_demand_only(padded):
    N = N_SMALL
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=25)
        RT.trace(N)
        raw(RT, "n").fill_(-7.0)
        RT.trace(N)
        img = RT.detector_image()
    assert img.power() > 0
    assert RT.rays._n_stale
    assert bool((raw(RT, "n") == -7.0).all()), "trace and detector image must leave the plane alone"
    n = RT.rays.n_list
    assert not RT.rays._n_stale and n.shape == (N, RT.rays.Nt) and n.min() >= 1.0 and n.max() < 2.0


# ---- CPU tier ----------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_check_their_arguments():
    import pathlib
    header = (pathlib.Path(__file__).resolve().parent.parent / "include" / "optrace_amd.h").read_text()
    for name in ("ot_scene_set_index_store", "ot_rays_fill_index"):
        assert f"int {name}(" in header and name in _capi.SIGNATURES
    lib = _capi.load_library()
    assert lib.ot_scene_set_index_store(None, 0) == -1  # OT_ERR_INVALID
    rays = _capi.Rays()
    assert lib.ot_rays_fill_index(None, C.byref(rays), 0, 0, None) == -1
    assert lib.ot_rays_fill_index(None, None, 0, 0, None) == -1
    assert b"ot_rays_fill_index" in lib.ot_last_error()
