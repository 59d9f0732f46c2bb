"""Aspheres with more than OT_MAX_ASPH = 12 coefficients on the device (OT_SURF_FLAG_ASPH_TABLE; csrc/ot_device.hpp::
asph_poly_long, the table-carrying kernels): leaf calls, the trace, the detector image and the render-only trace against the
reference's recorded output (tests/golden/leaf_surfaces_asph_long.npz, trace_asphere_long*.npz -- the plain-C oracle keeps
its twelve-coefficient limit and takes no part here), the seam between twelve and thirteen coefficients, and the argument
checks of the C-ABI.  Tolerances: those of tests/test_gpu_surfaces3.py and tests/test_gpu_parity.py for aspheres."""
import ctypes as C

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd._device import ptr, stream_ptr
from optrace_amd.scene import CompiledScene

import scenes_asph_long as sal
import test_gpu_parity as parity
from helpers import load, assert_close
from test_gpu_fused_detector import same_image
from test_gpu_render_only import settings

pytestmark = pytest.mark.gpu

# the scene under the names its fixtures carry: test_gpu_parity's own comparisons then run on it unchanged
parity.ALL_SCENES["asphere_long"] = (sal.asphere_long_scene, 2500)
TRACES = ["asphere_long", "asphere_long_nopol"]


@pytest.fixture(scope="module")
def zoo():
    with ot.global_options.no_warnings():
        return sal.surface_zoo_long(ot)


@pytest.fixture(scope="module")
def leaf():
    return load("leaf_surfaces_asph_long.npz")


@pytest.mark.parametrize("name", sal.NAMES)
def test_find_hit(zoo, leaf, name):
    sf = zoo[name]
    assert len(sf.coeff) > _capi.OT_MAX_ASPH
    p, s = leaf[f"{name}/p"], leaf[f"{name}/s"]
    assert p.shape == (1500, 3)
    ph, hit, ill = sf.find_hit(p, s)
    assert hit.shape == (1500,) and ill.shape == (1500,)
    assert np.array_equal(hit, leaf[f"{name}/is_hit"]), "hit mask must be bit-exact"
    assert np.array_equal(np.asarray(ill, dtype=bool), leaf[f"{name}/ill"]), "ill-conditioned mask must be bit-exact"
    err = np.abs(ph - leaf[f"{name}/p_hit"])
    print(f"{name}: hits {hit.sum()}, ill {ill.sum()}, max |p_hit - ref| = {err.max():.3e}")
    assert_close(ph, leaf[f"{name}/p_hit"], rtol=0, atol=1e-11, what=f"{name} p_hit")


@pytest.mark.parametrize("name", sal.NAMES)
def test_mask_values_normals(zoo, leaf, name):
    sf = zoo[name]
    x, y = leaf[f"{name}/x"], leaf[f"{name}/y"]
    assert x.shape == (1500,)
    assert np.array_equal(sf.mask(x, y), leaf[f"{name}/mask"])
    v, n = sf.values(x, y), sf.normals(x, y)
    print(f"{name}: max |values - ref| = {np.abs(v - leaf[f'{name}/values']).max():.3e}, "
          f"max |normals - ref| = {np.abs(n - leaf[f'{name}/normals']).max():.3e}")
    assert_close(v, leaf[f"{name}/values"], rtol=1e-13, atol=1e-14, what=f"{name} values")
    assert_close(n, leaf[f"{name}/normals"], rtol=1e-11, atol=1e-13, what=f"{name} normals")


@pytest.mark.parametrize("name", TRACES)
def test_trace_matches_reference(name):
    """test_gpu_parity's comparison of a scene trace: counters and alive masks bit-exact, positions 1e-11, weights,
    pol_list, refractive indices and final directions at that file's tolerances."""
    parity.test_trace_matches_reference(name)


def test_scene_takes_the_table_carrying_level():
    """Long aspheres raise the scene to the spline level; the short-asphere scene stays where it was."""
    g, RT = parity.gpu_trace("asphere_long")
    d = CompiledScene(RT).surfaces
    assert [d[i].ncoeff for i in range(4)] == [16, 24, 3, 0]
    assert d[0].flags & d[1].flags & _capi.SURF_FLAG_ASPH_TABLE and not d[2].flags
    assert int(g["msgs"].sum()) > 0 and (g["w_list"][:, -2] > 0).sum() * 2 >= int(g["N"])


@pytest.mark.parametrize("name", TRACES)
def test_detector_image_matches_reference(name):
    """test_gpu_parity's comparison of the detector stage: hit count exact, image 1e-4 in image norm, extent 1e-9."""
    parity.test_detector_image_matches_reference(name)


@pytest.mark.parametrize("no_pol", [False, True])
def test_iterative_render_render_only_equals_stored_path(no_pol):
    """Three chunks of 400 000 rays (the first two render-only, `ot_trace_t*`) against the same chunks through the ray
    storage: same pixels lit, sums within the bounds of tests/test_gpu_render_only.py (1e-11 of the image maximum,
    1e-12 in power), equal counters."""
    with ot.global_options.no_warnings():
        n = 400_000
        out = {}
        for mode in (True, False):
            RT = sal.asphere_long_scene(ot, seed=5, no_pol=no_pol)
            traced = []
            orig = RT.trace

            def spy(N, **kw):
                traced.append((N, kw.get("_tail") is not None))
                return orig(N, **kw)

            RT.trace = spy
            with settings(ITER_RAYS_STEP=n, ITER_RENDER_ONLY=mode, ITER_EXTENT_RAYS=1 << 60, ITER_MERGE_LAST=False):
                imgs = RT.iterative_render(3 * n + 77, extent=[-4, 4, -4, 4])
            del RT.trace
            assert traced == [(n, mode), (n, mode), (n + 77, False)]
            assert not RT.geometry_error
            out[mode] = (imgs, RT._msgs.copy())
    (a, ma), (b, mb) = out[True], out[False]
    assert np.array_equal(ma, mb)
    for x, y in zip(a, b):
        same_image(x, y, tol=1e-11)
        assert abs(x.power() - y.power()) <= 1e-12 * y.power()


def test_thirteenth_coefficient_of_zero_changes_nothing(leaf):
    """A 12-coefficient surface (inline coefficients, the unrolled chain) and the same surface with a thirteenth
    coefficient of 0.0 (table, runtime-length loop).  np.polyval with a leading zero is the same arithmetic -- the
    first steps give (0 r + 0) r = 0, then 0 r + a_12 = a_12 -- so bit equality is expected and reported, but only
    identical hit masks and agreement within the asphere tolerances are required."""
    name = "asph_n13_last_zero"
    c13 = leaf[f"{name}/param/coeff"]
    assert c13.shape == (13,) and c13[-1] == 0.0
    with ot.global_options.no_warnings():
        s12 = ot.AsphericSurface(r=2.5, R=-9.0, k=0.6, coeff=list(c13[:12]))
        s13 = ot.AsphericSurface(r=2.5, R=-9.0, k=0.6, coeff=list(c13))
    for sf in (s12, s13):
        sf.move_to(leaf[f"{name}/param/pos"])
    assert (s12.z_min, s12.z_max) == (s13.z_min, s13.z_max)
    assert not s12._desc().flags and s13._desc().flags & _capi.SURF_FLAG_ASPH_TABLE
    p, s, x, y = (leaf[f"{name}/{k}"] for k in "psxy")
    (ph12, hit12, ill12), (ph13, hit13, ill13) = s12.find_hit(p, s), s13.find_hit(p, s)
    v12, v13, n12, n13 = s12.values(x, y), s13.values(x, y), s12.normals(x, y), s13.normals(x, y)
    print("bit-equal: p_hit", np.array_equal(ph12, ph13), "values", np.array_equal(v12, v13), "normals",
          np.array_equal(n12, n13))
    assert np.array_equal(hit12, hit13) and np.array_equal(ill12, ill13)
    assert np.array_equal(hit13, leaf[f"{name}/is_hit"])
    assert_close(ph12, ph13, rtol=0, atol=1e-11, what="p_hit")
    assert_close(v12, v13, rtol=1e-13, atol=1e-14, what="values")
    assert_close(n12, n13, rtol=1e-11, atol=1e-13, what="normals")


# ---- argument checks (validation only: every call below is refused before anything is launched) ----------------------
def long_desc(n=13):
    with ot.global_options.no_warnings():
        sf = ot.AsphericSurface(r=2.5, R=8.0, k=-2.5, coeff=sal.long_coeff(2.5, n))
    return sf._desc()


def bad_descs():
    d = long_desc()
    d.flags &= ~_capi.SURF_FLAG_ASPH_TABLE  # 13 coefficients, nowhere to read the thirteenth from
    yield "no flag", d
    d = long_desc()
    d.tab = None
    yield "tab NULL", d
    d = long_desc()
    d.tab_len = 12
    yield "tab_len short", d
    d = long_desc()
    d.tab_len = 14
    yield "tab_len long", d
    d = long_desc()
    d.ncoeff = 16  # 16 coefficients announced, 13 given
    yield "ncoeff above tab_len", d


@pytest.mark.parametrize("case", [c for c, _ in bad_descs()])
def test_leaf_calls_refuse_inconsistent_long_aspheres(case):
    lib = _capi.load_library()
    d = dict(bad_descs())[case]
    n = 64
    x = torch.zeros(n, dtype=torch.float64, device="cuda")
    p = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    s = torch.zeros(3 * n, dtype=torch.float64, device="cuda")
    s[2 * n:] = 1.0
    out = torch.full((3 * n,), 7.0, dtype=torch.float64, device="cuda")
    flags = torch.full((2 * n,), 7, dtype=torch.uint8, device="cuda")
    calls = {
        "values": lambda: lib.ot_surface_values(C.byref(d), n, ptr(x), ptr(x), ptr(out), stream_ptr()),
        "normals": lambda: lib.ot_surface_normals(C.byref(d), n, ptr(x), ptr(x), ptr(out), stream_ptr()),
        "mask": lambda: lib.ot_surface_mask(C.byref(d), n, ptr(x), ptr(x), ptr(flags), stream_ptr()),
        "find_hit": lambda: lib.ot_surface_find_hit(C.byref(d), n, ptr(p), ptr(s), ptr(out), ptr(flags),
                                                    ptr(flags[n:]), stream_ptr()),
    }
    for what, call in calls.items():
        rc = call()
        msg = lib.ot_last_error()
        assert rc < 0, f"{case}: {what} accepted the descriptor"
        assert msg and b"asphere" in msg, (case, what, msg)
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((flags == 7).all()), "nothing was launched: the outputs are untouched"


@pytest.mark.parametrize("case", [c for c, _ in bad_descs()])
def test_scene_create_refuses_inconsistent_long_aspheres(case):
    lib = _capi.load_library()
    with ot.global_options.no_warnings():
        RT = sal.asphere_long_scene(ot)
        sc = CompiledScene(RT)
    bad = dict(bad_descs())[case]
    keep = sc.surfaces[0]
    for f in ("ncoeff", "flags", "tab", "tab_len"):
        setattr(keep, f, getattr(bad, f))
    handle = C.c_void_p()
    rc = lib.ot_scene_create(C.byref(sc.desc), C.byref(handle))
    msg = lib.ot_last_error()
    assert rc < 0 and not handle.value
    assert msg and b"asphere" in msg, msg
