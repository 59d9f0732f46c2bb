"""The step loop on its hot records against the same kernels on the surface records (`ot_scene_set_hot_steps`), and both
against the CPU oracle.

Small scenes whose steps mix the hot forms with OTHER.  The scenes built through `Raytracer` end with the tracer's own end
aperture, a rectangle (OTHER): `ring` is one hot step and that OTHER step, a lens two hot steps in front of it.  The
one-step scenes are scene descriptions handed to `ot_scene_create` and `ot_trace` directly (one aperture, nothing behind
it): n_steps == 1, a device table of two records of which the second is the padding, read back and checked.  193 rays are
three waves and one lane, 4096 rays sixteen workgroups; both sizes run every scene.

Per scene and size: a generating trace with the hot steps on and off -- every plane of the storage after its fills, the
final directions, the wavelengths and the counters bit for bit --, then the rays of that trace handed in again (the
formula kernels), on and off bit for bit and against `oracle_bridge.trace` on the same rays: masks and counters exact,
positions and weights within the bars of tests/test_gpu_parity.py::test_trace_matches_oracle.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd.ray_storage import TailStorage
from optrace_amd.scene import CompiledScene

import oracle_bridge as ob
from helpers import assert_close

pytestmark = pytest.mark.gpu

SIZES = (193, 4096)
LINES = dict(lines=[486.1327, 587.5618, 656.272], line_vals=[1., 2., 1.])


def build(name: str, spectrum: str = "lines", **rt_args):
    RT = ot.Raytracer(outline=[-6, 6, -6, 6, -12, 40], seed=5, **rt_args)
    spec = ot.LightSpectrum("Lines", **LINES) if spectrum != "formulas" else ot.LightSpectrum("Gaussian", mu=550., sig=40.)
    RT.add(ot.RaySource(ot.CircularSurface(r=2.8), divergence="Isotropic", div_angle=4, pos=[0.1, -0.05, -10],
                        spectrum=spec, polarization="Uniform"))
    glass = ot.RefractionIndex("Abbe", n=1.62, V=36.)
    if spectrum == "tables":
        glass = ot.RefractionIndex("Data", wls=np.linspace(380., 780., 41), vals=1.5 + 0.1 * np.exp(-np.linspace(0, 3, 41)))
    sph = ot.SphericalSurface
    if name == "three":  # hot -> OTHER -> hot: spherical lens, rotated rectangular aperture, conic lens
        RT.add(ot.Lens(sph(r=2.5, R=20.), sph(r=2.5, R=-25.), de=0.2, pos=[0, 0, 0], n=glass))
        rect = ot.RectangularSurface(dim=[1.2, 0.7])  # (an aperture absorbs what hits its surface)
        rect.rotate(25.)
        RT.add(ot.Aperture(rect, pos=[0.6, 0.4, 2]))
        RT.add(ot.Lens(ot.ConicSurface(r=2.5, R=8., k=-0.6), ot.ConicSurface(r=2.5, R=-10., k=-2.5), de=0.1, pos=[0, 0, 6],
                       n=ot.RefractionIndex("Cauchy", coeff=[1.49, 0.00354, 0, 0])))
    elif name == "spheres":  # plain next to stable: |R| on either side of 4096
        RT.add(ot.Lens(sph(r=2.5, R=20.), sph(r=2.5, R=-5000.), de=0.3, pos=[0, 0, 0], n=glass))
        RT.add(ot.Lens(sph(r=2.5, R=4097.), sph(r=2.5, R=-4096.), de=0.3, pos=[0, 0, 5], n=glass))
    elif name == "flat":
        RT.add(ot.Lens(ot.CircularSurface(r=2.2), ot.CircularSurface(r=2.2), de=0.5, pos=[0, 0, 2], n=glass))
    elif name == "ring":
        RT.add(ot.Aperture(ot.RingSurface(r=3., ri=0.9), pos=[0.2, 0.1, 3]))
    elif name == "decentred":  # px, py != 0 in the record: hit search, disc mask and normal are all relative to them
        RT.add(ot.Lens(sph(r=2.5, R=7.), sph(r=2.5, R=-9.), de=0.2, pos=[0.45, -0.35, 0], n=glass))
    elif name == "same_medium":  # N == 1
        RT.add(ot.Lens(sph(r=2.5, R=7.), sph(r=2.5, R=-9.), de=0.2, pos=[0, 0, 0], n=ot.RefractionIndex("Constant", n=1.0)))
    else:
        raise KeyError(name)
    return RT


SCENES = [("three", "lines"), ("three", "formulas"), ("three", "tables"), ("spheres", "lines"), ("flat", "lines"),
          ("ring", "lines"), ("decentred", "lines"), ("same_medium", "lines")]
FORMS = {"three": [_capi.HOT_SPHERE, _capi.HOT_SPHERE, 0, _capi.HOT_CONIC, _capi.HOT_CONIC, 0],
         "spheres": [_capi.HOT_SPHERE, _capi.HOT_SPHERE_STABLE, _capi.HOT_SPHERE_STABLE, _capi.HOT_SPHERE, 0],
         "flat": [_capi.HOT_FLAT, _capi.HOT_FLAT, 0], "ring": [_capi.HOT_RING, 0],
         "decentred": [_capi.HOT_SPHERE, _capi.HOT_SPHERE, 0], "same_medium": [_capi.HOT_SPHERE, _capi.HOT_SPHERE, 0]}


HOT_WORDS = 48  # int32 words of one hot record; word 1 is the form


def device_forms(handle, n_steps: int) -> np.ndarray:
    """The hot table as the device holds it: the forms of the steps; the padding record is checked to be zero."""
    buf = np.full((n_steps + 1) * HOT_WORDS, -1, dtype=np.int32)
    n = C.c_int32()
    _capi.check(_capi.load_library().ot_scene_read_hot_steps(handle, buf.ctypes.data, buf.nbytes, C.byref(n)))
    assert n.value == n_steps + 1
    tab = buf.reshape(-1, HOT_WORDS)
    assert not tab[-1].any(), "the record behind the last step is zeroed padding"
    return tab[:-1, 1].copy()


def hot_steps(RT, on: int) -> None:
    """Flip the switch of the tracer's scene and see on the device that it took."""
    handle, n_steps = RT._scene_handle, RT._scene.nt - 1
    _capi.check(_capi.load_library().ot_scene_set_hot_steps(handle, on))
    forms = device_forms(handle, n_steps)
    if on:
        assert forms.any() and forms[-1] == _capi.HOT_OTHER  # (every scene here has a hot step; the end aperture is OTHER)
    else:
        assert not forms.any()


def planes(RT) -> dict:
    """Every plane of the storage (reading them runs the fills with the scene as it is now), copied."""
    r = RT.rays
    out = dict(p=r.p_list.copy(), w=r.w_list.copy(), n=r.n_list.copy(), s=r.s0_list.copy(), wl=r.wl_list.copy(),
               msgs=RT._msgs.copy())
    if not RT.no_pol:
        out["pol"] = r.pol_list.copy()
    return out


def assert_same(a: dict, b: dict, what: str) -> None:
    assert a.keys() == b.keys()
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].tobytes() == b[k].tobytes(), f"{what}: {k} differs between hot steps on and off"


def on_and_off(RT, N: int, **kw) -> tuple:
    with ot.global_options.no_warnings():
        RT.trace(N, **kw)
        assert not RT.geometry_error
        handle = RT._scene_handle.value
        on = planes(RT)
        hot_steps(RT, 0)
        try:
            RT.trace(N, **kw)
            off = planes(RT)
            assert RT._scene_handle.value == handle, "the second trace ran on the scene whose forms were switched off"
        finally:
            hot_steps(RT, 1)
    return on, off


def test_forms_of_the_scenes():
    lib = _capi.load_library()
    for name, forms in FORMS.items():
        with ot.global_options.no_warnings():
            sc = CompiledScene(build(name))
        n, size = C.c_int32(), C.c_int32()
        buf = np.zeros((len(forms) + 1) * 48, dtype=np.int32)
        assert lib.ot_scene_records_host(C.byref(sc.desc), 0, 1, buf.ctypes.data, buf.nbytes, C.byref(n), C.byref(size)) == 0
        assert (n.value, size.value) == (len(forms) + 1, 192)
        assert buf.reshape(-1, 48)[:-1, 1].tolist() == forms, name


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("name,spectrum", SCENES)
def test_hot_steps_on_equal_off_and_the_oracle(name, spectrum, N):
    RT = build(name, spectrum)
    on, off = on_and_off(RT, N)
    assert_same(on, off, "generated rays")
    assert RT._scene.desc.n_lines == (3 if spectrum != "formulas" else 0)
    w = on["w"]
    assert (w[:, 0] > 0).all() and (w[:, -1] == 0).all()
    assert (w[:, -2] > 0).any() and (w[:, 1] == 0).any(), "some rays reach the last section, some end at the first surface"

    # the same rays handed in: the kernels that load section 0 and evaluate the formulas per ray
    d = on["p"][:, 1] - on["p"][:, 0]
    s0 = d / np.linalg.norm(d, axis=1)[:, None]
    init = (on["p"][:, 0].copy(), s0, on["pol"][:, 0].copy(), on["w"][:, 0].copy(), on["wl"].copy())
    RT2 = build(name, spectrum)
    ion, ioff = on_and_off(RT2, N, _initial_rays=init)
    assert_same(ion, ioff, "handed-in rays")
    sc = CompiledScene(RT2)
    rays = ob.HostRays(N, sc.nt, False)
    rays.set_initial(*init)
    msgs, st = ob.trace(sc.desc, rays, None)
    assert st == 0
    assert np.array_equal(msgs, ion["msgs"]), f"counters differ:\n{msgs}\n{ion['msgs']}"
    assert np.array_equal(rays.w_list > 0, ion["w"] > 0), "alive masks per section must be bit-exact"
    assert_close(ion["p"], rays.p_list, rtol=1e-11, atol=1e-11, what="p_list")
    assert_close(ion["w"], rays.w_list, rtol=1e-6, atol=1e-15, what="w_list")


@pytest.mark.parametrize("N", SIZES)
def test_no_pol_trace_on_equals_off(N):
    on, off = on_and_off(build("three", no_pol=True), N)
    assert_same(on, off, "no_pol")


def tail_records(RT, N: int) -> np.ndarray:
    tail = TailStorage()
    RT.trace(N, _tail=tail)
    cap, n = tail._cap, tail.N
    p = tail._dev["p"].view(3, 2, cap)[:, :, :n].cpu().numpy()
    tw = tail._dev["w"].view(2, cap)[:, :n].cpu().numpy()
    twl = tail._dev["wl"][:n].cpu().numpy()
    live = tw[0] > 0
    assert int(live.sum()) == tail.alive > 0
    a = np.concatenate([p[:, 0, live].T, p[:, 1, live].T, tw[0, live, None].astype(np.float64),
                        twl[live, None].astype(np.float64)], axis=1)
    return a[np.lexsort(a.T[::-1])], RT._msgs.copy()


def test_render_only_trace_on_equals_off():
    RT = build("three")
    with ot.global_options.no_warnings():
        RT.trace(4096)  # (compiles the scene)
        a, ma = tail_records(RT, 4096)
        hot_steps(RT, 0)
        try:
            b, mb = tail_records(RT, 4096)
        finally:
            hot_steps(RT, 1)
    assert a.tobytes() == b.tobytes() and np.array_equal(ma, mb)


def test_polarisation_fill_on_equals_off():
    """The replay behind `pol_list` (`ot_rays_fill_pol`) with the hot steps off fills what the trace with them on left out."""
    RT = build("three")
    with ot.global_options.no_warnings():
        RT.trace(4096)
        ref = RT.rays.pol_list.copy()
        RT.trace(4096)  # the planes are pending again
        hot_steps(RT, 0)
        try:
            got = RT.rays.pol_list.copy()
        finally:
            hot_steps(RT, 1)
    assert np.isfinite(ref[:, 0]).all() and ref.tobytes() == got.tobytes()


# ---- one-step scenes: a description of a single aperture, straight through the C-ABI -----------------------------------------
def one_step_desc(kind: str):
    from test_hot_step_host import Desc
    with ot.global_options.no_warnings():
        if kind == "ring":
            sf, form = ot.RingSurface(r=3., ri=0.9), _capi.HOT_RING
        elif kind == "disc":
            sf, form = ot.CircularSurface(r=1.4), _capi.HOT_FLAT
        else:
            sf, form = ot.RectangularSurface(dim=[2., 1.]), _capi.HOT_OTHER
            sf.rotate(20.)
        sf.move_to([0.2, 0.1, 3.])
        d = Desc([(sf._desc(), _capi.EL_APERTURE, 0.0)])
    d.desc.n0, d.desc.no_pol, d.desc.use_hurb, d.desc.n_lines = 0, 0, 0, 0
    d.desc.outline[:] = [-6., 6., -6., 6., -12., 40.]
    return d, form


def handed_in_rays(N: int):
    rng = np.random.default_rng(N)
    r, ph = 2.8 * np.sqrt(rng.uniform(0, 1, N)), rng.uniform(0, 2 * np.pi, N)
    p0 = np.stack([0.1 + r * np.cos(ph), -0.05 + r * np.sin(ph), np.full(N, -10.)], axis=1)
    th, a = np.radians(4) * np.sqrt(rng.uniform(0, 1, N)), rng.uniform(0, 2 * np.pi, N)
    s0 = np.stack([np.sin(th) * np.cos(a), np.sin(th) * np.sin(a), np.cos(th)], axis=1)
    pol = np.cross(s0, [0., 1., 0.])
    pol /= np.linalg.norm(pol, axis=1)[:, None]
    w0 = np.ones(N, dtype=np.float32)
    w0[3::8] = 0  # rays without power ride along
    wl = rng.choice(np.array([486.1327, 587.5618, 656.272], dtype=np.float32), N)
    return p0, s0, pol, w0, wl


def device_trace(handle, host: "ob.HostRays") -> dict:
    """`ot_trace` on device copies of a host storage whose section 0 is set; every plane and the counters back on the host."""
    lib = _capi.load_library()
    N, nt = host.N, host.nt
    dev = {k: torch.from_numpy(getattr(host, k).copy()).cuda() for k in ("p", "s", "w", "n", "wl", "pol")}
    r = _capi.Rays()
    r.N, r.nt = N, nt
    for k, t in dev.items():
        setattr(r, k, t.data_ptr())
    msgs = torch.zeros(5 * nt + 1, dtype=torch.int64, device="cuda")
    _capi.check(lib.ot_trace(handle, C.byref(r), None, 1, msgs.data_ptr(), None))
    torch.cuda.synchronize()
    out = {k: t.cpu().numpy() for k, t in dev.items()}
    out["msgs"] = msgs.cpu().numpy()
    return out


@pytest.mark.parametrize("N", SIZES)
@pytest.mark.parametrize("kind", ["ring", "disc", "rect"])
def test_one_step_scene_on_equals_off_and_the_oracle(kind, N):
    lib = _capi.load_library()
    d, form = one_step_desc(kind)
    handle = C.c_void_p()
    _capi.check(lib.ot_scene_create(C.byref(d.desc), C.byref(handle)))
    try:
        nt = lib.ot_scene_sections(handle)
        assert nt == 2, "one step: two sections"
        assert device_forms(handle, 1).tolist() == [form]
        init = handed_in_rays(N)

        def storage():
            h = ob.HostRays(N, nt, False)
            h.set_initial(*init)
            return h

        on = device_trace(handle, storage())
        _capi.check(lib.ot_scene_set_hot_steps(handle, 0))
        assert device_forms(handle, 1).tolist() == [_capi.HOT_OTHER]
        off = device_trace(handle, storage())
        _capi.check(lib.ot_scene_set_hot_steps(handle, 1))
        assert device_forms(handle, 1).tolist() == [form]
        assert_same(on, off, f"one step, {kind}")
        ref = storage()
        msgs, st = ob.trace(d.desc, ref, None)
        assert st == 0
        assert on["msgs"][-1] == 0 and np.array_equal(on["msgs"][:-1].reshape(5, nt), msgs)
        w = on["w"].reshape(nt, N).T
        assert np.array_equal(w > 0, ref.w_list > 0), "alive masks per section must be bit-exact"
        assert (w[:, 1] > 0).any() and (w[init[3] > 0, 1] == 0).any(), "the aperture passes some rays and absorbs some"
        assert_close(on["p"].reshape(3, nt, N).transpose(2, 1, 0), ref.p_list, rtol=1e-11, atol=1e-11, what="p_list")
        assert_close(w, ref.w_list, rtol=1e-6, atol=1e-15, what="w_list")
    finally:
        lib.ot_scene_destroy(handle)
