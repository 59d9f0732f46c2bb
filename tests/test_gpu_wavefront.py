"""Raytracer.wavefront_analysis and the `ot_wavefront_*` entry points on the GPU.

Truth is NumPy longdouble following the definition (tests/wavefront_cases.py): on the device's own ray storage read back, on the
reference's recorded arrays (tests/golden/trace_*.npz) for rays injected into the device trace, and on synthetic lists.

Bounds.  Per ray, optical path and pupil coordinates carry the bounds stated with the feature, formed from the truth's own
magnitudes (`wavefront_cases.paths`).  Every reduced sum is held to (n + 40) eps sum |terms|, which holds for n terms of 40
operations added in any order; what counts as a term is said in wavefront_cases.py.  Each pass is measured on the inputs it was
given: the sums of a later pass are formed, in longdouble, from the planes and the record that the device's earlier passes left,
so that a rounding of 1e-14 mm in a 50 mm path, or in its mean, is an input of the later pass and not its error.  For the same
reason the end-to-end coefficients are compared with the longdouble solution of the normal equations formed from the planes the
device produces for the focus and radius it reports, about the mean, centre and pupil radius it reports -- each of which is
checked on its own against the truth.  One comparison stays independent of the device's planes: the coefficients, the mean path
and the RMS against the whole definition in longdouble on the storage's arrays, within a bound that carries what float64 planes
cannot hold (`check_against_independent_truth`)."""
import ctypes as C
import functools
import warnings

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd import wavefront as wf
from optrace_amd._device import ptr, stream_ptr, to_dev
from optrace_amd._warn import OptraceWarning
from optrace_amd.ray_storage import RayStorage

import scenes
import wavefront_cases as wc
from helpers import load
from wavefront_cases import check_empty

pytestmark = pytest.mark.gpu

EPS = wc.EPS
LD = wc.LD
d3 = C.c_double * 3


@functools.lru_cache(maxsize=None)
def traced(name):
    """(fixture, Raytracer with the fixture's rays traced on the device, as test_gpu_parity.py::gpu_trace injects them), once per
    scene: the analyses change nothing."""
    g = load(f"trace_{name}.npz")
    with ot.global_options.no_warnings():
        RT = {**scenes.SCENES, **scenes.SCENES2}[name][0](ot)
        hn = g["hurb_normals"] if "hurb_normals" in g else None
        RT.trace(int(g["N"]), _initial_rays=(g["p0"], g["s0"], g["pol0"], g["w0"], g["wl"]), _hurb_normals=hn, _N_list=g["N_list"])
    assert not RT.geometry_error
    return g, RT


# ---- the entry points, device tensors in and host arrays out ------------------------------------------------------------------
def dev():
    return torch.device("cuda", torch.cuda.current_device())


def call_focus(rays, first, count, k, origin):
    lib = _capi.load_library()
    ws = torch.empty(_capi.WF_WS, dtype=torch.float64, device=dev())
    out = torch.full((_capi.WF_FOCUS_M,), np.nan, dtype=torch.float64, device=dev())
    _capi.check(lib.ot_wavefront_focus(C.byref(rays._rays_struct()), first, count, k, d3(*origin), ptr(ws), ptr(out), stream_ptr()))
    return out.cpu().numpy()


def call_paths(rays, first, count, k, focus, radius):
    """-> (u, v, opl, w_out as device tensors, n_missed)"""
    lib = _capi.load_library()
    rays._dev["n"]  # (through the hook: fills a stale index plane)
    u, v, opl = (torch.full((count,), -7.0, dtype=torch.float64, device=dev()) for _ in range(3))
    w = torch.full((count,), -7.0, dtype=torch.float32, device=dev())
    missed = torch.full((1,), 99, dtype=torch.int64, device=dev())
    _capi.check(lib.ot_wavefront_paths(C.byref(rays._rays_struct()), first, count, k, d3(*(float(c) for c in focus)), float(radius),
                                       ptr(u), ptr(v), ptr(opl), ptr(w), ptr(missed), stream_ptr()))
    return u, v, opl, w, int(missed.cpu()[0])


def call_moments(u, v, opl, w, wl=None):
    lib = _capi.load_library()
    ws = torch.empty(_capi.WF_WS, dtype=torch.float64, device=dev())
    mom = torch.full((_capi.WF_M,), np.nan, dtype=torch.float64, device=dev())
    _capi.check(lib.ot_wavefront_moments(u.shape[0], ptr(u), ptr(v), ptr(opl), ptr(w), ptr(wl), ptr(ws), ptr(mom), stream_ptr()))
    return mom


def call_map(u, v, opl, w, mom, pupil_radius, n_grid):
    lib = _capi.load_library()
    out = torch.zeros(2 * n_grid * n_grid, dtype=torch.float64, device=dev())
    pr = np.nan if pupil_radius is None else pupil_radius
    _capi.check(lib.ot_wavefront_map(u.shape[0], ptr(u), ptr(v), ptr(opl), ptr(w), ptr(mom), pr, n_grid, ptr(out), stream_ptr()))
    return out.cpu().numpy().reshape(2, n_grid, n_grid)


def call_zernike(u, v, opl, w, mom, pupil_radius, J):
    lib = _capi.load_library()
    ws = torch.empty(_capi.WF_WS, dtype=torch.float64, device=dev())
    out = torch.full((J * (J + 1) // 2 + J,), np.nan, dtype=torch.float64, device=dev())
    pr = np.nan if pupil_radius is None else pupil_radius
    _capi.check(lib.ot_wavefront_zernike(u.shape[0], ptr(u), ptr(v), ptr(opl), ptr(w), ptr(mom), pr, J, ptr(ws), ptr(out), stream_ptr()))
    return out.cpu().numpy()


def within(got, want, bound, what):
    got, want, bound = (np.ravel(a) for a in np.broadcast_arrays(np.asarray(got, dtype=LD), np.asarray(want, dtype=LD),
                                                                  np.asarray(bound, dtype=LD)))
    err = np.abs(got - want)
    worst = int(np.argmax(err - bound))
    print(f"{what}: largest error {float(err.max()):.3e}; closest to its bound {float(err[worst]):.3e} of {float(bound[worst]):.3e}")
    assert np.all(err <= bound), f"{what}: error {float(err[worst]):.3e} above {float(bound[worst]):.3e} ({got[worst]!r} for {want[worst]!r})"


def check_reductions(u, v, opl, w, wl, J, n_grid, pupil_radius=None):
    """Moments, normal equations and map totals of the planes (device tensors) against the truth formed from the same planes.
    -> (record, G, g) of the device."""
    hu, hv, hl, hw = (t.cpu().numpy() for t in (u, v, opl, w))
    hwl = None if wl is None else wl.cpu().numpy()
    mom_d = call_moments(u, v, opl, w, wl)
    mom = mom_d.cpu().numpy()
    assert np.array_equal(mom, call_moments(u, v, opl, w, wl).cpu().numpy()), "two calls, different bits"
    val, mag = wc.first_moments(hu, hv, hl, hw, hwl)
    n = int(val[1])
    assert mom[1] == n
    within(mom[[0, 2, 3, 4, 5]], val[[0, 2, 3, 4, 5]], wc.sum_bound(n, mag[[0, 2, 3, 4, 5]]), "first moments")
    if not n:
        assert mom[6] == np.inf and mom[7] == -np.inf and mom[8] == 0 and mom[9] == 0 and mom[10] == 0
        return mom, None, None
    assert mom[6] == val[6] and mom[7] == val[7], "minimum and maximum are entries of the list"
    s2, s2_mag, r2 = wc.central_moments(hu, hv, hl, hw, mom)
    within(mom[8], s2, wc.sum_bound(n, s2_mag), "sum w opd^2")
    within(mom[9], r2, 8 * EPS * r2, "largest squared pupil distance")
    within(mom[10], np.sqrt(LD(mom[9])), 2 * EPS * mom[10], "pupil radius: the root of the slot before it")

    packed = call_zernike(u, v, opl, w, mom_d, pupil_radius, J)
    assert np.array_equal(packed, call_zernike(u, v, opl, w, mom_d, pupil_radius, J)), "two calls, different bits"
    G, g = wf.unpack_normal_equations(packed, J)
    Gt, Ga, gt, ga, cnt = wc.normal_equations(hu, hv, hl, hw, mom, pupil_radius, J)
    within(G, Gt, wc.sum_bound(cnt, Ga), "G")
    within(g, gt, wc.sum_bound(cnt, ga), "g")

    sums = call_map(u, v, opl, w, mom_d, pupil_radius, n_grid)
    mw, mo, ma = wc.pupil_map(hu, hv, hl, hw, mom, pupil_radius, n_grid)
    within(sums[0].sum(), mw.sum(), wc.sum_bound(cnt, mw.sum()), "map: total weight")
    within(sums[1].sum(), mo.sum(), wc.sum_bound(cnt, ma.sum()), "map: total w opd")
    assert np.count_nonzero(sums[0]) <= cnt and np.all(sums[0] >= 0)
    return mom, G, g


# ---- 1. entry points on the device's own storage ------------------------------------------------------------------------------
CASES = [("c1_single_lens", 0, None), ("c1_single_lens", 0, 1), ("double_gauss", 0, None), ("double_gauss", 2, None),
         ("double_gauss", 4, None), ("prism", 0, None)]


def storage_case(name, source, section):
    g, RT = traced(name)
    rays = RT.rays
    p, n, w = rays.p_list, rays.n_list, rays.w_list
    first, end = int(rays.B_list[source]), int(rays.B_list[source + 1])
    k = rays.Nt - 2 if section is None else section
    return RT, p, n, w, first, end, k


@pytest.mark.parametrize("name,source,section", CASES)
def test_entry_points_on_the_devices_own_storage(name, source, section):
    RT, p, n, w, first, end, k = storage_case(name, source, section)
    rays, count = RT.rays, end - first
    origin = np.array(p[first, k])
    val, mag, n_used = wc.focus_sums(p, w, k, first, end, origin)
    sums = call_focus(rays, first, count, k, origin)
    assert np.array_equal(sums, call_focus(rays, first, count, k, origin)), "two calls, different bits"
    assert sums[1] == n_used and n_used > 100
    within(sums, val, wc.sum_bound(n_used, mag), "focus sums")

    # focus and radius from the truth, so that both sides meet the same sphere
    focus, radius, cond = wc.sphere_from_sums(val, origin)
    focus, radius = focus.astype(np.float64), float(radius)
    print(name, source, "section", k, "rays used", n_used, "cond(A)", cond, "focus", focus, "radius", radius)
    if name == "prism":
        assert radius < 0
    t = wc.paths(p, n, w, k, first, end, focus, radius)
    u, v, opl, wo, missed = call_paths(rays, first, count, k, focus, radius)
    assert missed == t["n_missed"] == 0
    assert np.array_equal(wo.cpu().numpy(), t["w"].astype(np.float32)), "weights of the rays used, 0 for the others"
    for key, got in (("opl", opl), ("u", u), ("v", v)):
        got = got.cpu().numpy()
        assert np.array_equal(np.isnan(got), np.isnan(t[key].astype(np.float64))), f"{key}: NaN exactly where a ray is not used"
        ok = ~np.isnan(got)
        within(got[ok], t[key][ok], t["b_" + key][ok], key)
    check_reductions(u, v, opl, wo, rays._dev["wl"][first:end], 15, 16)


# ---- 2. end to end, defaults everywhere ----------------------------------------------------------------------------------------
def check_against_own_planes(RT, wa, source, J=15):
    """The figures of `wa` that follow the sphere, from the planes the device forms for the sphere `wa` reports (module docstring)."""
    rays = RT.rays
    first, end = (int(rays.B_list[source]), int(rays.B_list[source + 1])) if source is not None else (0, rays.N)
    u, v, opl, w, missed = call_paths(rays, first, end - first, wa.section, wa.focus, wa.radius)
    hu, hv, hl, hw = (t.cpu().numpy() for t in (u, v, opl, w))
    assert missed == wa.n_missed
    val, mag = wc.first_moments(hu, hv, hl, hw, rays.wl_list[first:end])
    n = int(val[1])
    assert wa.N == n and isinstance(wa.N, int)
    W = val[0]
    within(wa.power, W, wc.sum_bound(n, mag[0]), "power")
    # (a quotient of two sums: the numerator's bound over W, and as much again for W's own, since |sum w a| <= sum w |a|)
    for key, slot in (("opl_mean", 2), ("wavelength", 5)):
        within(getattr(wa, key), val[slot] / W, 2 * wc.sum_bound(n, mag[slot]) / W, key)
    within(wa.pupil_centre, val[3:5] / W, 2 * wc.sum_bound(n, mag[3:5]) / W, "pupil centre")
    # about the means that `wa` reports
    mom = np.array([1.0, n, wa.opl_mean, wa.pupil_centre[0], wa.pupil_centre[1], 0, 0, 0, 0, wa.pupil_radius ** 2, wa.pupil_radius])
    s2, s2_mag, r2 = wc.central_moments(hu, hv, hl, hw, mom)
    within(wa.rms, np.sqrt(s2 / W), 4 * EPS * np.sqrt(s2 / W) + wc.sum_bound(n, s2_mag) / (W * np.sqrt(s2 / W)), "rms")
    within(wa.pupil_radius, np.sqrt(r2), 8 * EPS * np.sqrt(r2), "pupil radius")
    assert wa.opd_min == val[6].astype(np.float64) - wa.opl_mean and wa.opd_max == val[7].astype(np.float64) - wa.opl_mean
    assert wa.pv == wa.opd_max - wa.opd_min
    Gt, _, gt, _, cnt = wc.normal_equations(hu, hv, hl, hw, mom, None, J, pr=wa.pupil_radius)
    assert cnt == n
    G64 = Gt.astype(np.float64)
    a = np.linalg.solve(G64, gt.astype(np.float64))
    cond = np.linalg.cond(G64)
    print("cond(G)", cond, "largest coefficient", np.abs(a).max(), "rms", wa.rms, "waves", wa.rms_waves, "strehl", wa.strehl)
    within(wa.zernike, a, cond * 64 * EPS * np.abs(a).max(), "zernike")
    # the map: every ray in one cell, the cells' weighted OPD adds up to nothing
    assert wa.weight_map.shape == wa.opd_map.shape
    within(wa.weight_map.sum(), W, wc.sum_bound(n, mag[0]), "map: total weight")
    assert np.array_equal(np.isnan(wa.opd_map), wa.weight_map == 0)
    filled = wa.weight_map > 0
    assert np.all(wa.opd_map[filled] >= wa.opd_min - 1e-15) and np.all(wa.opd_map[filled] <= wa.opd_max + 1e-15)
    return a


def check_against_independent_truth(wa, p, n, w, k, first, end, focus, radius, cond_A, J=15):
    """The coefficients once more, against a truth that takes nothing from the device: the whole definition in longdouble on the
    storage's arrays, with the truth's own sphere, means and pupil.  The bound is loose, because it has to carry what float64
    planes cannot hold.  With d_sphere = cond(A) 64 eps (1 + |c|) for the focus and as much for the radius (the bounds of those
    two above), a ray's path may differ by its per-ray bound b_opl plus n_k 2 d_sphere (|o| + |R|) / sqrt(D) for the moved sphere
    (the sphere step's derivative with respect to c and R, as in the parity bound of the feature), and its OPD by twice the largest
    of these, D_opd, because the mean moves as well.  Its pupil coordinates may differ by d_xy = (4 max(b_u, b_v) + 4 d_sphere / |R|)
    / pupil radius (its own bound, the centre's, the radius', the moved sphere), which changes sum_j a_j Z_j by at most
    J |a|_max L d_xy with L = 16 sqrt(10) >= |grad Z_j| on the disc for j <= 15.  A weighted least-squares fit maps a change of
    the data of weighted RMS e to a change of the coefficients of norm at most e / sqrt(lambda_min(G / W)); the float64 solve adds
    cond(G) 64 eps |a|_max."""
    t = wc.paths(p, n, w, k, first, end, focus.astype(np.float64), float(radius))
    val, _ = wc.first_moments(t["u"], t["v"], t["opl"], t["w"])
    W = val[0]
    mom = np.zeros(11, dtype=LD)
    mom[:8] = val
    mom = mom.astype(np.float64)
    _, _, r2 = wc.central_moments(t["u"], t["v"], t["opl"], t["w"], mom)
    mom[9], mom[10] = r2, np.sqrt(r2)
    Gt, _, gt, _, cnt = wc.normal_equations(t["u"], t["v"], t["opl"], t["w"], mom, None, J)
    assert cnt == wa.N
    a = _solve_ld(Gt, gt).astype(np.float64)
    G64 = Gt.astype(np.float64)
    lam_min = np.linalg.eigvalsh(G64 / float(W)).min()
    a_max = np.abs(a).max()
    used = t["w"] > 0
    d_sphere = cond_A * 64 * EPS * (1 + np.abs(focus).max())
    moved = t["n_max"] * 2 * d_sphere * (t["o"][used] + abs(radius)) / np.sqrt(t["D"][used])
    d_opd = 2 * float((t["b_opl"][used] + moved).max())
    d_xy = (4 * float(max(t["b_u"][used].max(), t["b_v"][used].max())) + 4 * d_sphere / abs(float(radius))) / mom[10]
    bound = (d_opd + J * a_max * 16 * np.sqrt(10) * d_xy) / np.sqrt(lam_min) + np.linalg.cond(G64) * 64 * EPS * a_max
    print("independent truth: lambda_min(G / W)", lam_min, "d_opd", d_opd, "d_xy", float(d_xy))
    within(wa.zernike, a, bound, "zernike against the independent truth")
    within(wa.opl_mean, val[2] / W, d_opd, "opl_mean against the independent truth")
    within(wa.rms, np.sqrt(wc.central_moments(t["u"], t["v"], t["opl"], t["w"], mom)[0] / W), d_opd, "rms against the independent truth")


@pytest.mark.parametrize("name,source,section", CASES)
def test_wavefront_analysis_end_to_end(name, source, section):
    RT, p, n, w, first, end, k = storage_case(name, source, section)
    with ot.global_options.no_warnings():
        wa = RT.wavefront_analysis(source) if section is None else RT.wavefront_analysis(source, section=section)
    origin = np.array(p[first, k])
    val, mag, n_used = wc.focus_sums(p, w, k, first, end, origin)
    focus, radius, cond = wc.sphere_from_sums(val, origin)
    assert isinstance(wa, ot.WavefrontAnalysis) and wa.section == k and wa.N == n_used and wa.n_missed == 0
    within(wa.focus, focus, cond * 64 * EPS * (1 + np.abs(focus).max()), "focus")
    # |R| = |c - pbar|: the focus' error and the rounding of the mean start
    within(wa.radius, radius, cond * 64 * EPS * (1 + np.abs(focus).max()) + 64 * EPS * (1 + np.abs(origin).max()), "radius")
    assert wa.zernike.shape == (15,) and wa.opd_map.shape == (64, 64) and not wa.zernike.flags.writeable
    check_against_own_planes(RT, wa, source)
    check_against_independent_truth(wa, p, RT.rays.n_list, w, k, first, end, focus, radius, cond)
    # a second call returns the same bits where the order of the additions is fixed
    with ot.global_options.no_warnings():
        wb = RT.wavefront_analysis(source) if section is None else RT.wavefront_analysis(source, section=section)
    for key in ("N", "power", "radius", "rms", "pv", "opl_mean", "wavelength", "pupil_radius"):
        assert getattr(wa, key) == getattr(wb, key), key
    assert np.array_equal(wa.focus, wb.focus) and np.array_equal(wa.zernike, wb.zernike)


def test_ideal_lens_before_the_section_warns_and_still_returns(monkeypatch):
    g, RT = traced("hurb_ring_ideal")
    # (the switch is process-wide, and threads that leave `no_warnings` in another order than they entered it -- the workers of
    # test_gpu_threads.py -- can leave it off: this test is about a warning, so it says what it needs)
    monkeypatch.setattr(ot.global_options, "show_warnings", True)
    with pytest.warns(UserWarning, match="ideal lens"):
        wa = RT.wavefront_analysis(0)
    assert wa.N > 100 and wa.n_missed == 0 and np.isfinite(wa.rms) and np.all(np.isfinite(wa.zernike))
    p, w = RT.rays.p_list, RT.rays.w_list
    k = RT.rays.Nt - 2
    val, _, n_used = wc.focus_sums(p, w, k, 0, RT.rays.N, np.array(p[0, k]))
    focus, radius, cond = wc.sphere_from_sums(val, np.array(p[0, k]))
    print("cond(A)", cond)
    assert wa.N == n_used
    within(wa.focus, focus, cond * 64 * EPS * (1 + np.abs(focus).max()), "focus")
    check_against_own_planes(RT, wa, 0)
    with warnings.catch_warnings():  # (section 0 lies before the lens: nothing to warn about)
        warnings.simplefilter("error", category=OptraceWarning)
        RT.wavefront_analysis(0, section=0, focus=[0, 0, -50], radius=-40.0)


# ---- 3. against the reference's recorded arrays ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c1_single_lens", "double_gauss"])
def test_against_the_reference_recorded_arrays(name):
    g, RT = traced(name)
    p, n, w = g["p_list"], g["n_list"], g["w_list"]
    first, end = 0, int(g["N_list"][0])
    k = p.shape[1] - 2
    origin = np.array(p[first, k])
    val, _, n_used = wc.focus_sums(p, w, k, first, end, origin)
    focus, radius, _ = wc.sphere_from_sums(val, origin)
    focus, radius = focus.astype(np.float64), float(radius)
    t = wc.paths(p, n, w, k, first, end, focus, radius)
    assert t["n_missed"] == 0
    used = t["w"] > 0
    W = t["w"][used].sum()
    opd_t = t["opl"][used] - (t["w"][used] * t["opl"][used]).sum() / W
    dp = 1e-11 * (1 + np.abs(p).max())  # what test_gpu_parity grants positions
    bound = t["n_max"] * dp * (2 * (k + 1) + 2 * (t["o"][used] + abs(radius)) / np.sqrt(t["D"][used]))

    u, v, opl, wo, missed = call_paths(RT.rays, first, end - first, k, focus, radius)
    hl, hw = opl.cpu().numpy(), wo.cpu().numpy()
    assert missed == 0 and np.array_equal(hw > 0, used), "the same rays are used"
    hl, hw = hl[used].astype(LD), hw[used].astype(LD)
    opd_d = hl - (hw * hl).sum() / hw.sum()
    within(opd_d, opd_t, bound, "per-ray OPD")

    with ot.global_options.no_warnings():
        wa = RT.wavefront_analysis(0, focus=focus, radius=radius)
    rms_t = np.sqrt((t["w"][used] * opd_t ** 2).sum() / W)
    print(name, "rays", n_used, "radius", radius, "rms", float(rms_t), "device", wa.rms, "pv", wa.pv)
    assert wa.N == n_used and np.array_equal(wa.focus, focus) and wa.radius == radius
    within(wa.rms, rms_t, 2 * bound.max(), "rms")
    within(wa.pv, opd_t.max() - opd_t.min(), 2 * bound.max(), "pv")


# ---- 4. synthetic lists ----------------------------------------------------------------------------------------------------------
def synthetic(n, seed):
    """Random entries in a disc, a fifth of them dead: those carry NaN everywhere and weight 0."""
    rng = np.random.default_rng(seed)
    r, phi = 0.3 * np.sqrt(rng.uniform(0, 1, n)), rng.uniform(0, 2 * np.pi, n)
    u, v = 0.05 + r * np.cos(phi), -0.02 + r * np.sin(phi)
    opl = 50 + 2e-3 * (u * u + v * v) / 0.09 + 1e-4 * rng.standard_normal(n)
    w = rng.uniform(0.5, 1.5, n).astype(np.float32)
    wl = rng.uniform(400, 700, n).astype(np.float32)
    dead = rng.uniform(0, 1, n) < 0.2
    if n > 1:
        dead[0] = False
    else:
        dead[:] = False
    for a in (u, v, opl):
        a[dead] = np.nan
    w[dead] = 0
    return [to_dev(a, a.dtype) for a in (u, v, opl, w, wl)]


CAP_N = 2048 * 256 + 257  # the first size at which the cap of 2048 workgroups binds: every walker takes more than one step


@pytest.mark.parametrize("n", [1, 63, 65, 257, 70001, CAP_N])
def test_reductions_of_synthetic_lists(n):
    """Lane, wave, workgroup and grid edges, and the capped walk; dead entries hold NaN and must not reach any sum (one would turn
    it into NaN)."""
    u, v, opl, w, wl = synthetic(n, n)
    # (at CAP_N the longdouble truth of the 36-polynomial normal equations alone takes 20 s: that size runs the table of 15)
    mom, G, g = check_reductions(u, v, opl, w, wl, 36 if n < CAP_N else 15, 16)
    assert np.all(np.isfinite(mom)) and np.all(np.isfinite(G)) and np.all(np.isfinite(g))
    # the smaller table, a given pupil radius that leaves entries out, and the global-atomics path of the map
    check_reductions(u, v, opl, w, None, 7, 1024, pupil_radius=0.2)
    if n > 1:
        _, _, _, _, cnt = wc.normal_equations(*(t.cpu().numpy() for t in (u, v, opl, w)), mom, 0.2, 1)
        assert 0 < cnt < mom[1], "the given radius leaves some entries out and keeps some"


def test_all_dead_list_and_empty_list():
    nan = np.full(100, np.nan)
    u, v, opl = (to_dev(nan, np.float64) for _ in range(3))
    w = to_dev(np.zeros(100), np.float32)
    mom_d = call_moments(u, v, opl, w)
    mom = mom_d.cpu().numpy()
    assert np.array_equal(mom, [0, 0, 0, 0, 0, 0, np.inf, -np.inf, 0, 0, 0])
    assert np.array_equal(call_zernike(u, v, opl, w, mom_d, None, 15), np.zeros(135))
    assert np.array_equal(call_map(u, v, opl, w, mom_d, None, 8), np.zeros((2, 8, 8)))


def cell_centre_list(n_grid, given_radius):
    """Entries on the centres of the cells of an n_grid x n_grid pupil grid whose unit-disc coordinates are exact: the centre is
    (0, 0) by symmetry (sums of dyadic numbers are exact in any order) and the radius is 1, either given (then the cells beyond
    the disc hold dead entries) or found (then the grid is drawn at half size and four entries at distance 1 set the radius).
    OPL is an odd function of the position in whole numbers, so its mean is 0 and every sum is exact.
    -> (u, v, opl, w, expected weight map, expected w opd map)"""
    i = np.arange(n_grid)
    c = (2 * i + 1) / n_grid - 1
    x, y = np.meshgrid(c, c)  # x along columns
    ix, iy = np.meshgrid(i, i)
    odd_x, odd_y = 2 * ix + 1 - n_grid, 2 * iy + 1 - n_grid
    opl = (odd_x + 2 * odd_y).astype(np.float64)
    w = (1 + (ix + iy) % 2).astype(np.float32)
    if given_radius:
        dead = x * x + y * y > 1
        u, v = x.copy(), y.copy()
        u[dead] = v[dead] = opl[dead] = np.nan
        w[dead] = 0
        u, v, opl, w = u.ravel(), v.ravel(), opl.ravel(), w.ravel()
        wm = w.reshape(n_grid, n_grid).astype(np.float64)
        om = np.where(dead, 0.0, wm * np.nan_to_num(opl.reshape(n_grid, n_grid)))
        return u, v, opl, w, wm, om
    # half size: the entries fall into the middle cells of the grid, (x + 1) / 2 * n_grid = n_grid / 4 + (2 i + 1) / 4
    u = np.concatenate([(x / 2).ravel(), [1, -1, 0, 0]])
    v = np.concatenate([(y / 2).ravel(), [0, 0, 1, -1]])
    l = np.concatenate([opl.ravel(), [3, -3, 5, -5]])
    ww = np.concatenate([w.ravel(), np.ones(4, dtype=np.float32)])
    wm, om = np.zeros((n_grid, n_grid)), np.zeros((n_grid, n_grid))
    cx = np.minimum(np.floor((u + 1) / 2 * n_grid), n_grid - 1).astype(int)
    cy = np.minimum(np.floor((v + 1) / 2 * n_grid), n_grid - 1).astype(int)
    np.add.at(wm, (cy, cx), ww)
    np.add.at(om, (cy, cx), ww * l)
    return u, v, l, ww, wm, om


@pytest.mark.parametrize("n_grid", [8, 64])
@pytest.mark.parametrize("given_radius", [True, False])
def test_map_is_exact_cell_by_cell(n_grid, given_radius):
    u, v, opl, w, wm, om = cell_centre_list(n_grid, given_radius)
    # three copies of the list: several entries per cell, and more entries than one workgroup walks
    tu, tv, tl = (to_dev(np.tile(a, 3), np.float64) for a in (u, v, opl))
    tw = to_dev(np.tile(w, 3), np.float32)
    mom_d = call_moments(tu, tv, tl, tw)
    mom = mom_d.cpu().numpy()
    assert mom[2] == 0 and mom[3] == 0 and mom[4] == 0 and mom[0] == 3 * w.astype(np.float64).sum()
    if not given_radius:
        assert mom[9] == 1 and mom[10] == 1
    sums = call_map(tu, tv, tl, tw, mom_d, 1.0 if given_radius else None, n_grid)
    assert np.array_equal(sums[0], 3 * wm), "weights: row from v, column from u"
    assert np.array_equal(sums[1], 3 * om)
    assert not np.array_equal(wm, wm.T) or not np.array_equal(om, om.T), "(the case tells rows from columns)"


def stratified_disc():
    """4096 disc points, symmetric about the centre and on a 2^-20 grid (their sums are exact: the pupil centre is (0, 0)), and the
    centre itself."""
    i, j = np.meshgrid(np.arange(32), np.arange(64), indexing="ij")
    r, phi = np.sqrt((i + 0.5) / 32), (j + 0.5) * np.pi / 64  # the upper half
    x, y = np.round(r * np.cos(phi) * 2 ** 20) / 2 ** 20, np.round(r * np.sin(phi) * 2 ** 20) / 2 ** 20
    x, y = np.concatenate([x.ravel(), -x.ravel(), [0.0]]), np.concatenate([y.ravel(), -y.ravel(), [0.0]])
    return x, y


@pytest.mark.parametrize("J", [15, 22, 36])
def test_zernike_recovery(J):
    """OPD = a known combination of Z_4, Z_7, Z_11 and Z_22 in the pupil the device finds.  With J >= 22 the combination lies in the
    span and the fit returns it, whatever the points; with J = 15 the fit is the longdouble least-squares solution on these points
    (Z_22 is not orthogonal to the others on a finite set).  The device subtracts the mean: Z_1 takes minus the mean."""
    known = {4: 1.5e-3, 7: -4e-4, 11: 2.5e-4, 22: -1e-4}
    x, y = stratified_disc()
    scale = 0.125  # pupil coordinates of a bundle: the disc of radius `scale` times the largest |point|
    xl, yl = x.astype(LD), y.astype(LD)
    rmax = np.sqrt((xl * xl + yl * yl).max())
    opd = sum(a * wc.zernike_ld(j, xl / rmax, yl / rmax) for j, a in known.items()).astype(np.float64)
    u, v, opl = (to_dev(a, np.float64) for a in (x * scale, y * scale, opd))
    w = to_dev(np.ones(x.shape[0]), np.float32)
    mom_d = call_moments(u, v, opl, w)
    mom = mom_d.cpu().numpy()
    assert mom[3] == 0 and mom[4] == 0, "the centre entry lies at the exact pupil centre"
    packed = call_zernike(u, v, opl, w, mom_d, None, J)
    G, g = wf.unpack_normal_equations(packed, J)
    got = np.linalg.solve(G, g)
    Gt, _, gt, _, cnt = wc.normal_equations(x * scale, y * scale, opd, np.ones(x.shape[0]), mom, None, J)
    assert cnt == 4097
    cond = np.linalg.cond(Gt.astype(np.float64))
    bound = cond * 64 * EPS * max(abs(a) for a in known.values())
    print("J", J, "cond(G)", cond, "bound", bound)
    if J >= 22:
        want = np.zeros(J)
        for j, a in known.items():
            want[j - 1] = a
        want[0] = -mom[2] / mom[0]
    else:
        want = _solve_ld(Gt, gt)
    within(got, want, bound, "coefficients")


def _solve_ld(G, g):
    """Gaussian elimination with partial pivoting in longdouble."""
    A = np.concatenate([np.array(G, dtype=LD), np.array(g, dtype=LD)[:, None]], axis=1)
    n = A.shape[0]
    for c in range(n):
        piv = c + int(np.argmax(np.abs(A[c:, c])))
        A[[c, piv]] = A[[piv, c]]
        A[c + 1:] -= (A[c + 1:, c] / A[c, c])[:, None] * A[c]
    x = np.zeros(n, dtype=LD)
    for c in range(n - 1, -1, -1):
        x[c] = (A[c, n] - A[c, c + 1:n] @ x[c + 1:]) / A[c, c]
    return x


def test_entry_points_refuse_bad_arguments_without_a_launch():
    """(the same list as without a device: the checks come first, and a refused call leaves its outputs alone)"""
    lib = _capi.load_library()
    wc.entry_point_argument_checks(lib)
    u, v, opl, w, _ = synthetic(65, 3)
    out = torch.full((16,), -3.0, dtype=torch.float64, device=dev())
    st = stream_ptr()
    assert lib.ot_wavefront_moments(65, ptr(u), ptr(v), ptr(opl), None, None, ptr(out), ptr(out), st) == -1
    mom = call_moments(u, v, opl, w)
    assert lib.ot_wavefront_zernike(65, ptr(u), ptr(v), ptr(opl), ptr(w), ptr(mom), np.nan, 37, ptr(out), ptr(out), st) == -3
    assert b"ot_wavefront_zernike" in lib.ot_last_error()
    assert lib.ot_wavefront_map(65, ptr(u), ptr(v), ptr(opl), ptr(w), ptr(mom), -1.0, 4, ptr(out), st) == -1
    assert lib.ot_wavefront_map(65, ptr(u), ptr(v), ptr(opl), ptr(w), ptr(mom), np.nan, 1025, ptr(out), st) == -3
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), np.full(16, -3.0))


# ---- 5. storage edges --------------------------------------------------------------------------------------------------------------
def lens_tracer(aim_at_aperture=False):
    RT = ot.Raytracer(outline=[-6, 6, -6, 6, -1, 60], no_pol=True, seed=11)
    RT.add(ot.RaySource(ot.CircularSurface(r=2.5), divergence="None", spectrum=ot.LightSpectrum("Lines", lines=[486.0, 656.0], line_vals=[1, 2]),
                        pos=[0, 0.3, 0], s=[0, 0.01, 1]))
    if aim_at_aperture:  # a disc that stops the whole bundle
        RT.add(ot.Aperture(ot.CircularSurface(r=5), pos=[0, 0, 4]))
    RT.add(ot.Lens(ot.SphericalSurface(r=4, R=30), ot.SphericalSurface(r=4, R=-25), n=ot.presets.refraction_index.BK7, pos=[0, 0, 8], d=1.5))
    return RT


def test_padded_storage_and_stale_index_plane(monkeypatch):
    """A generated trace of 4099 rays in planes 4224 apart, its index plane still unwritten when the analysis is asked for."""
    monkeypatch.setattr(RayStorage, "PAD_FROM", 512)
    RT = lens_tracer()
    with ot.global_options.no_warnings():
        RT.trace(4099)
        assert RT.rays._Np == 4224 and RT.rays._n_stale, "nothing here may have read the plane through the hook"
        wa = RT.wavefront_analysis(0)
        assert not RT.rays._n_stale
        wb = RT.wavefront_analysis(0)
    assert wa.N == 4099 and wa.n_missed == 0 and wa.radius > 0 and 486 < wa.wavelength < 656
    for key in ("N", "power", "radius", "rms", "pv", "opl_mean", "wavelength", "pupil_radius"):
        assert getattr(wa, key) == getattr(wb, key), key
    assert np.array_equal(wa.focus, wb.focus) and np.array_equal(wa.zernike, wb.zernike)
    # the truth from the arrays read afterwards
    p, n, w = RT.rays.p_list, RT.rays.n_list, RT.rays.w_list
    assert p.shape == (4099, 4, 3) and n.min() >= 1 and n[:, 1].min() > 1.5
    k = 2
    origin = np.array(p[0, k])
    val, _, n_used = wc.focus_sums(p, w, k, 0, 4099, origin)
    focus, radius, cond = wc.sphere_from_sums(val, origin)
    assert n_used == 4099
    within(wa.focus, focus, cond * 64 * EPS * (1 + np.abs(focus).max()), "focus")
    t = wc.paths(p, n, w, k, 0, 4099, wa.focus, wa.radius)
    u, v, opl, wo, missed = call_paths(RT.rays, 0, 4099, k, wa.focus, wa.radius)
    within(opl.cpu().numpy(), t["opl"], t["b_opl"], "opl")
    check_against_own_planes(RT, wa, 0)


def test_all_absorbed_bundle_gives_the_empty_result():
    RT = lens_tracer(aim_at_aperture=True)
    with ot.global_options.no_warnings():
        RT.trace(1000)
        wa = RT.wavefront_analysis(0, n_zernike=6, n_grid=4)
        check_empty(wa, 6, 4)
        assert wa.section == 3 and wa.n_missed == 0 and np.all(np.isnan(wa.focus)) and np.isnan(wa.radius)
        check_empty(RT.wavefront_analysis(None, focus=[0, 0, 30], radius=5.0, n_zernike=1, n_grid=1), 1, 1)
        before = RT.wavefront_analysis(0, section=0, focus=[0, 0, -100], radius=-104.0)  # (the section before the stop is alive)
    assert before.N == 1000
