"""The basis-free polarisation and Fresnel form of the refraction step (refraction_polarization, refract of
csrc/ot_trace.hpp) on the device, through the plate machinery of tests/refraction_cases.py: one plate with a flat and one
with a tilted front normal, 9001 rays per launch that are dense in sin(alpha) across the near-normal threshold
(pol_form.NEAR, a factor 16 either side), with ordinary angles, rays at and beyond the critical angle, rays that miss the
plate and dead rays among them.

  * w and pol behind the front face against per-ray exact values of the reference's formulas (mpmath) with the bars of
    tests/test_gpu_refraction_step.py (refraction_cases.w_bar, pol_bar), no others; the used fractions are printed;
  * everything discrete (counters, alive masks, total-reflection verdicts) and the direction behind the plate with the C
    oracle's bits; dead and missed rays keep their pol;
  * the kernels for SPEC 0 (constant media), 1 (tabulated medium) and 2 (discrete spectrum, rays generated in the kernel)
    agree bit for bit in w and pol;
  * no_pol weights against the exact T(1/2, 1/2);
  * one double-Gauss trace of 20 000 handed-in rays against the oracle: alive masks and counters identical, p within 1e-12,
    w within 1e-6 relative.
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd._device import stream_ptr

import pol_form as pf
import refraction_cases as rc
import scenes

pytestmark = pytest.mark.gpu
pytest.importorskip("mpmath")

TIR, MISSING = 1, 0   # Raytracer.INFOS
N_DENSE, N_WIDE, N_EDGE, N_MISSED = 6400, 2000, 129, 472
N_RAYS = N_DENSE + N_WIDE + N_EDGE + N_MISSED
DENSE, WIDE, EDGE, MISSED = range(4)
PLATES = {"flat": rc.Scene("pol_form/flat", "flat", 1.7, 1.0, (), None),
          "tilt": rc.Scene("pol_form/tilt", "tilt_a", 1.6, 1.33, (), None)}


@functools.lru_cache(maxsize=None)
def inputs(key: str) -> dict:
    sc = PLATES[key]
    rng = np.random.default_rng([20261, sorted(PLATES).index(key)])
    n, N = rc.unit_normal(sc.normal), sc.n1 / sc.n2
    near = np.sqrt(pf.NEAR)
    s_dense = pf.directions(sc.normal, near * 2.0 ** rng.uniform(-4, 4, N_DENSE), rng)
    s_wide = pf.directions(sc.normal, rng.uniform(0.05, 0.95, 6 * N_WIDE), rng)   # beyond the critical angle as well
    ns = rc._rdot(s_wide, np.broadcast_to(n, s_wide.shape))
    s_wide = s_wide[(s_wide[:, 2] >= 0.25) & (np.abs(1 - N * N * (1 - ns * ns)) >= 2.0 ** -16)][:N_WIDE]
    if sc.normal == "flat":   # the consecutive doubles around the critical angle
        s_edge = rc._directions(sc._replace(classes=("critical",)), "critical", rng)
    else:                     # sin(alpha) within a few 2^-40 of n2 / n1, either side
        s_edge = pf.directions(sc.normal, (1 / N) * (1 + rng.uniform(-1, 1, 8 * N_EDGE) * 2.0 ** -38), rng)
        s_edge = s_edge[s_edge[:, 2] >= 0.25][:N_EDGE]
    s_missed = pf.directions(sc.normal, rng.uniform(0.01, 0.3, N_MISSED), rng)
    s0 = np.concatenate((s_dense, s_wide, s_edge, s_missed))
    cls = np.repeat([DENSE, WIDE, EDGE, MISSED], [N_DENSE, N_WIDE, N_EDGE, N_MISSED])
    assert s0.shape == (N_RAYS, 3) and N_RAYS % 64 != 0 and cls.shape[0] == N_RAYS
    xy = rng.uniform(-rc.HIT_HALF_WIDTH, rc.HIT_HALF_WIDTH, (N_RAYS, 2))
    ang = rc._unit2(rng, N_MISSED)   # outside the plate's radius, inside the outline
    xy[cls == MISSED] = np.stack(ang, axis=1) * rng.uniform(3.5, 5.0, N_MISSED)[:, None]
    hit = np.column_stack((xy, -rc.D1 + xy[:, 0] * (-n[0] / n[2]) + xy[:, 1] * (-n[1] / n[2])))
    w0 = rng.uniform(0.25, 1.0, N_RAYS).astype(np.float32)
    w0[3::8] = 0.0
    return dict(p0=hit - rc.DEPTH * s0, s0=s0, pol0=pf.tilted_pol(s0, rng, along=2.0 ** -24), w0=w0,
                wl=np.full(N_RAYS, rc.WL, dtype=np.float32), cls=cls)


class Run:
    pass


@functools.lru_cache(maxsize=None)
def run(key: str, variant: str) -> Run:
    sc, inp = PLATES[key], inputs(key)
    r = Run()
    with ot.global_options.no_warnings():
        RT = rc.raytracer(ot, sc, variant)
        pol0 = None if RT.no_pol else inp["pol0"]
        RT.trace(N_RAYS, _initial_rays=(inp["p0"], inp["s0"], pol0, inp["w0"], inp["wl"]), _N_list=np.array([N_RAYS]))
        assert not RT.geometry_error
        r.p, r.w, r.s = RT.rays.p_list.copy(), RT.rays.w_list.copy(), RT.rays.s0_list.copy()
        r.pol = None if RT.no_pol else RT.rays.pol_list.copy()
        r.msgs = np.array(RT._msgs)
        r.orc, r.orc_msgs, _ = rc.oracle_trace(RT, inp)
    return r


@functools.lru_cache(maxsize=None)
def exact(key: str):
    """-> (sel, T (longdouble), pol' (longdouble), a): the live rays that meet the plate and pass it with W >= 2^-8."""
    sc, inp = PLATES[key], inputs(key)
    n = rc.unit_normal(sc.normal)
    ns = rc._rdot(inp["s0"], np.broadcast_to(n, inp["s0"].shape))
    sel = (inp["w0"] > 0) & (inp["cls"] <= WIDE) & (1 - (sc.n1 / sc.n2) ** 2 * (1 - ns * ns) >= 2.0 ** -16)
    T, pol = pf.exact(dict(n=n, s=inp["s0"][sel], pol=inp["pol0"][sel], n1=sc.n1, n2=sc.n2))
    return sel, T, pol, rc.sin_alpha(n, inp["s0"][sel])


def bits(a, b) -> bool:
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def test_inputs_cover_the_threshold_and_the_edges():
    for key, sc in PLATES.items():
        inp = inputs(key)
        a = rc.sin_alpha(rc.unit_normal(sc.normal), inp["s0"]).astype(np.float64)
        near = np.sqrt(pf.NEAR)
        live = inp["w0"] > 0
        assert np.count_nonzero(live & (a < near) & (a > near / 16.5)) > 2000
        assert np.count_nonzero(live & (a >= near) & (a < near * 16.5)) > 2000
        r = run(key, "plain")
        tir = r.orc_msgs[TIR, 0]
        assert tir > 100 and r.orc_msgs[MISSING, 1] == np.count_nonzero(live & (inp["cls"] == MISSED)) > 300
        edge = live & (inp["cls"] == EDGE)
        assert 10 < np.count_nonzero(r.orc.w_list[edge, 1] > 0) < np.count_nonzero(edge) - 10, "both sides of the critical angle"
        assert np.count_nonzero(exact(key)[0]) > 6000


@pytest.mark.parametrize("variant", ["plain", "data_medium", "no_pol"])
@pytest.mark.parametrize("key", list(PLATES))
def test_discrete_results_and_direction_are_the_oracles(key, variant):
    r, inp = run(key, variant), inputs(key)
    assert np.array_equal(r.msgs, r.orc_msgs), f"{r.msgs}\n{r.orc_msgs}"
    assert np.array_equal(r.w > 0, r.orc.w_list > 0), "alive masks"
    assert np.all(np.isfinite(r.w)) and np.all(np.isfinite(r.p))
    through = r.orc.w_list[:, -2] > 0
    assert np.count_nonzero(through) > 6000 and bits(r.s[through], r.orc.s_final[through])
    # around the critical angle the weight is the oracle's to one float32 unit (W is small there: no exact bar)
    edge = (inp["cls"] == EDGE) & (inp["w0"] > 0)
    assert np.all(rc.ulp32_distance(r.w[edge, 1], r.orc.w_list[edge, 1]) <= 1)
    if r.pol is not None:
        dead, missed = inp["w0"] == 0, (inp["cls"] == MISSED) & (inp["w0"] > 0)
        assert all(bits(r.pol[dead, i], inp["pol0"][dead]) for i in range(r.pol.shape[1])), "dead rays' pol"
        assert all(bits(r.pol[missed, i], inp["pol0"][missed]) for i in range(r.pol.shape[1])), "missed rays' pol"
        assert np.all(r.w[missed, 1:] == 0) and np.all(r.w[dead] == 0)


@pytest.mark.parametrize("variant", ["plain", "data_medium"])
@pytest.mark.parametrize("key", list(PLATES))
def test_weights_and_polarisation_against_exact_values(key, variant, capsys):
    r, inp = run(key, variant), inputs(key)
    sel, T, pol, a = exact(key)
    w0 = inp["w0"][sel]
    w_used = np.abs(r.w[sel, 1].astype(rc.LD) - w0.astype(rc.LD) * T) / rc.w_bar(w0, T, a)
    p_used = np.max(np.abs(r.pol[sel, 1].astype(rc.LD) - pol), axis=1) / rc.pol_bar(a)
    below = a < np.sqrt(pf.NEAR)
    with capsys.disabled():
        print(f"\n{key:5s} {variant:12s} n={w0.size}: w uses {float(w_used.max()):.3f} of its bar, pol {float(p_used.max()):.3f} "
              f"(below the threshold {float(p_used[below].max()):.3f}, within 16 x above {float(p_used[~below & (a < 2.0 ** -21)].max()):.3f})")
    assert np.all(np.isfinite(r.w[sel, 1])) and np.all(np.isfinite(r.pol[sel, 1]))
    assert float(w_used.max()) <= 1 and float(p_used.max()) <= 1
    gain = np.where(T <= 1, r.w[sel, 1] / w0, 0.0)
    assert np.max(gain) <= 1, "no ray gains power"


@pytest.mark.parametrize("key", list(PLATES))
def test_no_pol_weights_against_exact_half_half(key):
    r, inp = run(key, "no_pol"), inputs(key)
    sc = PLATES[key]
    sel, _, _, a = exact(key)
    w0 = inp["w0"][sel]
    T = rc.nopol_T(rc.unit_normal(sc.normal), inp["s0"][sel], sc.n1, sc.n2)
    assert float(np.max(np.abs(r.w[sel, 1].astype(rc.LD) - w0.astype(rc.LD) * T) / rc.w_bar(w0, T, a))) <= 1
    assert np.all(np.isnan(r.pol)) if r.pol is not None else True


@pytest.mark.parametrize("key", list(PLATES))
def test_tabulated_medium_kernel_has_the_same_bits(key):
    """SPEC 1 against SPEC 0 on the handed-in rays."""
    a, b = run(key, "plain"), run(key, "data_medium")
    assert bits(a.w, b.w) and bits(a.pol, b.pol) and bits(a.p, b.p)


@pytest.mark.parametrize("key", list(PLATES))
def test_discrete_spectrum_kernel_has_the_same_bits(key):
    """SPEC 2 generates its rays in the kernel (a monochromatic source is a discrete spectrum): the same rays from
    ot_rays_generate, handed to the SPEC 0 and SPEC 1 kernels, end with the same w and pol in every section."""
    lib, N, seed = _capi.load_library(), 4999, 31
    sc = PLATES[key]
    with ot.global_options.no_warnings():
        RT = rc.raytracer(ot, sc)
        RT.seed = seed
        RT.trace(N)
        st = RT.rays
        w2, pol2, p2 = st.w_list.copy(), st.pol_list.copy(), st.p_list.copy()
        tab, rng = st._source_table(seed), st._source_ranges()
        buf = {k: torch.empty(m * N, dtype=dt, device="cuda") for k, m, dt in
               (("p", 3, torch.float64), ("s", 3, torch.float64), ("w", 1, torch.float32), ("n", 1, torch.float64),
                ("wl", 1, torch.float32), ("pol", 3, torch.float32))}
        rays = _capi.Rays()
        rays.N, rays.nt = N, 1
        rays.p, rays.s, rays.w, rays.n, rays.wl = (buf[k].data_ptr() for k in ("p", "s", "w", "n", "wl"))
        rays.pol = buf["pol"].data_ptr()
        _capi.check(lib.ot_rays_generate(tab.handle, rng, len(rng), seed, 0, C.byref(rays), stream_ptr()))
        torch.cuda.synchronize()
        host = {k: v.cpu().numpy() for k, v in buf.items()}
        init = (host["p"].reshape(3, N).T.copy(), host["s"].reshape(3, N).T.copy(), host["pol"].reshape(3, N).T.copy(),
                host["w"], host["wl"])
        assert bits(init[0], p2[:, 0]) and bits(init[3], w2[:, 0]), "the generated rays are the traced ones"
        for variant in ("plain", "data_medium"):
            RT1 = rc.raytracer(ot, sc, variant)
            RT1.trace(N, _initial_rays=init, _N_list=np.array([N]))
            assert bits(RT1.rays.w_list, w2) and bits(RT1.rays.pol_list, pol2), variant
    assert np.count_nonzero(w2[:, 1] > 0) > 4000 and np.any(pol2[:, 1] != pol2[:, 0])


def test_double_gauss_against_the_oracle():
    from optrace_amd.scene import CompiledScene
    import oracle_bridge as ob
    N = 20_000
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=9)
        RT.trace(N)
        p0, wl, w0, pol0 = (RT.rays.p_list[:, 0].copy(), RT.rays.wl_list.copy(), RT.rays.w_list[:, 0].copy(),
                            RT.rays.pol_list[:, 0].copy())
        d = RT.rays.p_list[:, 1] - p0
        s0 = d / np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + d[:, 2] ** 2)[:, None]
        RT2 = scenes.double_gauss(ot)
        RT2.trace(N, _initial_rays=(p0, s0, pol0, w0, wl))
    csc = CompiledScene(RT2)
    rays = ob.HostRays(N, csc.nt, False)
    rays.set_initial(p0, s0, pol0, w0, wl)
    msgs, status = ob.trace(csc.desc, rays, None)
    assert status == 0 and np.array_equal(msgs, RT2._msgs), (msgs, RT2._msgs)
    assert np.array_equal(rays.w_list > 0, RT2.rays.w_list > 0)
    np.testing.assert_allclose(RT2.rays.p_list, rays.p_list, rtol=1e-12, atol=1e-12)
    live = rays.w_list > 0
    assert np.count_nonzero(live[:, -2]) > N // 2
    assert np.max(np.abs(RT2.rays.w_list[live].astype(np.float64) / rays.w_list[live] - 1)) <= 1e-6
    assert np.max(np.abs(RT2.rays.pol_list.astype(np.float64) - rays.pol_list)[live]) <= 1e-6
