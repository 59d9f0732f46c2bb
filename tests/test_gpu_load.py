"""Loaded lens prescriptions on the device: `ot.load_zmx(file, ot.load_agf(subset))` is put into a Raytracer (no geometry
comes from a fixture: the loader builds the scene, the fixture supplies rays and expectations), traced with the reference's
injected rays (tests/golden/trace_zmx_*.npz) and compared by the rules of tests/test_gpu_parity.py: hit masks and the five
counters per section bit-exact, weights, wavelengths, indices, polarisation as there.

Positions.  1e-11 mm is the project's figure for up to 17 sections.  The tolerance of a fixture is 1e-11 mm where the
largest position deviation of the C oracle from the reference (printed by tests/golden/generate_golden_load.py and by
tests/test_oracle_load.py) is below 2.5e-12 mm, else four times that deviation: oracle and kernel are two float64
evaluations of the same formulas that differ in contraction and in the kernel's own reciprocal and square-root cores, so
their rounding should grow with depth alike, within a small factor.  The factor 4 is a chosen margin, not a measurement.
On trace_double_gauss (17 sections) the oracle's deviation is exactly 0, so the existing 1e-11 has no finite margin over
this yardstick to use instead; the rule stands as stated.

    fixture           sections   oracle - reference [mm]   tolerance [mm]
    achromat              6      0                          1e-11
    tessar               11      0                          1e-11
    tessar_nopol         11      0                          1e-11
    liang                12      2.66e-15                   1e-11
    blank_aspheres       12      3.44e-15                   1e-11
    nikon60x             78      1.25e-12                   1e-11
"""
import numpy as np
import pytest

import optrace_amd as ot

import load_cases as lc
from helpers import load, assert_close

pytestmark = pytest.mark.gpu

ORACLE_DEVIATION = {"achromat": 0., "tessar": 0., "tessar_nopol": 0., "liang": 2.66e-15, "blank_aspheres": 3.44e-15,
                    "nikon60x": 1.25e-12}


def position_tolerance(fixture: str) -> float:
    dev = ORACLE_DEVIATION[fixture]
    return 1e-11 if dev < 2.5e-12 else 4 * dev


def test_tolerance_table_is_the_generators():
    g = load("load.npz")
    for fixture, dev in ORACLE_DEVIATION.items():
        assert abs(float(g[f"oracle/{fixture}"]) - dev) <= 0.005 * dev, fixture


@pytest.mark.parametrize("fixture", list(lc.TRACE_FIXTURES))
def test_loaded_system_traces_like_the_reference(fixture):
    system, no_pol = lc.TRACE_FIXTURES[fixture]
    g = load(f"trace_zmx_{fixture}.npz")
    with ot.global_options.no_warnings():
        RT = lc.traced_scene(ot, system, no_pol=no_pol)
        init = (g["p0"], g["s0"], None if no_pol else g["pol0"], g["w0"], g["wl"])
        RT.trace(int(g["N"]), _initial_rays=init, _N_list=g["N_list"])
    assert not RT.geometry_error
    r = RT.rays
    assert r.p_list.shape == g["p_list"].shape
    assert np.array_equal(RT._msgs, g["msgs"]), f"counters differ:\n{RT._msgs}\n{g['msgs']}"
    assert np.array_equal(r.w_list > 0, g["w_list"] > 0), "alive masks per section must be bit-exact"
    tol = position_tolerance(fixture)
    print(f"{fixture}: {r.p_list.shape[1]} sections, device - reference: {np.abs(r.p_list - g['p_list']).max():.3g} mm "
          f"(tolerance {tol:.3g})")
    assert_close(r.p_list, g["p_list"], rtol=0, atol=tol, what="p_list")
    assert np.array_equal(r.wl_list, g["wl"])
    assert_close(r.n_list, g["n_list"], rtol=1e-13, what="n_list")
    assert_close(r.w_list, g["w_list"], rtol=2e-7, atol=1e-30, what="w_list")
    assert_close(r.s0_list, g["s_final"], rtol=1e-10, atol=1e-12, what="s_final")
    if not no_pol:
        assert r.pol_list.dtype == np.float32
        assert_close(r.pol_list, g["pol_list"], rtol=1e-5, atol=2e-7, what="pol_list")


def test_achromat_focuses_where_the_reference_finds_it():
    """Collimated beam through the loaded achromat, the reference's rays: focus_search("RMS Spot Size") started at the
    focal point of the analysis ends at focal_points[1] minus the spherical-aberration residual the reference shows for the
    same beam, within the search's own resolution (1e-9 of the search span, as tests/test_gpu_tma.py holds this method)."""
    g, ref = load("trace_zmx_achromat.npz"), load("load.npz")
    with ot.global_options.no_warnings():
        RT = lc.traced_scene(ot, "achromat")
        RT.trace(int(g["N"]), _initial_rays=(g["p0"], g["s0"], g["pol0"], g["w0"], g["wl"]), _N_list=g["N_list"])
        F2 = RT.tma().focal_points[1]
        assert abs(F2 - float(ref["focus/achromat/F2"])) <= 1e-12 * abs(F2)
        res, d = RT.focus_search("RMS Spot Size", z_start=F2)
    assert d["N"] == int(ref["focus/achromat/N"])
    assert np.allclose(d["bounds"], ref["focus/achromat/bounds"], rtol=1e-14, atol=0)
    residual = float(ref["focus/achromat/x"]) - float(ref["focus/achromat/F2"])
    span = d["bounds"][1] - d["bounds"][0]
    print(f"focus achromat: device {res.x:.12g}, focal_points[1] {F2:.12g}, reference's residual {residual:+.3g} mm")
    assert abs(res.x - (F2 + residual)) <= 1e-9 * span, (res.x, F2, residual, span)


def test_tessar_image_has_the_power_of_its_hits():
    N = 1_000_000
    with ot.global_options.no_warnings():
        RT = lc.traced_scene(ot, "tessar", seed=3)
        RT.trace(N)
        assert not RT.geometry_error
        img = RT.detector_image()
        ph, hw, wl, ext, projection, ill = RT._hit_detector("x", 0, None, None, None)
    power = float(hw.double().sum().item())
    assert 0.2 < power < 1.0, "a good part of the beam passes the stop, Fresnel losses at eight surfaces"
    assert abs(img.power() - power) <= 1e-6 * power


def test_adding_a_marker_between_two_traces_keeps_the_shortcut():
    with ot.global_options.no_warnings():
        RT = lc.traced_scene(ot, "achromat", seed=5)
        RT.trace(100_000)
        rec = RT._record
        assert rec is not None and RT._scene_unchanged() and len(RT.markers) == 1
        first = RT.rays.p_list.copy()
        F2 = RT.tma().focal_points[1]
        RT.add(ot.PointMarker("F2", [0, 0, F2]))
        RT.add(ot.LineMarker(r=5, pos=[0, 0, F2], desc="focal plane"))
        RT.markers[0].move_to([0, 20, 0])
        assert RT._scene_unchanged(), "markers are no scene change"
        RT.trace(100_000)
        assert RT._record is rec, "the second trace took the shortcut"
        assert np.array_equal(RT.rays.p_list, first), "same seed, same scene: same rays"
        RT.lenses[0].move_to([0, 0, 1])
        assert not RT._scene_unchanged()
