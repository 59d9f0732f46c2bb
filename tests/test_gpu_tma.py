"""The paraxial analysis meets the device tracer: the planes ot.TMA predicts are where the HIP kernels put the light
(fixtures: tests/golden/tma.npz, "ideal/..." and "focus/...", written by tests/golden/generate_golden_tma.py)."""
import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd.tma import index_at

import scenes
import scenes_tma as st
from helpers import load

pytestmark = pytest.mark.gpu

POSITION_FLOOR = 1e-11  # mm, the project's position tolerance


@pytest.fixture(scope="module")
def golden():
    return load("tma.npz")


@pytest.mark.parametrize("which", ["one", "two"])
def test_ideal_lenses_image_a_point_where_the_analysis_says(golden, which):
    """Ideal lenses map tangents: an off-axis point is imaged to a point at any ray height.  1e6 device rays land within
    10 x the spread of the reference's own rays (other random rays, hence the factor; at least 1e-11 mm) of
    image_magnification * (x0, y0) in the plane image_position; no ray is left out."""
    N = 1_000_000
    with ot.global_options.no_warnings():
        RT, zb, point = st.ideal_imaging_scene(ot, which, seed=5)
        assert abs(zb - float(golden[f"ideal/{which}/zb"])) <= 1e-12 * abs(zb)
        assert np.allclose(point, golden[f"ideal/{which}/point"], rtol=1e-12, atol=0)
        RT.trace(N)
        assert not RT.geometry_error
        hits, alive = st.plane_hits(RT.rays, zb)
        assert alive.all() and hits.shape[0] == N, "no ray is absorbed in front of the image plane"
        dist = np.hypot(hits[:, 0] - point[0], hits[:, 1] - point[1])
        bound = max(10 * float(golden[f"ideal/{which}/spread"]), POSITION_FLOOR)
        print(f"ideal lenses ({which}): largest distance {dist.max():.3g} mm, bound {bound:.3g} mm")
        assert dist.max() <= bound, (dist.max(), bound)

        # the same through the detector stage: all power in the pixel that holds the predicted point
        # (945 pixels per side: 0.3 and 0.7 of the side put the point at 283.5 and 661.5, the middle of a pixel)
        h = 1e-3
        extent = [point[0] - 0.3 * h, point[0] + 0.7 * h, point[1] - 0.7 * h, point[1] + 0.3 * h]
        img = RT.detector_image(extent=extent)
        W = img._data[:, :, 3]
        e = img.extent
        ny, nx = W.shape
        fx, fy = (point[0] - e[0]) / (e[1] - e[0]) * nx, (point[1] - e[2]) / (e[3] - e[2]) * ny
        assert min(fx % 1, fy % 1) > 0.4 and max(fx % 1, fy % 1) < 0.6, "the point is not on a pixel edge"
        ix, iy = int(fx), int(fy)
        total = float(np.sum(RT.rays.w_list[:, -2], dtype=np.float64))
        assert W[iy, ix] > 0 and np.count_nonzero(W) == 1
        assert abs(W[iy, ix] - total) <= 1e-6 * total, (W[iy, ix], total)


@pytest.mark.parametrize("name", st.FOCUS_SCENES)
def test_real_lenses_focus_where_the_reference_finds_it(golden, name):
    """A thin collimated beam, the reference's rays injected: focus_search started at the focal point of the analysis
    ends where the reference's ends, at the tolerance of tests/test_gpu_focus.py for this method (1e-9 of the search
    span).  How far that is from focal_points[1] is recorded, not bounded."""
    k = f"focus/{name}"
    with ot.global_options.no_warnings():
        RT = st.focus_scene(ot, name, no_pol=True)
        init = (golden[f"{k}/p0"], golden[f"{k}/s0"], None, golden[f"{k}/w0"], golden[f"{k}/wl"])
        RT.trace(int(golden[f"{k}/N_list"].sum()), _initial_rays=init, _N_list=golden[f"{k}/N_list"])
        assert not RT.geometry_error
        F2 = RT.tma().focal_points[1]
        assert abs(F2 - float(golden[f"{k}/F2"])) <= 1e-12 * abs(F2)
        res, d = RT.focus_search("RMS Spot Size", z_start=F2)
    assert d["N"] == int(golden[f"{k}/N"])
    assert np.allclose(d["bounds"], golden[f"{k}/bounds"], rtol=1e-14, atol=0)
    span = d["bounds"][1] - d["bounds"][0]
    xr = float(golden[f"{k}/x"])
    print(f"focus {name}: device {res.x:.12g}, reference {xr:.12g}, focal_points[1] {F2:.12g}")
    assert abs(res.x - xr) <= 1e-9 * span, (res.x, xr, span)


def test_typical_script_with_an_analysis_between_two_traces():
    """Put the detector at the focal point the analysis gives, trace, render; RT.tma() between two traces leaves the
    unchanged-scene shortcut of `trace` in place (its record of the last full trace survives and is used)."""
    with ot.global_options.no_warnings():
        RT = ot.Raytracer(outline=[-5, 5, -5, 5, -10, 60], n0=ot.RefractionIndex("Constant", n=1.1), seed=11)
        RT.add(ot.RaySource(ot.CircularSurface(r=0.3), divergence="None", s=[0, 0, 1], pos=[0, 0, -5],
                            spectrum=ot.LightSpectrum("Monochromatic", wl=555.)))
        RT.add(ot.Lens(ot.SphericalSurface(r=3, R=30), ot.SphericalSurface(r=3, R=-20), de=0.1, pos=[0, 0, 0],
                       n=ot.RefractionIndex("Abbe", n=1.6, V=40.)))
        tma = RT.tma()
        assert tma.n1 == 1.1 and 0 < tma.focal_points[1] < 60
        RT.add(ot.Detector(ot.RectangularSurface(dim=[1, 1]), pos=[0, 0, tma.focal_points[1]]))
        RT.trace(100_000)
        rec = RT._record
        assert rec is not None and RT._scene_unchanged()
        img = RT.detector_image()
        assert max(img.s) < 0.02 and img.power() > 0.8  # a spot of a few um where a 0.6 mm beam went in (Fresnel losses: 7 %)
        assert RT._scene_unchanged()
        again = RT.tma()
        again.image_position(-100.), RT.lenses[0].tma(n0=RT.n0).pupil_position(1.)
        assert RT._scene_unchanged(), "an analysis is no scene change"
        RT.trace(100_000)
        assert RT._record is rec, "the second trace took the shortcut"
        assert again.focal_points == tma.focal_points
        RT.lenses[0].move_to([0, 0, 1])   # a real change still ends it
        assert not RT._scene_unchanged()


@pytest.mark.parametrize("name", ["Abbe", "Sellmeier1", "Conrady", "Extended3", "Data"])
def test_host_index_is_the_device_index(name):
    """The analysis evaluates n on the host; at wavelengths that are float32 numbers it is the n the kernels use
    (device: repeated multiplication for whole-number powers, within 3 ulp of pow per term)."""
    ri = ot.RefractionIndex(name, **scenes.MEDIA[name])
    wl = np.array([400., 486.125, 555., 656.25, 780.])
    dev = ri(wl)
    host = np.array([index_at(ri, float(w)) for w in wl])
    assert np.all(np.abs(dev - host) <= 1e-14 * host), (dev, host)
