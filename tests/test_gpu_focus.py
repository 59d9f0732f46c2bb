"""GPU parity of Raytracer.focus_search against the reference's fixtures
(tests/golden/focus.npz: cost curves, optimiser results, mean positions)."""
import numpy as np
import pytest
import torch

import optrace_amd as ot
import scenes
from helpers import load, assert_close
from test_gpu_parity import gpu_trace

pytestmark = pytest.mark.gpu

CASES = {  # mirrors FOCUS_CASES of tests/golden/generate_golden.py
    "c1_single_lens": ("c1_single_lens", None),
    "double_gauss_src0": ("double_gauss", 0),
    "double_gauss_all": ("double_gauss", None),
    "asphere": ("asphere", None),
    "mixed_first_gap": ("mixed_geometry", 1),
}


PLATEAU = {"mixed_first_gap"}


@pytest.mark.parametrize("cname", list(CASES))
def test_focus_search_matches_reference(cname):
    tname, si = CASES[cname]
    g, RT = gpu_trace(tname)
    f = load("focus.npz")
    z_start = float(f[f"{cname}/z_start"])
    with ot.global_options.no_warnings():
        for mi, method in enumerate(RT.focus_search_methods):
            k = f"{cname}/{mi}"
            res, d = RT.focus_search(method, z_start, source_index=si, return_cost=True, _z_samples=f[f"{k}/z"])
            assert d["N"] == int(f[f"{k}/N"]), "number of rays used must be exact"
            assert_close(d["bounds"], f[f"{k}/bounds"], rtol=1e-14, what="bounds")
            ref_cost = f[f"{k}/cost"]
            err = np.abs(d["cost"] - ref_cost) / np.maximum(np.abs(ref_cost), 1e-300)
            if mi == 0:
                assert err.max() < 1e-9, (method, err.max())
            else:
                # a hit within rounding of a pixel edge may fall into the neighbour pixel at single samples.  The looseness
                # comes from the two tracers' lines differing (1e-11), not from the kernels: on the device's own lines every
                # one of these samples agrees with a longdouble host evaluation within the summation bound, with no sample
                # ambiguous (test_gpu_focus_kernels.py::test_scene_curves_on_the_device_lines).
                assert np.quantile(err, 0.97) < 1e-8 and err.max() < 0.05, (method, np.sort(err)[-5:])
            span = d["bounds"][1] - d["bounds"][0]
            xr, fr = float(f[f"{k}/x"]), float(f[f"{k}/fun"])
            if mi == 0:
                assert abs(res.x - xr) <= 1e-9 * span
                assert abs(res.fun - fr) <= 1e-7 * abs(fr)  # spot of 20 um from positions that agree to 1e-11 rel.
            else:
                # the cost function itself: evaluated at the reference's optimum it gives the reference's value
                _, dr = RT.focus_search(method, z_start, source_index=si, return_cost=True, _z_samples=np.array([xr]))
                assert abs(dr["cost"][0] - fr) <= 1e-8 * abs(fr), (method, dr["cost"][0], fr)
                # same SciPy optimiser on a piecewise-constant, noisy cost function: pixel sums are accumulated
                # in a different order than np.add.at does, so exact ties of the reference can break here and
                # the optimiser may settle a few steps away -- within one sample spacing, same cost to 2 %.
                # (PLATEAU: parallel bundle, the cost does not depend on z at all; only the value is comparable.)
                assert abs(res.fun - fr) <= 0.02 * abs(fr), (method, res.fun, fr)
                if cname not in PLATEAU:
                    assert abs(res.x - xr) <= span / 320, (method, res.x, xr)
            if abs(res.x - xr) <= 1e-9 * span:
                assert_close(d["pos"], f[f"{k}/pos"], rtol=1e-6, atol=1e-9 * span, what="pos")
            assert d["pos"][2] == res.x
            res2, d2 = RT.focus_search(method, z_start, source_index=si)
            assert d2["z"] is None and d2["cost"] is None
            if mi == 0:  # closed form, no sampling or simplex involved
                assert abs(res2.x - res.x) <= 1e-12 * span


def test_focus_finds_the_paraxial_focus():
    """Ideal lens, parallel bundle: every method has to end near z = lens + f."""
    with ot.global_options.no_warnings():
        RT = ot.Raytracer(outline=[-5, 5, -5, 5, -5, 60], seed=3)
        RT.add(ot.RaySource(ot.CircularSurface(r=1.5), divergence="None", s=[0, 0, 1], pos=[0, 0, -2],
                            spectrum=ot.LightSpectrum("Monochromatic", wl=550.)))
        RT.add(ot.IdealLens(r=3, D=1000 / 30, pos=[0, 0, 0]))
        RT.trace(200_000)
        np.random.seed(4)
        for method in RT.focus_search_methods:
            res, d = RT.focus_search(method, 20., return_cost=method != "RMS Spot Size")
            assert d["N"] == 200_000
            # (an aberration-free image on its own auto-extent looks the same at every z: the two sharpness
            # methods have no minimum to find here; they are only required to stay finite and inside the bounds)
            if method == "RMS Spot Size":
                assert abs(res.x - 30.) < 1e-6, (method, res.x)
            elif method == "Irradiance Variance":
                assert abs(res.x - 30.) < 0.5, (method, res.x)
            assert d["bounds"][0] <= res.x <= d["bounds"][1] and np.isfinite(res.fun)
            assert abs(d["pos"][0]) < 1e-3 and abs(d["pos"][1]) < 1e-3 and d["pos"][2] == res.x
            if d["cost"] is not None:
                assert d["cost"].shape == (320,) and np.all(np.isfinite(d["cost"]))
                assert np.all(np.diff(d["z"]) > 0) and d["bounds"][0] <= d["z"][0] and d["z"][-1] <= d["bounds"][1]


def test_focus_large_bundle_pixel_count_and_linearity():
    """3 M rays: N_px follows sqrt(N); the RMS cost is the same whether rays come in one bundle or two sources."""
    with ot.global_options.no_warnings():
        RT = scenes.c1_single_lens(ot, seed=9)
        RT.trace(3_000_000)
        res, d = RT.focus_search("RMS Spot Size", 14., return_cost=True, _z_samples=np.linspace(11, 19, 320))
        assert d["N"] == 3_000_000 and np.all(np.isfinite(d["cost"]))
        j = int(np.argmin(d["cost"]))
        assert abs(d["z"][j] - res.x) < 0.1 and res.fun <= d["cost"].min() * (1 + 1e-9)
        res2, d2 = RT.focus_search("Irradiance Variance", 14.)
        assert abs(res2.x - res.x) < 2.0


def test_focus_errors():
    with ot.global_options.no_warnings():
        RT = scenes.c1_single_lens(ot, seed=1)
        with pytest.raises(RuntimeError):
            RT.focus_search("RMS Spot Size", 12.)
        RT.trace(5000)
        with pytest.raises(ValueError):
            RT.focus_search("Best Guess", 12.)
        with pytest.raises(ValueError):
            RT.focus_search("RMS Spot Size", 1e4)
        with pytest.raises(IndexError):
            RT.focus_search("RMS Spot Size", 12., source_index=-1)
        with pytest.raises(IndexError):
            RT.focus_search("RMS Spot Size", 12., source_index=7)
        # search region in front of the only source start: no rays -> placeholder result
        RT2 = ot.Raytracer(outline=[-5, 5, -5, 5, -5, 60], seed=3)
        RT2.add(ot.RaySource(ot.CircularSurface(r=1.5), divergence="None", s=[0, 0, 1], pos=[0, 0, -2]))
        RT2.add(ot.Aperture(ot.CircularSurface(r=3), pos=[0, 0, 5]))  # absorbs everything
        RT2.add(ot.IdealLens(r=3, D=10, pos=[0, 0, 10]))
        RT2.trace(3000)
        res, d = RT2.focus_search("RMS Spot Size", 20.)
        assert d["N"] == 0 and np.all(np.isnan(d["pos"]))


def test_rms_closed_form_equals_per_sample_kernel():
    """The RMS cost curve from the quadratic moment form against the two-pass kernel evaluation (ot_focus_cost)."""
    import ctypes as C
    from optrace_amd import _capi
    from optrace_amd._device import ptr, stream_ptr
    lib = _capi.load_library()
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=5)
        RT.trace(300_000)
        zs = np.linspace(146., 165., 97)
        res, d = RT.focus_search("RMS Spot Size", 150., return_cost=True, _z_samples=zs)
        # the same lines through the per-sample kernels
        b = d["bounds"]
        n = RT.rays.N
        pasb = torch.empty(4 * n, dtype=torch.float64, device="cuda")
        w = torch.empty(n, dtype=torch.float32, device="cuda")
        nu = torch.empty(1, dtype=torch.int64, device="cuda")
        rays = RT.rays._rays_struct()
        _capi.check(lib.ot_focus_prepare(C.byref(rays), 0, n, b[0] + RT.N_EPS, ptr(pasb), ptr(w), ptr(nu), stream_ptr()))
        ws = torch.empty(_capi.FOCUS_WS + 4, dtype=torch.float64, device="cuda")
        out = torch.empty(zs.shape[0], dtype=torch.float64, device="cuda")
        _capi.check(lib.ot_focus_cost(n, ptr(pasb), ptr(w), 0, zs.ctypes.data_as(C.POINTER(C.c_double)), zs.shape[0], 2,
                                      ptr(ws), ptr(out), stream_ptr()))
    ref = out.cpu().numpy()
    assert np.all(np.abs(d["cost"] - ref) <= 1e-9 * ref), np.abs(d["cost"] / ref - 1).max()
    assert d["cost"].min() >= res.fun * (1 - 1e-9)


def test_all_methods_find_the_focus_of_a_lens():
    """After the reference's test_focus (tests/test_tracer.py:295-366): every method finds the focal point of a biconvex
    lens in n0 = 1.1 (33.084 mm behind it) within 0.15 mm, per source as well; a second source at g = 60 mm is imaged
    at b = 73.73 mm; wrong arguments raise like the reference."""
    fs = 33.08433714
    with ot.global_options.no_warnings():
        RT = ot.Raytracer(outline=[-3, 3, -3, 3, -10, 40], n0=ot.RefractionIndex("Constant", n=1.1), seed=3)
        RT.add(ot.RaySource(ot.CircularSurface(r=0.5), pos=[0, 0, -3]))
        RT.add(ot.Lens(ot.SphericalSurface(r=3, R=30), ot.ConicSurface(r=3, R=-20, k=1), ot.RefractionIndex("Constant", n=1.5),
                       de=0.1, pos=[0, 0, 0]))
        with pytest.raises(RuntimeError):
            RT.focus_search(RT.focus_search_methods[0], z_start=5)  # nothing traced yet
        RT.trace(200_000)
        for method in RT.focus_search_methods:
            res, _ = RT.focus_search(method, z_start=5.0)
            assert abs(res.x - fs) < 0.15, method
        res, _ = RT.focus_search(RT.focus_search_methods[0], z_start=5.0, source_index=0)
        assert abs(res.x - fs) < 0.15

        RT.add(ot.RaySource(ot.Point(), divergence="Isotropic", div_angle=0.5, pos=[0, 0, -60]))
        RT.outline = [-3, 3, -3, 3, -70, 80]
        RT.trace(100_000)
        res, _ = RT.focus_search(RT.focus_search_methods[0], z_start=5.0, source_index=0)
        assert abs(res.x - fs) < 0.15
        res, _ = RT.focus_search(RT.focus_search_methods[0], z_start=5.0, source_index=1)
        assert abs(res.x - 73.73) < 0.1

        with pytest.raises(ValueError):
            RT.focus_search(RT.focus_search_methods[0], z_start=-100)
        with pytest.raises(ValueError):
            RT.focus_search("AA", z_start=10)
        for bad in (-1, 10):
            with pytest.raises(IndexError):
                RT.focus_search(RT.focus_search_methods[0], z_start=10, source_index=bad)
        # search regions before, between and behind the elements
        RT.focus_search(RT.focus_search_methods[0], z_start=RT.outline[4])
        RT.focus_search(RT.focus_search_methods[0], z_start=RT.outline[4], source_index=0)
        RT.focus_search(RT.focus_search_methods[0], z_start=RT.outline[5])
        RT.focus_search(RT.focus_search_methods[0], z_start=RT.lenses[0].extent[5] + 0.01)
        RT.focus_search("Irradiance Variance", z_start=RT.outline[5])
