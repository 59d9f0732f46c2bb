"""Refractive indices and filter transmissions on the device, value by value and route by route (medium_n, filter_T of
csrc/ot_device.hpp; tests/wavelength_cases.py, tests/golden/wavelength_step.npz).

Each value of a case is read back from
  leaf      the leaf kernel ot_refraction_index (media)
  formula   the formula kernel (injected rays through one plate of the medium, or one filter disc): the index plane the
            kernel stores itself (index store on; sections 1 and 2) and the weight behind the filter against the weight in
            front of it; also with a numeric-hit asphere lens or a spline-surface lens behind, and without polarisation
  table     the table kernel: the same scene with a tabulated filter behind -- the bits of `formula`
  fill      ot_rays_fill_index with the index store off -- the bits of `formula`
  lines     the line tables the host builds for discrete sources: the same element under a Lines source of eight of the
            case's wavelengths, traced fused, launch after launch until every wavelength was a line once; the expectation
            of a ray comes from its wavelength in wl_list; again with the asphere lens or the spline lens behind and
            without polarisation (the bits of the plain launches)
  tail      one render-only launch per filter type: the weights of the living rays are the stored form's
and held to the bar of its model (wavelength_cases: bitwise to the reference's recorded value, a forward error bound for
the models with powers, float32 units for the Gaussian).  The log lists the largest error over bar per case and route and
the number of samples on which `formula` and `lines` differ.
"""
import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd.ray_storage import TailStorage

import wavelength_cases as wc
from helpers import load

pytestmark = pytest.mark.gpu

bits = wc.bits
N = wc.N_WL
BEHIND = ("plain", "asphere_behind", "spline_behind", "no_pol")
OUTLINE = [-5, 5, -5, 5, -10, 40]
N_LINES = 256   # rays of a launch under a Lines source


@pytest.fixture(scope="module")
def g():
    return load("wavelength_step.npz")


def raytracer(element, variant="plain", source=None, seed=None):
    const = lambda n: ot.RefractionIndex("Constant", n=n)
    RT = ot.Raytracer(outline=OUTLINE, n0=const(1.0), no_pol=(variant == "no_pol"), **({} if seed is None else dict(seed=seed)))
    RT.add(source or ot.RaySource(ot.Point(), divergence="None", s=[0, 0, 1], pos=[0, 0, -5], spectrum=ot.LightSpectrum("Monochromatic", wl=550.)))
    if isinstance(element, ot.RefractionIndex):
        RT.add(ot.Lens(ot.CircularSurface(r=3), ot.CircularSurface(r=3), n=element, n2=element, pos=[0, 0, 0], d1=0.5, d2=0.5))
    else:
        RT.add(ot.Filter(ot.CircularSurface(r=3), pos=[0, 0, 0], spectrum=element))
    if variant == "asphere_behind":
        RT.add(ot.Lens(ot.AsphericSurface(r=4, R=12, k=-0.8, coeff=[2e-3, -4e-5, 3e-7]), ot.CircularSurface(r=4), de=0.5,
                       n=const(1.6), pos=[0, 0, 8]))
    if variant == "spline_behind":
        Y, X = np.mgrid[-4:4:80j, -4:4:80j]
        RT.add(ot.Lens(ot.DataSurface2D(r=4.0, data=X ** 2 / 20 + Y ** 2 / 14), ot.CircularSurface(r=4.0), de=0.5, n=const(1.6), pos=[0, 0, 8]))
    if variant == "data_behind":
        RT.add(ot.Filter(ot.CircularSurface(r=3), pos=[0, 0, 8],
                         spectrum=ot.TransmissionSpectrum("Data", wls=np.linspace(380.0, 780.0, 41), vals=np.full(41, 0.5))))
    return RT


def injected(wl, w0):
    n = wl.shape[0]
    p0 = np.tile([0.0, 0.0, -5.0], (n, 1))
    p0[:, 0] = 0.25 * (np.arange(n) % 5)     # (a few start points: nothing here depends on them)
    s0 = np.tile([0.0, 0.0, 1.0], (n, 1))
    pol0 = np.tile(np.array([1.0, 0.0, 0.0], dtype=np.float32), (n, 1))
    return p0, s0, pol0, w0, wl


def raw_n(RT, count):
    t = dict.__getitem__(RT.rays._dev, "n")
    return t.view(RT.rays._nt, RT.rays._Np)[:, :count].cpu().numpy().T.copy()


def trace_both(RT, count, **kw):
    """-> (n plane filled on demand, n plane stored by the trace kernel, w_list, wl_list) of the same call."""
    lib = _capi.load_library()
    RT.trace(count, **kw)
    assert not RT.geometry_error and RT.rays._n_stale
    w, wl = RT.rays.w_list.copy(), RT.rays.wl_list.copy()
    filled = RT.rays.n_list.copy()
    _capi.check(lib.ot_scene_set_index_store(RT._scene_handle, 1))
    dict.__getitem__(RT.rays._dev, "n").fill_(float("nan"))
    RT.trace(count, **kw)
    assert RT.rays._n_stale, "nothing here may have read the plane through the hook"
    stored = raw_n(RT, count)
    assert bits(RT.rays.w_list, w) and bits(RT.rays.wl_list, wl)
    return filled, stored, w, wl


def line_chunks(wl):
    u = np.unique(wl)
    return [u[i:i + 8] for i in range(0, u.shape[0], 8)]


def lines_source(chunk):
    # (power = ray count: every ray starts with weight 1, so the weight behind a filter shows fl32(T) as it is)
    return ot.RaySource(ot.Point(), divergence="None", s=[0, 0, 1], pos=[0, 0, -5], power=float(N_LINES),
                        spectrum=ot.LightSpectrum("Lines", lines=[float(v) for v in chunk], line_vals=[1.0] * len(chunk)))


def lines_route(element, wl, variant="plain", chunks=None):
    """Every wavelength as a line once -> (wavelengths seen, n of sections 1 and 2 as the kernel stored them, w1 / w0 pairs)."""
    WL, NS, W = [], [], []
    for k, chunk in enumerate(line_chunks(wl)[:chunks]):
        RT = raytracer(element, variant, source=lines_source(chunk), seed=100 + k)
        filled, stored, w, seen = trace_both(RT, N_LINES)
        assert RT._scene.desc.n_lines == len(chunk), "the line tables are in use"
        assert bits(filled, stored), "the fill and the kernel's own store under a discrete source"
        assert set(np.unique(seen)) == set(chunk), "every line was drawn"
        WL.append(seen)
        NS.append(stored[:, 1:3])
        W.append(w[:, :2])
    return np.concatenate(WL), np.concatenate(NS), np.concatenate(W)


def per_wavelength(wl, seen, values):
    """The value each wavelength of `wl` got among the rays `seen` (all rays of one wavelength agree bitwise)."""
    out = np.empty(wl.shape[0], dtype=values.dtype)
    for i, v in enumerate(wl):
        sel = values[seen == v]
        assert sel.shape[0] and (np.all(sel == sel[0]) or np.all(np.isnan(sel))), float(v)
        out[i] = sel[0]
    return out


@pytest.mark.parametrize("case", wc.media_names())
def test_refractive_index_route_by_route(g, case, capsys):
    ri = wc.medium(ot, case)
    wl = wc.medium_wavelengths(case, ri)
    assert bits(wl, g[f"n/{case}/wl"]), "the archive belongs to other wavelengths"
    w0 = np.full(N, 1.0, dtype=np.float32)
    routes, lines = {}, []
    with ot.global_options.no_warnings():
        routes["leaf"] = np.asarray(ri(wl.astype(np.float64)), dtype=np.float64)
        base = None
        for variant in BEHIND + ("data_behind",):
            RT = raytracer(ri, variant)
            pol = None if RT.no_pol else injected(wl, w0)[2]
            p0, s0, _, _, _ = injected(wl, w0)
            filled, stored, w, _ = trace_both(RT, N, _initial_rays=(p0, s0, pol, w0, wl), _N_list=np.array([N]))
            assert bits(filled[:, :3], stored[:, :3]), f"{variant}: ot_rays_fill_index against the kernel's own store"
            assert bits(stored[:, 1], stored[:, 2]), "lens and the medium behind it are the same medium"
            assert np.all(stored[:, 0] == 1.0)
            if base is None:
                base = stored[:, 1].copy()
                routes["formula"] = base
            assert bits(stored[:, 1], base), f"{variant}: what stands behind changes the tested sections"
        seen, ns, _ = lines_route(ri, wl)
        assert bits(ns[:, 0], ns[:, 1])
        routes["lines"] = per_wavelength(wl, seen, ns[:, 0].copy())
        for variant in BEHIND[1:]:
            seen_v, ns_v, _ = lines_route(ri, wl, variant)
            assert bits(per_wavelength(np.unique(seen_v), seen_v, ns_v[:, 0].copy()), per_wavelength(np.unique(seen_v), seen, ns[:, 0].copy())), variant
    ok = True
    for route, got in routes.items():
        line, passes = wc.index_report(case, ri, wl, g, got, route)
        lines.append(line + ("" if passes else "   <-- FAILS"))
        ok &= passes
    lines.append(f"           n {case:24s} formula and lines routes differ on {int(np.count_nonzero(routes['formula'] != routes['lines']))} of {N} samples")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert ok, "\n".join(lines)
    if wc.model_of(ri) in wc.BITWISE_MEDIA:
        assert bits(routes["formula"], routes["lines"]) and bits(routes["formula"], routes["leaf"])


@pytest.mark.parametrize("case", list(wc.FILTER_CASES))
def test_filter_transmission_route_by_route(g, case, capsys):
    kw = wc.FILTER_CASES[case][0]
    spec = wc.filter_spectrum(ot, case)
    wl = wc.filter_wavelengths(case)
    assert bits(wl, g[f"T/{case}/wl"]), "the archive belongs to other wavelengths"
    ones = np.full(N, 1.0, dtype=np.float32)
    w0 = wc.weights(list(wc.FILTER_CASES).index(case))
    lines, ok, routes = [], True, {}
    with ot.global_options.no_warnings():
        base = None
        for variant in BEHIND + ("data_behind",):
            RT = raytracer(spec, variant)
            for weights in (ones, w0):
                p0, s0, pol, _, _ = injected(wl, weights)
                RT.trace(N, _initial_rays=(p0, s0, None if RT.no_pol else pol, weights, wl), _N_list=np.array([N]))
                w = RT.rays.w_list.copy()
                if weights is ones:
                    T = w[:, 1].astype(np.float64)
                    if base is None:
                        base = routes["formula"] = T
                    assert bits(T, base), f"{variant}: what stands behind changes the tested section"
                else:   # the weight is (float)((double)w0 * T), T the double the kernel had: fl32 of it is what w0 = 1 shows
                    if kw["spectrum_type"] != "Gaussian" or not kw.get("inverse"):
                        Td = g[f"T/{case}/ref"] if kw["spectrum_type"] != "Gaussian" else base
                        assert bits(w[:, 1], (weights.astype(np.float64) * Td).astype(np.float32)), f"{variant}: the product's two roundings"
                    half = weights == 0.5   # (halving is exact or, for a subnormal, the one rounding of the product)
                    assert bits(w[half, 1], (base[half] * 0.5).astype(np.float32)), f"{variant}: half of fl32(T)"
                dead = base == 0
                assert np.all(w[dead, 1:] == 0), "T = 0: the ray dies with weight exactly 0"
        seen, _, wpair = lines_route(spec, wl)
        assert np.all(wpair[:, 0] == 1.0)
        routes["lines"] = per_wavelength(wl, seen, wpair[:, 1].astype(np.float64))
        for variant in BEHIND[1:]:
            seen_v, _, wp_v = lines_route(spec, wl, variant)
            u = np.unique(seen_v)
            assert bits(per_wavelength(u, seen_v, wp_v[:, 1].copy()), per_wavelength(u, seen, wpair[:, 1].copy())), variant
        # render-only: the weights of the living rays of a fused launch are the stored form's
        chunk = line_chunks(wl)[0]
        RT = raytracer(spec, source=lines_source(chunk), seed=5)
        RT.trace(N_LINES)
        w, nt = RT.rays.w_list.copy(), RT.rays.Nt
        tail = TailStorage()
        RT.trace(N_LINES, _tail=tail)
        tw = tail._dev["w"].view(2, tail._cap)[0, :tail.N].cpu().numpy()
        assert bits(np.sort(tw[tw > 0]), np.sort(w[w[:, nt - 2] > 0, nt - 2])), "tail"
    if kw["spectrum_type"] == "Gaussian" and not kw.get("inverse"):
        routes = {k: v.astype(np.float32).astype(np.float64) for k, v in routes.items()}
    for route, got in routes.items():
        line, passes = wc.transmission_report(case, g, got, route)
        lines.append(line + ("" if passes else "   <-- FAILS"))
        ok &= passes
    lines.append(f"           T {case:24s} formula and lines routes differ on {int(np.count_nonzero(routes['formula'] != routes['lines']))} of {N} samples")
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert ok, "\n".join(lines)
    if kw["spectrum_type"] != "Gaussian":
        assert bits(routes["formula"], routes["lines"])


index_function, transmission_function = wc.index_function, wc.transmission_function


def test_function_spectra_on_lines_are_the_functions_values():
    """A Function medium or filter under a discrete source is tabulated at the lines (OT_N_LINES, OT_T_LINES: an exact-match
    search): every ray gets the function's own double at its wavelength, bit for bit, inverse or not."""
    wl = wc.wavelengths(999)
    with ot.global_options.no_warnings():
        seen, ns, _ = lines_route(ot.RefractionIndex("Function", func=index_function), wl)
        assert bits(ns[:, 0], index_function(seen.astype(np.float64))) and bits(ns[:, 1], ns[:, 0])
        for inverse in (False, True):
            spec = ot.TransmissionSpectrum("Function", func=transmission_function, inverse=inverse)
            seen, _, w = lines_route(spec, wl)
            T = transmission_function(seen.astype(np.float64))
            assert bits(w[:, 1], (1.0 - T if inverse else T).astype(np.float32)), inverse
    assert set(np.unique(seen)) == set(np.unique(wl))


def test_function_spectra_under_a_continuous_source_are_their_fine_table():
    """A Function medium or filter under a continuous source becomes a Data table of 65537 nodes (inverse folded in):
    every value is np.interp on that table, bit for bit (interp_tab restates NumPy's interpolation) -- on the nodes, next to
    them and between them; from the leaf-free routes of the other cases: the kernel's own index store, ot_rays_fill_index,
    the weights behind the filter, each also with a tabulated filter, an asphere or a spline lens behind and no_pol."""
    wl = wc.function_wavelengths()
    x = wl.astype(np.float64)
    ones = np.full(N, 1.0, dtype=np.float32)
    w0 = wc.weights(777)
    # (a monochromatic source is discrete: the scene would tabulate the function at its one line, and an injected ray of
    # another wavelength would find no match)
    continuous = lambda: ot.RaySource(ot.Point(), divergence="None", s=[0, 0, 1], pos=[0, 0, -5],
                                      spectrum=ot.LightSpectrum("Rectangle", wl0=380., wl1=780.))
    with ot.global_options.no_warnings():
        ri = ot.RefractionIndex("Function", func=index_function)
        want = np.interp(x, *wc.function_table(index_function))
        for variant in BEHIND + ("data_behind",):
            RT = raytracer(ri, variant, source=continuous())
            p0, s0, pol, _, _ = injected(wl, ones)
            filled, stored, _, _ = trace_both(RT, N, _initial_rays=(p0, s0, None if RT.no_pol else pol, ones, wl), _N_list=np.array([N]))
            assert bits(stored[:, 1], want) and bits(stored[:, 2], want), variant
            assert bits(filled[:, :3], stored[:, :3]), variant
        for inverse in (False, True):
            spec = ot.TransmissionSpectrum("Function", func=transmission_function, inverse=inverse)
            T = np.interp(x, *wc.function_table(transmission_function, inverse))
            for variant in BEHIND + ("data_behind",):
                RT = raytracer(spec, variant, source=continuous())
                for weights in (ones, w0):
                    p0, s0, pol, _, _ = injected(wl, weights)
                    RT.trace(N, _initial_rays=(p0, s0, None if RT.no_pol else pol, weights, wl), _N_list=np.array([N]))
                    assert bits(RT.rays.w_list[:, 1], (weights.astype(np.float64) * T).astype(np.float32)), (inverse, variant)
