"""The focus-search kernels (csrc/ot_focus.hpp: ot_focus_prepare, ot_focus_cost, ot_focus_moments) against a host
restatement in np.longdouble (tests/focus_cases.py, itself pinned to the reference by tests/test_focus_host.py).

a. ot_focus_cost on dyadic lines: hit positions are exact, pixel indices identical, pixel sums exact -- extent and image
   must be bit-equal at every size, including a workgroup chunk with more distinct pixels than the LDS hash has slots
   (OT_FHASH_N = 4096), chunks longer than a workgroup, and trailing workgroups without rays.
b. ot_focus_moments on the same lines.
c. ot_focus_prepare against NumPy on traced rays.
d. The five fixture scenes of test_gpu_focus.py, evaluated on the host from the device's own lines: every one of the 320
   samples of every curve within the bounds of a.

Tolerances are derived, none is measured.  u = 2^-53.  An f64 sum of T rounded terms taken in any order (lanes, waves,
workgroups, atomics) errs by at most (T + c) u sum |terms|; c counts the roundings inside one term.  From that, with
e_p <= k_p u I_p the error of a pixel sum of k_p weights (0 on dyadic lines):
  Image Sharpness          g = sum d^2 over the T = 2 n_px (n_px - 1) neighbour differences d: an error E = e_p + e_q of d
                           moves g by D = sum (2 |d| E + E^2), the roundings by (T + 8) u (g + D): absolute bound on g.
  Image Center Sharpness   the window 1 + cos(pi R) is formed from X, Y (1 rounding each, |X| <= 1), R (3 u), pi R (2 roundings
                           of a value below 4.45), cos (2 ulp of a value below 1) and the addition: 32 u absolute covers
                           it.  Windowed pixels then err by e0 = e_p win + I_p (32 u + u win); their sum s by
                           sum e0 + (n_px^2 + 2) u (s + sum e0), g as above from e0, and cost = g / s^2 by the quotient of
                           the relative errors plus 4 u.
  Irradiance Variance      over the m lit pixels: S relative sum e / S + (m + 2) u, so the mean by delta = |mean| times that;
                           V = sum (v - mean)^2 moves by sum (2 |a| eps + eps^2) + 2 delta sum eps + m delta^2 with
                           a = v - mean, eps = e + 2 u |a| (a mean error alone only adds m delta^2, since sum a = 0), the
                           roundings by (m + 8) u of that; V / m / Ap^2 adds 10 u relative; through the logarithm the
                           relative bound r becomes -log(1 - r) absolute, plus 4 u |cost| for the two logarithms.
  RMS Spot Size            compared in variance: the mean errs by delta = (n + 4) u (sum |w x| / W + |mean|), which only
                           adds W delta^2 to V = sum w (x - mean)^2; the roundings (n + 8) u of that;
                           fact = W - W2 / W errs by (2 n + 6) u (W + W2 / W); 8 u for the final operations.
The moment sums and the public quantities formed from them have their bounds stated at the tests of b."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd._device import ptr, stream_ptr, to_dev, require_device
import focus_cases as fc
from focus_cases import LD, U
from helpers import load
from test_gpu_focus import CASES as SCENE_CASES
from test_gpu_parity import gpu_trace

pytestmark = pytest.mark.gpu
WS = _capi.FOCUS_WS
HASH_SLOTS = 4096   # OT_FHASH_N
WIN_ERR = 32 * U
RATIOS = {}         # largest error / bound seen per quantity


def note(key, err, bound):
    """Keep (and print, when it rises) the largest error / bound per quantity: the figures of DESIGN.md section 7."""
    err, bound = np.asarray(err, dtype=np.float64), np.asarray(bound, dtype=np.float64)
    ok = np.isfinite(err) & (bound > 0)
    if np.any(ok) and float(np.max(err[ok] / bound[ok])) > RATIOS.get(key, -1.0):
        RATIOS[key] = float(np.max(err[ok] / bound[ok]))
        print(f"ratio {key}: {RATIOS[key]:.3g}")


# ---- bounds -----------------------------------------------------------------------------------------------------------
def _grad_move(a, e):
    """sum over the neighbour differences of 2 |d| E + E^2."""
    out = LD(0)
    for d, E in ((a[1:] - a[:-1], e[1:] + e[:-1]), (a[:, 1:] - a[:, :-1], e[:, 1:] + e[:, :-1])):
        out += (2 * np.abs(d) * E + E * E).sum()
    return out


def pixel_error(t):
    return t["cnt"] * LD(U) * t["img_ld"]


def sharp_bound(t):
    D = _grad_move(t["img_ld"], pixel_error(t))
    g = t["sharp"]["g"]
    return float(D + (t["sharp"]["T"] + 8) * U * (g + D))


def center_bound(t):
    c, img, win = t["center"], t["img_ld"], t["center"]["win"].astype(LD)
    e0 = pixel_error(t) * win + img * (WIN_ERR + U * win)
    D = _grad_move(c["im0"], e0)
    dg = D + (c["T"] + 8) * U * (c["g"] + D)
    ds = e0.sum() + (img.size + 2) * U * (c["s"] + e0.sum())
    if c["s"] == 0 or c["g"] == 0:
        return float(dg)
    rg, rs = dg / c["g"], ds / c["s"]
    cost = c["g"] / (c["s"] * c["s"])
    return float(cost * ((1 + rg) / (1 - rs) ** 2 - 1) + 4 * U * cost)


def irr_bound(t):
    r = t["irr"]
    v, m = r["v"], r["m"]
    e = r["k"] * LD(U) * v
    a = v - r["mean"]
    delta = abs(r["mean"]) * (e.sum() / r["S"] + (m + 2) * U)
    eps = e + 2 * U * np.abs(a)
    D = (2 * np.abs(a) * eps + eps * eps).sum() + 2 * delta * eps.sum() + m * delta * delta
    rel = (D + (m + 8) * U * (r["V"] + D)) / r["V"] + 10 * U
    return float(-np.log1p(-rel) + 4 * U * abs(r["cost"]))


def rms_var_bound(r):
    n, W = r["n"], r["W"]
    dx, dy = (n + 4) * U * (r["Ax"] / W + abs(r["mx"])), (n + 4) * U * (r["Ay"] / W + abs(r["my"]))
    Dm = W * (dx * dx + dy * dy)
    V = r["Vx"] + r["Vy"]
    dV = Dm + (n + 8) * U * (V + Dm)
    rf = (2 * n + 6) * U * (W + r["W2"] / W) / r["fact"]
    return float(r["var"] * (dV / V + rf / (1 - rf) + 8 * U))


def check_cost(key, mode, got, t):
    """One device cost against the host terms t of the same z: kind and sign where not finite, the derived bound else."""
    want = t["costs"][mode]
    assert fc.same_kind(got, want), (key, fc.METHODS[mode], got, want)
    if not np.isfinite(want) or want == 0:
        return
    if mode == 0:
        err, bound = abs(LD(got) ** 2 - t["rms"]["var"]), rms_var_bound(t["rms"])
    else:
        err, bound = abs(LD(got) - LD(want)), (None, irr_bound, sharp_bound, center_bound)[mode](t)
    note(fc.METHODS[mode], float(err), bound)
    assert err <= bound, (key, fc.METHODS[mode], got, want, float(err), bound)


# ---- a. ot_focus_cost on dyadic lines -----------------------------------------------------------------------------------
def cu_count():
    return torch.cuda.get_device_properties(0).multi_processor_count


COST_CASES = {
    **fc.FIXTURE_CASES,
    "n64": dict(n=64, seed=9),
    "extremes_w0": dict(n=1025, seed=7, extremes_w0=True),
    "chunk2048": dict(n=lambda: 1024 * cu_count() + 1, seed=10),   # chunks of 2048 rays, trailing workgroups empty
    "overflow": dict(n=2_250_000, seed=11, out=0.0),         # n_px = 201, more than 4096 distinct pixels in one chunk
}
BIG = ("overflow",)


@functools.lru_cache(maxsize=None)
def cost_case(name):
    """-> lines, z samples, host terms per z; computed once, shared, read-only."""
    args = dict(COST_CASES[name])
    if callable(args["n"]):
        args["n"] = args["n"]()
    pa, sb, w = fc.lines(**args)
    zs = fc.Z_SAMPLES[1:] if name in BIG else fc.Z_SAMPLES
    n_px = fc.n_px_for(int(np.count_nonzero(w >= 0)))
    terms = {float(z): fc.cost_terms(pa, sb, w, float(z), n_px) for z in zs}
    dev = (to_dev(np.concatenate([pa[:, 0], pa[:, 1], sb[:, 0], sb[:, 1]]), np.float64), to_dev(w, np.float32))
    return pa, sb, w, zs, n_px, terms, dev


def focus_cost(dev, mode, zs, n_px):
    """-> cost[len(zs)], extent slots, image left in the workspace; workspace and costs start as NaN."""
    lib = _capi.load_library()
    pasb, w = dev
    ws = torch.full((WS + n_px * n_px,), float("nan"), dtype=torch.float64, device=require_device())
    out = torch.full((len(zs),), float("nan"), dtype=torch.float64, device=require_device())
    zs = np.ascontiguousarray(zs, dtype=np.float64)
    _capi.check(lib.ot_focus_cost(w.shape[0], ptr(pasb), ptr(w), mode, zs.ctypes.data_as(C.POINTER(C.c_double)), len(zs), n_px,
                                  ptr(ws), ptr(out), stream_ptr()))
    h = ws.cpu().numpy()
    return out.cpu().numpy(), h[:4], h[WS:].reshape(n_px, n_px)


def bin_chunks(n):
    """The pieces focus_bin_kernel cuts n rays into: one workgroup of 1024 per piece, at most one per compute unit."""
    groups = min(-(-n // 1024), cu_count())
    chunk = -(-(-(-n // groups)) // 1024) * 1024
    return groups, chunk


@pytest.mark.parametrize("name", list(COST_CASES))
def test_cost_on_dyadic_lines(name):
    pa, sb, w, zs, n_px, terms, dev = cost_case(name)
    n = w.shape[0]
    groups, chunk = bin_chunks(n)
    if name == "chunk2048":
        assert chunk == 2048 and groups == cu_count() and (groups // 2 + 1) * chunk >= n, (groups, chunk)   # the later half starts past n
    if name in BIG:
        assert n_px == 201 and chunk > 1024
        wk = w[w >= 0]
        for z in zs:   # (no ray is left out in this case: positions in the kept arrays are positions in the launch)
            pix = terms[float(z)]["pix"]
            most = max(np.unique(pix[s:s + chunk][wk[s:s + chunk] > 0]).size for s in range(0, n, chunk))
            assert most > HASH_SLOTS, (z, most)
    if name == "extremes_w0":
        for z in zs:
            x, y = fc.hit_positions(*fc.kept(pa, sb, w)[:2], float(z))
            assert all(np.all(w[w >= 0][(v == v.min()) | (v == v.max())] == 0) for v in (x, y))
    if name in fc.FIXTURE_CASES:
        recorded = load("focus_lines.npz")[f"{name}/cost"]
    batch = list(zs) + [zs[0]]
    for mode in range(4):
        runs = [(batch, focus_cost(dev, mode, batch, n_px))] + [([z], focus_cost(dev, mode, [z], n_px)) for z in zs]
        for zlist, (cost, ext, img) in runs:
            assert cost.shape == (len(zlist),)
            for z, c in zip(zlist, cost):
                check_cost((name, z), mode, float(c), terms[float(z)])
            last = terms[float(zlist[-1])]
            assert np.array_equal(ext, last["ext"]), (name, mode, ext, last["ext"])
            if mode:
                assert np.array_equal(img, last["img"]), (name, mode, zlist[-1], np.count_nonzero(img != last["img"]))
        # batch, single and repeated samples: each is within the bound of the same host value, so they agree within two
        b = runs[0][1][0]
        assert fc.same_kind(float(b[0]), float(b[-1]))
        if name in fc.FIXTURE_CASES:   # the recorded reference values, within the bound plus the f64 rounding of the record
            for i, z in enumerate(zs):
                t, got, ref = terms[float(z)], float(runs[1 + i][1][0][0]), float(recorded[i, mode])
                assert fc.same_kind(got, ref)
                if np.isfinite(ref) and ref != 0:
                    assert abs(ref - t["costs"][mode]) <= 1e-13 * abs(ref)
                    if mode:
                        bound = (None, irr_bound, sharp_bound, center_bound)[mode](t) + 1e-13 * abs(ref)
                        assert abs(got - ref) <= bound, (name, z, mode, got, ref)
                    else:
                        assert abs(got ** 2 - ref ** 2) <= rms_var_bound(t["rms"]) + 3e-13 * ref ** 2, (name, z, got, ref)


def test_cost_refuses_bad_arguments():
    lib = _capi.load_library()
    require_device()
    P, z = C.c_void_p(8), (C.c_double * 1)(1.0)   # (never followed: refused before)
    for args in [(0, P, P, 0, z, 1, 101, P, P), (5, P, P, 4, z, 1, 101, P, P), (5, P, P, 1, z, 1, 1, P, P), (5, P, P, 1, z, 0, 101, P, P),
                 (5, None, P, 0, z, 1, 101, P, P), (5, P, P, 0, z, 1, 101, None, P)]:
        assert lib.ot_focus_cost(*args, None) == -1 and b"ot_focus_cost" in lib.ot_last_error()


# ---- b. ot_focus_moments ----------------------------------------------------------------------------------------------
MOMENT_CASES = {k: v for k, v in COST_CASES.items() if k not in ("n2_w0",) + BIG}
MOMENT_CASES["cross"] = dict(n=1025, seed=12, cross=3.125)
MOMENT_CASES["stride"] = dict(n=lambda: 2048 * cu_count() + 1, seed=13)   # 8 workgroups of 256 per compute unit, then the stride loop


def device_moments(dev, b0, b1):
    lib = _capi.load_library()
    pasb, w = dev
    sums = torch.full((16,), float("nan"), dtype=torch.float64, device=require_device())
    _capi.check(lib.ot_focus_moments(w.shape[0], ptr(pasb), ptr(w), b0, b1, ptr(sums), stream_ptr()))
    return sums.cpu().numpy()


def centring_errors(sm, b0, b1):
    """Bounds on the rounding of the constants focus_moments2_kernel forms in f64 from the means mp = sums[1..2] / sums[0],
    ms = sums[3..4] / sums[0] (each operation rounds by u; P bounds every intermediate |mp| + |ms| max |b|):
    pb0, m0: 2 roundings -> 2 u P;  v = (pb1 - pb0) / (b1 - b0): (4 u P + u P) / (b1 - b0) + u |ms| <= 6 u P / (b1 - b0)
    for b1 - b0 >= 1.  The division that forms a mean rounds too: u |mean|, inside P.  -> (d_pb0, d_v, d_m0) per axis max."""
    W = sm[0]
    P = max(abs(sm[1] / W) + abs(sm[3] / W) * max(abs(b0), abs(b1)), abs(sm[2] / W) + abs(sm[4] / W) * max(abs(b0), abs(b1)))
    return 3 * U * P, 6 * U * P / (b1 - b0) + U * max(abs(sm[3] / W), abs(sm[4] / W)), 3 * U * P


@pytest.mark.parametrize("name", list(MOMENT_CASES))
def test_moments_on_dyadic_lines(name):
    """sums[0..4], [7] against longdouble sums: (n + 3) u sum |terms| (one product per term).  sums[5], [6], [8..13] against
    longdouble sums about the device's own means: the summation bound (n + 8) u sum |terms| plus what the f64 rounding of the
    centring constants moves them by (first derivatives from focus_cases.moment_sums, second order added).
    z_best = -s6 / s5 against the direct solution about the exact means: the errors E5, E6 of the two sums -- summation,
    plus the derivatives times the mean errors (n + 3) u sum |w pa| / W and so on -- give |dz| <= (E6 + |z| E5) / (s5 - E5).
    The closed-form variance against the longdouble covariance form, compared in variance: every one of the six sums has
    non-negative terms or terms bounded by Cauchy-Schwarz, 2 |dz| sum |w x0 sx| <= s8 + dz^2 s10, so
    4 (n + 8) u (|s8 + s11| + 2 |dz| |s9 + s12| + dz^2 (s10 + s13)) / fact covers summation (factor 2), the rounding of fact and
    of the evaluation; the mean error adds W (d_m0 + |dz| d_ms)^2 / fact."""
    if name in COST_CASES:
        pa, sb, w, _, _, _, dev = cost_case(name)
    else:
        args = dict(MOMENT_CASES[name])
        if callable(args["n"]):
            args["n"] = args["n"]()
        pa, sb, w = fc.lines(**args)
        dev = (to_dev(np.concatenate([pa[:, 0], pa[:, 1], sb[:, 0], sb[:, 1]]), np.float64), to_dev(w, np.float32))
    b0, b1 = fc.BOUNDS
    sm = device_moments(dev, b0, b1)
    assert np.all(np.isfinite(sm[:14]))
    n = int(np.count_nonzero(w >= 0))
    S, M, _ = fc.moment_sums(pa, sb, w, b0, b1)
    for k in (0, 1, 2, 3, 4, 7):
        err, bound = abs(LD(sm[k]) - S[k]), (n + 3) * U * M[k]
        note("moments direct sums", float(err), float(bound))
        assert err <= bound, (name, k, sm[k], float(S[k]), float(err), float(bound))
    # about the device's means
    means = [sm[k] / sm[0] for k in (1, 2, 3, 4)]
    Sd, Md, pt = fc.moment_sums(pa, sb, w, b0, b1, means=means)
    d_pb0, d_v, d_m0 = centring_errors(sm, b0, b1)
    W2, W = pt["W2"], pt["W"]
    move = {5: pt["dS5_dv"] * d_v + 2 * W2 * d_v ** 2, 6: pt["dS6_dv"] * d_v + pt["dS6_dp"] * d_pb0 + 2 * W2 * d_v * d_pb0,
            8: pt["dS8_dm"] * d_m0 + W * d_m0 ** 2, 11: pt["dS11_dm"] * d_m0 + W * d_m0 ** 2,
            9: pt["dS9_dm"] * d_m0, 12: pt["dS12_dm"] * d_m0, 10: 0, 13: 0}
    for k in (5, 6, 8, 9, 10, 11, 12, 13):
        err, bound = abs(LD(sm[k]) - Sd[k]), (n + 8) * U * (Md[k] + move[k]) + move[k]
        note("moments centred sums", float(err), float(bound))
        assert err <= bound, (name, k, sm[k], float(Sd[k]), float(err), float(bound))

    # the direct solution
    ref = fc.direct_solution(pa, sb, w, (b0, b1))
    mass = M[1:5]
    e_mp, e_ms = float((n + 4) * U * max(mass[0], mass[1]) / W), float((n + 4) * U * max(mass[2], mass[3]) / W)
    t_pb0, t_v = e_mp + e_ms * max(abs(b0), abs(b1)) + d_pb0, e_ms + d_v
    Sx, Mx, px = ref["S"], ref["M"], ref["parts"]
    E5 = (n + 8) * U * Mx[5] + px["dS5_dv"] * t_v + 2 * W2 * t_v ** 2
    E6 = (n + 8) * U * Mx[6] + px["dS6_dv"] * t_v + px["dS6_dp"] * t_pb0 + 2 * W2 * t_v * t_pb0
    assert Sx[5] > E5
    z_dev = -sm[6] / sm[5]
    err, bound = abs(LD(z_dev) - ref["unclipped"]), (E6 + abs(ref["unclipped"]) * E5) / (Sx[5] - E5) + 2 * U * abs(ref["unclipped"])
    note("moments z_best", float(err), float(bound))
    assert err <= bound, (name, z_dev, float(ref["unclipped"]), float(err), float(bound))

    # the quadratic cost curve, in variance
    fact = sm[0] - sm[7] / sm[0]
    z0 = 0.5 * (b0 + b1)
    for z in fc.Z_SAMPLES:
        dz = z - z0
        got = (sm[8] + sm[11] + 2 * dz * (sm[9] + sm[12]) + dz ** 2 * (sm[10] + sm[13])) / fact
        want = fc.variance_at(pa, sb, w, float(z))
        scale = (abs(sm[8] + sm[11]) + 2 * abs(dz) * abs(sm[9] + sm[12]) + dz ** 2 * (sm[10] + sm[13])) / fact
        bound = 4 * (n + 8) * U * scale + float(W) * (d_m0 + e_mp + (abs(z0) + abs(dz)) * e_ms) ** 2 / fact
        err = abs(LD(got) - want)
        note("moments variance curve", float(err), bound)
        assert err <= bound, (name, z, got, float(want), float(err), bound)
        if name == "cross" and z == 3.125:   # all lines meet here: the true variance is 0
            assert want == 0 and np.isfinite(got)
            cost = float(np.sqrt(max(got, 0.0)))   # as Raytracer.focus_search forms it
            assert np.isfinite(cost) and cost <= np.sqrt(bound), (cost, bound)


# ---- c. ot_focus_prepare against NumPy on traced rays ------------------------------------------------------------------
N_LIST = np.array([65, 935])


@functools.lru_cache(maxsize=None)
def traced_scene():
    """Two sources with 65 and 935 injected rays; ring aperture (hole) at z = 5, lens at z = 10, Gaussian filter at z = 20;
    some rays leave through the side of the outline, some miss the hole, some are absorbed by the filter."""
    with ot.global_options.no_warnings():
        RT = ot.Raytracer(outline=[-3, 3, -3, 3, -5, 40], no_pol=True)
        for x in (-0.5, 0.5):
            RT.add(ot.RaySource(ot.CircularSurface(r=1), divergence="None", s=[0, 0, 1], pos=[x, 0, -3],
                                spectrum=ot.LightSpectrum("Monochromatic", wl=550.)))
        RT.add(ot.Aperture(ot.RingSurface(r=2.5, ri=1.2), pos=[0, 0, 5]))
        RT.add(ot.Lens(ot.SphericalSurface(r=2.5, R=12), ot.SphericalSurface(r=2.5, R=-12), de=0.1, pos=[0, 0, 10],
                       n=ot.RefractionIndex("Constant", n=1.5)))
        RT.add(ot.Filter(ot.CircularSurface(r=2.5), pos=[0, 0, 20], spectrum=ot.TransmissionSpectrum("Gaussian", mu=550., sig=30.)))
        N = int(N_LIST.sum())
        rng = np.random.default_rng(21)
        p0 = np.zeros((N, 3))
        p0[:, :2] = rng.uniform(-1.5, 1.5, (N, 2))
        p0[:, 2] = -3.0
        s0 = np.zeros((N, 3))
        s0[:, :2] = rng.normal(0, 0.04, (N, 2))
        s0[::7, 0] = rng.uniform(0.3, 0.6, s0[::7].shape[0])    # steep: out through the side of the outline in front of the aperture
        s0[:, 2] = 1.0
        s0 /= np.linalg.norm(s0, axis=1)[:, None]
        w0 = rng.uniform(0.2, 1.0, N).astype(np.float32)
        w0[::11] = 0.0
        wl = rng.uniform(400., 700., N).astype(np.float32)
        RT.trace(N, _initial_rays=(p0, s0, None, w0, wl), _N_list=N_LIST)
    return RT


def host_prepare(RT, first, count, z):
    """Section index argmax(z < p_z) - 1 per ray, rays without one left out; s = normalised difference of neighbouring
    positions, sb = s / s_z, pa = p - sb p_z."""
    P, Wl = RT.rays.p_list[first:first + count], RT.rays.w_list[first:first + count]
    nt = P.shape[1]
    k = np.argmax(z < P[:, :, 2], axis=1) - 1
    used = k >= 0
    i = np.arange(count)
    kk = np.where(used, k, 0)
    k1 = np.where(kk < nt - 1, kk + 1, kk)
    p = P[i, kk]
    d = P[i, k1] - p
    with np.errstate(all="ignore"):
        s = d / np.sqrt(d[:, 0] ** 2 + d[:, 1] ** 2 + d[:, 2] ** 2)[:, None]
        sb = s[:, :2] / s[:, 2:3]
    pa = p[:, :2] - sb * p[:, 2:3]
    w = np.where(used, Wl[i, kk], np.float32(-1)).astype(np.float32)
    return used, p, np.where(used[:, None], pa, 0.0), np.where(used[:, None], sb, 0.0), w


def device_prepare(RT, first, count, z):
    lib = _capi.load_library()
    dev = require_device()
    pasb = torch.full((4 * count,), float("nan"), dtype=torch.float64, device=dev)
    w = torch.full((count,), float("nan"), dtype=torch.float32, device=dev)
    nu = torch.full((1,), -7, dtype=torch.int64, device=dev)
    rays = RT.rays._rays_struct()
    _capi.check(lib.ot_focus_prepare(C.byref(rays), first, count, z, ptr(pasb), ptr(w), ptr(nu), stream_ptr()))
    h = pasb.cpu().numpy().reshape(4, count)
    return int(nu.item()), h[:2].T, h[2:].T, w.cpu().numpy()


@pytest.mark.parametrize("si", [None, 0, 1])
def test_prepare_against_numpy(si):
    """n_use, the set of rays left out and w exact.  sb within 2 ulp: the normalisation (three squares, two additions, a
    square root, a division) and the division by s_z are IEEE operations in the same order on both sides, contraction is off.
    pa within 2 u (|p_x| + |sb p_z|): one product, one subtraction, which allows one contraction."""
    RT = traced_scene()
    assert np.array_equal(RT.rays.N_list, N_LIST)
    first, end = RT._ray_range(si)
    count = end - first
    assert (first != 0) == (si == 1)
    pz_ap = RT.rays.p_list[first:end, 1, 2]
    vals, counts = np.unique(pz_ap[RT.rays.w_list[first:end, 1] > 0], return_counts=True)
    z_on = float(vals[np.argmax(counts)])   # the stored p_z, bit for bit, of most rays that pass the hole of the flat aperture
    on = pz_ap == z_on
    assert np.count_nonzero(on) >= 10
    seen_out = seen_w0 = 0
    for z in (-4.0, 1.0, z_on, 15.0, 30.0):
        used, p, pa, sb, w = host_prepare(RT, first, count, z)
        n_use, dpa, dsb, dw = device_prepare(RT, first, count, z)
        assert n_use == np.count_nonzero(used), (si, z, n_use)
        assert np.array_equal(dw == -1, ~used) and np.array_equal(dw, w), (si, z)
        assert np.all(np.abs(dsb - sb) <= 2 * np.spacing(np.abs(sb))), (si, z, np.abs(dsb - sb).max())
        assert np.all(np.abs(dpa - pa) <= 2 * U * (np.abs(p[:, :2]) + np.abs(sb * p[:, 2:3])) * used[:, None]), (si, z)
        note("prepare pa", np.abs(dpa - pa)[used].ravel(), (2 * U * (np.abs(p[:, :2]) + np.abs(sb * p[:, 2:3])))[used].ravel())
        if z == -4.0:
            assert n_use == 0   # in front of every ray's start
        elif z == z_on:   # strict z < p_z: the section behind the aperture, and the rays it absorbed are out
            k = np.argmax(z < RT.rays.p_list[first:end, :, 2], axis=1) - 1
            assert np.all(k[on & used] >= 1) and np.count_nonzero(on & used) >= 10 and np.count_nonzero(on & ~used) > 0
        else:
            assert 0 < n_use
        seen_out += np.count_nonzero(~used)
        seen_w0 += np.count_nonzero(w == 0)
    assert seen_out > 0
    n_use, dpa, dsb, dw = device_prepare(RT, first, 0, 1.0)   # count = 0: n_use is reset, nothing else is touched
    assert n_use == 0 and dw.shape == (0,)


# ---- d. the fixture scenes on the device's own lines ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def scene_lines(cname):
    """-> RT, the RMS result of focus_search, and the lines ot_focus_prepare gives for the search it ran (host copies)."""
    tname, si = SCENE_CASES[cname]
    _, RT = gpu_trace(tname)
    f = load("focus.npz")
    with ot.global_options.no_warnings():
        res0, d0 = RT.focus_search(RT.focus_search_methods[0], float(f[f"{cname}/z_start"]), source_index=si, return_cost=True,
                                   _z_samples=f[f"{cname}/0/z"])
    first, end = RT._ray_range(si)
    n_use, pa, sb, w = device_prepare(RT, first, end - first, d0["bounds"][0] + RT.N_EPS)
    assert n_use == d0["N"] == int(f[f"{cname}/0/N"])
    return RT, res0, d0, n_use, pa, sb, w


@pytest.mark.parametrize("mi", [1, 2, 3])
@pytest.mark.parametrize("cname", list(SCENE_CASES))
def test_scene_curves_on_the_device_lines(cname, mi):
    """Every sample of the three image curves within the bounds of a, on lines that c pins.  pa + sb z is formed both
    separately rounded and singly rounded; a sample at which some ray changes its pixel between the two may match either,
    at most 1 of 320 per curve (expected: none: 6.4e5 ray-samples, each within rounding of a pixel edge with about 1e-13)."""
    RT, _, _, n_use, pa, sb, w = scene_lines(cname)
    f = load("focus.npz")
    n_px = fc.n_px_for(n_use)
    pk, sk, wk = fc.kept(pa, sb, w)
    zs = f[f"{cname}/{mi}/z"]
    with ot.global_options.no_warnings():
        _, d = RT.focus_search(RT.focus_search_methods[mi], float(f[f"{cname}/z_start"]), source_index=SCENE_CASES[cname][1],
                               return_cost=True, _z_samples=zs)
    assert d["cost"].shape == zs.shape == (320,)
    ambiguous = 0
    for z, got in zip(zs, d["cost"]):
        t = fc.cost_terms(pa, sb, w, float(z), n_px)
        xy = fc.hit_positions(pk, sk, float(z), fused=True)
        if np.array_equal(t["pix"], fc.pixel_indices(*xy, n_px)[0]):
            check_cost((cname, z), mi, float(got), t)
            continue
        ambiguous += 1
        try:
            check_cost((cname, z), mi, float(got), t)
        except AssertionError:
            check_cost((cname, z), mi, float(got), fc.cost_terms(pa, sb, w, float(z), n_px, xy=xy))
    print(f"ambiguous samples {cname} {fc.METHODS[mi]}: {ambiguous}")
    assert ambiguous <= 1, (cname, mi, ambiguous)


@pytest.mark.parametrize("cname", list(SCENE_CASES))
def test_scene_rms_result_on_the_device_lines(cname):
    """res.x, res.fun and the mean position of the RMS search against the restatement of b on the device's lines."""
    RT, res0, d0, n_use, pa, sb, w = scene_lines(cname)
    bounds = d0["bounds"]
    pk, sk, wk = fc.kept(pa, sb, w)
    # RMS: direct solution and mean position from the moments
    ref = fc.direct_solution(pa, sb, w, bounds)
    dev = (to_dev(np.concatenate([pa[:, 0], pa[:, 1], sb[:, 0], sb[:, 1]]), np.float64), to_dev(w, np.float32))
    sm = device_moments(dev, bounds[0], bounds[1])
    n = n_use
    S, M, pt = ref["S"], ref["M"], ref["parts"]
    W, W2 = pt["W"], pt["W2"]
    d_pb0, d_v, d_m0 = centring_errors(sm, bounds[0], bounds[1])
    bmax = max(abs(bounds[0]), abs(bounds[1]))
    e_mp, e_ms = float((n + 4) * U * max(M[1], M[2]) / W), float((n + 4) * U * max(M[3], M[4]) / W)
    t_pb0, t_v = e_mp + e_ms * bmax + d_pb0, e_ms + d_v
    E5 = (n + 8) * U * M[5] + pt["dS5_dv"] * t_v + 2 * W2 * t_v ** 2
    E6 = (n + 8) * U * M[6] + pt["dS6_dv"] * t_v + pt["dS6_dp"] * t_pb0 + 2 * W2 * t_v * t_pb0
    zb = ref["unclipped"]
    assert bounds[0] <= res0.x <= bounds[1]
    if S[5] == 0:   # a parallel bundle has no spread of directions to minimise: the middle of the bounds, as the reference
        assert sm[5] == 0 and res0.x == 0.5 * (bounds[0] + bounds[1]) == ref["x"]
    else:           # (clipping to the bounds moves two values no further apart)
        assert S[5] > E5, (cname, float(S[5]), float(E5))
        bound = float((E6 + abs(zb) * E5) / (S[5] - E5) + 2 * U * abs(zb))
        note("scene z_best", abs(res0.x - ref["x"]), bound)
        assert abs(res0.x - ref["x"]) <= bound, (cname, res0.x, ref["x"], bound)
    # res.fun: the variance at res.x, bound as in b; the lines are not dyadic here, so x0 = pa + sb z0 rounds by pos_err per ray,
    # which moves s8 by at most 2 pos_err sum w |x0| <= 2 pos_err sqrt(W s8) and s9 by pos_err sqrt(W s10) (Cauchy-Schwarz)
    fact = sm[0] - sm[7] / sm[0]
    z0 = 0.5 * (bounds[0] + bounds[1])
    dz = res0.x - z0
    scale = (abs(sm[8] + sm[11]) + 2 * abs(dz) * abs(sm[9] + sm[12]) + dz ** 2 * (sm[10] + sm[13])) / fact
    pos_err = 2 * U * float(np.max(np.abs(pk) + np.abs(sk) * abs(z0)))   # of one x0 = pa + sb z0: a product and a sum round
    shift = d_m0 + e_mp + (abs(z0) + abs(dz)) * e_ms
    want = fc.variance_at(pa, sb, w, float(res0.x))
    vbound = (4 * (n + 8) * U * scale + float(W) * shift ** 2 / fact
              + 2 * pos_err * float(np.sqrt(2 * W)) * (np.sqrt(sm[8] + sm[11]) + abs(dz) * np.sqrt(sm[10] + sm[13])) / fact)
    note("scene variance", abs(res0.fun ** 2 - float(want)), vbound)
    assert abs(LD(res0.fun) ** 2 - want) <= vbound, (cname, res0.fun, float(np.sqrt(want)), vbound)
    # mean position at res.x: two sums of n terms each, a product, an addition, a division
    Wm, sums, mass = fc.mean_line(pk, sk, wk)
    for c in range(2):
        want_p = (sums[c] + sums[2 + c] * LD(res0.x)) / Wm
        pbound = (n + 6) * U * (mass[c] + mass[2 + c] * abs(res0.x)) / Wm + (n + 6) * U * abs(want_p)
        note("scene pos", abs(d0["pos"][c] - float(want_p)), float(pbound))
        assert abs(LD(d0["pos"][c]) - want_p) <= pbound, (cname, c, d0["pos"][c], float(want_p))
    assert d0["pos"][2] == res0.x
