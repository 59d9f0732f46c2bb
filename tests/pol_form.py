"""The basis-free form of the refraction step's float32 results (refraction_polarization of csrc/ot_trace.hpp), restated
in float64 NumPy without fused operations (which makes it a pessimistic stand-in for the device), and a seeded sweep of
rays to hold it to the exact values of the reference's formulas (refraction_cases.exact_step, mpmath).  Shared by
tests/test_pol_form_host.py and tests/test_gpu_pol_form.py.

With e = n - ns s, mm = e.e, tp = ns (s.pol) - n.pol, P = |pol|^2 - (s.pol)^2, ct = N - q ns, d1 = N ns + W, d2 = ns + N W:
    pol' = pol - (s.pol) s + (tp / mm) [(W - ns) s + (1 - ct) n]
    T    = 4 N ns W [P mm d2^2 + tp^2 (d1^2 - d2^2)] / (mm (d1 d2)^2)
below mm = NEAR:   pol' = pol - (s.pol) s,   T = 4 N ns W (P / 2) (d1^2 + d2^2) / (d1 d2)^2
n x s == 0 or s' == s bitwise:   pol' = pol and 1/2 for P / 2.
"""
from __future__ import annotations

import numpy as np

import refraction_cases as rc

NEAR = 2.0 ** -52   # OT_POL_NEAR of csrc/ot_trace.hpp

# (n1, n2): an ordinary step either way, dense media either way, and indices matched to 1e-3 either way
MEDIA = ((1.0, 1.5), (1.7, 1.0), (1.0, 1.9), (1.9, 1.0), (1.5, 1.5015), (1.5015, 1.5))
NORMALS = ("flat", "tilt_a", "tilt_b")


def basis_free_form(n, s, pol, n1, n2, near=NEAR, mm_from="e") -> dict:
    """n (3,), s (k, 3), pol (k, 3) f32 -> dict(T, pol_ (f64, before the float32 store), s_, tir).
    mm_from="ns": mm = 1 - ns^2 instead of e.e -- the cheaper form that must NOT be used (the bars catch it)."""
    n = np.broadcast_to(n, s.shape)
    pol = pol.astype(np.float64)
    N = n1 / n2
    ns = rc._rdot(n, s)
    with np.errstate(all="ignore"):
        W = np.sqrt(1 - N * N * (1 - ns * ns))
        Nns = N * ns
        q = Nns - W
        s_ = s * N - n * q[:, None]
        sp, np_ = rc._rdot(s, pol), rc._rdot(n, pol)
        P = rc._rdot(pol, pol) - sp * sp
        e = n - ns[:, None] * s
        mm = rc._rdot(e, e) if mm_from == "e" else 1 - ns * ns
        tp = ns * sp - np_
        A, B = P * mm, tp * tp
        mask = np.any(s != s_, axis=1)
        rare = ~(mm >= near) | ~mask
        m = rc._cross(n, s)
        keep = rare & (~mask | ~(rc._rdot(m, m) > 0))
        half = np.where(keep, 0.5, 0.5 * P)
        A, B, M = np.where(rare, 2 * half, A), np.where(rare, half, B), np.where(rare, 1.0, mm)
        tp = np.where(rare, 0.0, tp)
        d1, d2 = Nns + W, ns + N * W
        den = d1 * d2
        den2, d2s = den * den, d2 * d2
        rr = 1 / (M * den2)
        T = 4 * (Nns * W) * ((A * d2s + B * (d1 * d1 - d2s)) * rr)
        T = np.where(Nns == 0, np.nan, T)
        k = tp * (rr * den2)
        g, h = k * (1 - (N - q * ns)), k * (W - ns) - sp
        pol_ = pol + h[:, None] * s + g[:, None] * n
        pol_ = np.where(keep[:, None], pol, pol_)
        tir = ~np.isfinite(W)
    return dict(T=np.where(tir, 0.0, T), pol_=pol_, s_=s_, tir=tir)


def directions(normal_key: str, a: np.ndarray, rng) -> np.ndarray:
    """Unit directions at sin(alpha) = a to the normal, at random azimuths (as refraction_cases builds its ladders)."""
    n = rc.unit_normal(normal_key)
    cs = rc._unit2(rng, a.shape[0])
    if normal_key == "flat":
        return np.stack((a * cs[0], a * cs[1], np.sqrt(1 - a * a)), axis=1)
    return rc._normalized(rc._around(n, a, np.sqrt(1 - a * a), cs))


def tilted_pol(s, rng, along=2.0 ** -22) -> np.ndarray:
    """float32 pol vectors near the plane perpendicular to s with a component of up to `along` left along s: what a pol
    looks like after a few float32 stores, and more (the float32 rounding alone leaves ~2^-25)."""
    pol = rc._pol_for(s, rng).astype(np.float64)
    return (pol + rng.uniform(-along, along, s.shape[0])[:, None] * s).astype(np.float32)


def passes(n, s, N) -> np.ndarray:
    """W >= 2^-8 and no verdict within rounding of the critical angle (the `wide` class' condition)."""
    ns = rc._rdot(s, np.broadcast_to(n, s.shape))
    return (1 - N * N * (1 - ns * ns)) >= 2.0 ** -16


def sweep(a_lo=2.0 ** -30, a_hi=0.999, per_case=160, seed=20259):
    """-> list of dict(normal, n (3,), n1, n2, s (k, 3), pol (k, 3) f32): sin(alpha) log-uniform in a_lo .. a_hi, every
    normal with every pair of media, transmitted rays only."""
    out = []
    for i, nk in enumerate(NORMALS):
        for j, (n1, n2) in enumerate(MEDIA):
            rng = np.random.default_rng([seed, i, j])
            a = np.exp(rng.uniform(np.log(a_lo), np.log(a_hi), 2 * per_case))
            s = directions(nk, a, rng)
            n = rc.unit_normal(nk)
            s = s[passes(n, s, n1 / n2) & (s[:, 2] > 0.05)][:per_case]
            out.append(dict(normal=nk, n=n, n1=n1, n2=n2, s=s, pol=tilted_pol(s, rng)))
    return out


def exact(case) -> tuple:
    """-> (T (k,) longdouble, pol' (k, 3) longdouble) of the reference's formulas, exactly (mpmath)."""
    T, pol = [], []
    for r in range(case["s"].shape[0]):
        ex = rc.exact_step(case["n"], case["s"][r], case["pol"][r], case["n1"], case["n2"])
        assert ex is not None
        T.append(rc.split(ex[0]))
        pol.append([rc.split(v) for v in ex[1]])
    T, pol = np.array(T, dtype=object), np.array(pol, dtype=object)
    hi = lambda x: x[..., 0].astype(np.float64)
    lo = lambda x: x[..., 1].astype(np.float32)
    return rc.join(hi(T), lo(T)), rc.join(hi(pol), lo(pol))


def used(case, T, pol_, T_ex, pol_ex) -> tuple:
    """Fractions of the GPU test's bars that a result (float64 T and pol' before the store) uses after the float32 store,
    for unit incoming weights -> (w (k,), pol (k,)); and the same for the unrounded values against the noise part of the
    bars alone (the bars minus the store's 2^-24 and 2^-25) -> (w64, pol64)."""
    LD = rc.LD
    a = rc.sin_alpha(case["n"], case["s"])
    w0 = np.ones(T.shape[0], dtype=np.float32)
    w_bar, p_bar = rc.w_bar(w0, T_ex, a), rc.pol_bar(a)
    w = np.abs(T.astype(np.float32).astype(LD) - T_ex) / w_bar
    p = np.max(np.abs(pol_.astype(np.float32).astype(LD) - pol_ex), axis=1) / p_bar
    w64 = np.abs(T.astype(LD) - T_ex) / (w_bar - T_ex * LD(2.0 ** -24))
    p64 = np.max(np.abs(pol_.astype(LD) - pol_ex), axis=1) / (p_bar - LD(2.0 ** -25))
    return w.astype(np.float64), p.astype(np.float64), w64.astype(np.float64), p64.astype(np.float64)
