"""The basis-free form of refraction_polarization (csrc/ot_trace.hpp), restated in float64 NumPy without fused operations
(tests/pol_form.py), against the exact values of the reference's formulas (mpmath) on a seeded sweep: sin(alpha) from 2^-30
to 1 on three normals, both signs of n1 - n2, indices matched to 1e-3, W >= 2^-8, and float32 pol vectors that are not
perpendicular to s.  The bars are those of tests/test_gpu_refraction_step.py (refraction_cases.w_bar, pol_bar), applied
after the float32 store; the used fractions are printed, also for the unrounded values against the noise part of the bars
alone.  CPU only.

That the bars bite is shown with the threshold (test_threshold_is_not_arbitrary).  The cheaper denominator mm = 1 - ns^2
(pol_form.basis_free_form(mm_from="ns")) was expected to break them and does not: on this sweep it uses 0.97 of the pol bar
after the store and 0.49 of its noise part before it, where e.e uses 0.93 and 0.48.  In this form the P term of T carries mm
above and below the line, tp^2 / mm is multiplied by d1^2 - d2^2 = O(sin^2), the bend of pol' is of size sin(alpha), and
below sin(alpha) ~ 2^-26.5 the difference reads 0 and takes the near-normal branch.  So no test here claims that it fails;
the kernel keeps e.e because tp is formed from the same n and s, which keeps tp^2 <= P mm when n is unit only to rounding."""
import functools

import numpy as np
import pytest

import pol_form as pf
import refraction_cases as rc

pytest.importorskip("mpmath")


@functools.lru_cache(maxsize=None)
def swept():
    """The sweep with its exact values, computed once: a coarse pass over all angles and a dense one across the threshold."""
    cases = pf.sweep(per_case=100) + pf.sweep(a_lo=2.0 ** -30, a_hi=2.0 ** -22, per_case=100, seed=20260)
    return [(c, *pf.exact(c)) for c in cases]


def worst(**form_args):
    out = np.zeros(4)
    at = [None] * 4
    for c, T_ex, pol_ex in swept():
        res = pf.basis_free_form(c["n"], c["s"], c["pol"], c["n1"], c["n2"], **form_args)
        assert not np.any(res["tir"])
        a = rc.sin_alpha(c["n"], c["s"]).astype(np.float64)
        for i, u in enumerate(pf.used(c, res["T"], res["pol_"], T_ex, pol_ex)):
            j = int(np.argmax(u))
            if not u[j] <= out[i]:   # (a NaN counts)
                out[i], at[i] = u[j], f"{c['normal']} {c['n1']} -> {c['n2']} at sin(alpha) = 2^{np.log2(a[j]):.2f}"
    return out, at


def test_sweep_covers_what_it_claims():
    a = np.concatenate([rc.sin_alpha(c["n"], c["s"]).astype(np.float64) for c, _, _ in swept()])
    assert a.min() < 2.0 ** -29.5 and a.max() > 0.9 and a.size > 3000
    near = np.sqrt(pf.NEAR)
    assert np.count_nonzero((a > near / 16) & (a < near)) > 300 and np.count_nonzero((a >= near) & (a < near * 16)) > 300
    for c, _, _ in swept():
        sp = np.abs(rc._rdot(c["s"], c["pol"].astype(np.float64)))
        assert sp.max() > 2.0 ** -24 and c["pol"].dtype == np.float32, "pol has a part along s"
    assert {np.sign(c["n1"] - c["n2"]) for c, _, _ in swept()} == {-1.0, 1.0}
    assert any(abs(c["n1"] / c["n2"] - 1) <= 1.001e-3 for c, _, _ in swept())


def test_form_keeps_the_bars(capsys):
    used, at = worst()
    with capsys.disabled():
        print(f"\nbasis-free form, threshold 2^{np.log2(pf.NEAR):.0f}: uses {used[0]:.3f} of the w bar ({at[0]}), "
              f"{used[1]:.3f} of the pol bar ({at[1]});\n  before the float32 store, of the noise part alone: w {used[2]:.2e}, "
              f"pol {used[3]:.3f} ({at[3]})")
    assert used[0] <= 1 and used[1] <= 1
    assert used[2] <= 1 and used[3] <= 1, "the form's own error stays inside the noise part of the bars"


@pytest.mark.parametrize("near", [2.0 ** -60, 2.0 ** -44])
def test_threshold_is_not_arbitrary(near, capsys):
    """Far below the chosen threshold the form's noise breaks the noise part of the pol bar, far above it the dropped term does."""
    used, at = worst(near=near)
    with capsys.disabled():
        print(f"\nthreshold 2^{np.log2(near):.0f}: pol before the store uses {used[3]:.2f} of the noise part ({at[3]})")
    assert used[3] > 1


def test_contracts_of_the_unchanged_direction():
    """n x s == 0: pol' = pol bitwise and the transmission of A_ts^2 = A_tp^2 = 1/2, on a tilted normal too, where
    e = n - (n.n) n is not zero."""
    for nk in pf.NORMALS:
        n = rc.unit_normal(nk)
        s = np.tile(n, (5, 1))
        pol = pf.tilted_pol(s, np.random.default_rng(3))
        for n1, n2 in pf.MEDIA:
            res = pf.basis_free_form(n, s, pol, n1, n2)
            assert np.array_equal(res["pol_"], pol.astype(np.float64))
            T = rc.nopol_T(n, s, n1, n2)
            assert np.max(np.abs(res["T"] - T) / T) < 2.0 ** -50
