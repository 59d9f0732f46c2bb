"""The host restatement of the focus-search cost function and direct RMS solution (tests/focus_cases.py) against what the
reference itself gave on the same dyadic lines (tests/golden/focus_lines.npz, generator
tests/golden/generate_golden_focus_lines.py).  No GPU: this pins the yardstick of tests/test_gpu_focus_kernels.py."""
import numpy as np
import pytest

import focus_cases as fc
from helpers import load, GOLDEN

RTOL = 1e-13


@pytest.fixture(scope="module")
def g():
    return load("focus_lines.npz")


def test_fixture_inputs_regenerate_byte_for_byte(g, tmp_path):
    """The lines of the archive are the ones focus_cases.lines draws today, and writing the archive's arrays again gives the
    committed bytes (fixed time stamps, sorted names)."""
    arrays = {k: g[k] for k in g.files}
    assert sorted({k.split("/")[0] for k in arrays}) == sorted(fc.FIXTURE_CASES)
    for name, args in fc.FIXTURE_CASES.items():
        pa, sb, w = fc.lines(**args)
        for key, val in (("pa", pa), ("sb", sb), ("w", w), ("z", fc.Z_SAMPLES)):
            assert g[f"{name}/{key}"].dtype == val.dtype and g[f"{name}/{key}"].tobytes() == val.tobytes(), (name, key)
        arrays[f"{name}/pa"], arrays[f"{name}/sb"], arrays[f"{name}/w"], arrays[f"{name}/z"] = pa, sb, w, fc.Z_SAMPLES
    fc.write_npz(tmp_path / "again.npz", arrays)
    assert (tmp_path / "again.npz").read_bytes() == (GOLDEN / "focus_lines.npz").read_bytes()
    assert (GOLDEN / "focus_lines.npz").stat().st_size < 300_000


def test_lines_are_dyadic_and_hold_the_stated_shares():
    pa, sb, w = fc.lines(5000, 5)
    assert np.array_equal(pa * 4096, np.round(pa * 4096)) and pa.min() >= -1 and pa.max() < 1
    assert np.array_equal(sb * 256, np.round(sb * 256)) and np.abs(sb).max() <= 0.25
    pos = w[w > 0].astype(np.float64) * 1024
    assert w.dtype == np.float32 and np.array_equal(pos, np.round(pos)) and pos.min() >= 1 and pos.max() <= 1024
    assert abs(np.mean(w == 0) - fc.ZERO_SHARE) < 0.02 and abs(np.mean(w == -1) - fc.OUT_SHARE) < 0.02
    assert np.array_equal(fc.Z_SAMPLES * 8, np.round(fc.Z_SAMPLES * 8))
    # the hits are exact: the same from a separately rounded and from a singly rounded pa + sb z
    for z in fc.Z_SAMPLES:
        a, b = fc.hit_positions(pa, sb, z), fc.hit_positions(pa, sb, z, fused=True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # extremes at weight 0: nothing of positive weight reaches the extent
    pa, sb, w = fc.lines(1025, 7, extremes_w0=True)
    for z in fc.Z_SAMPLES:
        x, y = fc.hit_positions(*fc.kept(pa, sb, w)[:2], z)
        wk = w[w >= 0]
        for v in (x, y):
            assert np.all(wk[(v == v.min()) | (v == v.max())] == 0)
    pa, sb, w = fc.lines(1025, 6, fan=True)
    assert not pa[:, 1].any() and not sb[:, 1].any()
    pa, sb, w = fc.lines(65, 8, cross=3.125)
    x, y = fc.hit_positions(pa, sb, 3.125)
    assert np.all(x == 0.25) and np.all(y == -0.125)


def test_fused_rounding_is_exact_on_general_lines():
    """hit_positions(fused=True) against exact rational arithmetic on lines that are not dyadic."""
    from fractions import Fraction
    rng = np.random.default_rng(11)
    pa, sb, z = rng.normal(size=(400, 2)), rng.normal(size=(400, 2)) * 0.1, 13.7
    x, y = fc.hit_positions(pa, sb, z, fused=True)
    for i in range(400):
        assert x[i] == float(Fraction(pa[i, 0]) + Fraction(sb[i, 0]) * Fraction(z))
        assert y[i] == float(Fraction(pa[i, 1]) + Fraction(sb[i, 1]) * Fraction(z))
    xs, _ = fc.hit_positions(pa, sb, z)
    assert np.any(xs != x) and np.all(np.abs(xs - x) <= 2.0 ** -52 * (np.abs(x) + np.abs(sb[:, 0] * z)))  # by the roundings of product and sum


@pytest.mark.parametrize("name", list(fc.FIXTURE_CASES))
def test_restatement_reproduces_the_reference(g, name):
    """Costs to 1e-13 relative where finite; non-finite values (and zeros) in kind and sign."""
    pa, sb, w = g[f"{name}/pa"], g[f"{name}/sb"], g[f"{name}/w"]
    ref = g[f"{name}/cost"]
    assert ref.shape == (3, 4)
    for i, z in enumerate(g[f"{name}/z"]):
        got = fc.cost_terms(pa, sb, w, float(z))["costs"]
        for j, method in enumerate(fc.METHODS):
            assert fc.same_kind(got[j], ref[i, j]), (name, z, method, got[j], ref[i, j])
            if np.isfinite(ref[i, j]):
                assert abs(got[j] - ref[i, j]) <= RTOL * abs(ref[i, j]), (name, z, method, got[j], ref[i, j])
    d = fc.direct_solution(pa, sb, w, fc.BOUNDS)
    x, fun = float(g[f"{name}/x"]), float(g[f"{name}/fun"])
    assert abs(d["x"] - x) <= RTOL * 16, (d["x"], x)
    assert fc.same_kind(d["fun"], fun)
    if np.isfinite(fun):
        assert abs(d["fun"] - fun) <= RTOL * abs(fun), (d["fun"], fun)


def test_fixture_holds_the_degenerate_values(g):
    """Two rays, one of weight 0: nan / inf / finite / -0.0.  The fan: -inf for the irradiance variance, -0.0 for the centre
    sharpness.  The direct solution of the two-ray case has no spread to minimise: the middle of the bounds."""
    c = g["n2_w0/cost"]
    assert np.all(np.isnan(c[:, 0])) and np.all(c[:, 1] == np.inf) and np.all(np.isfinite(c[:, 2])) and np.all(c[:, 2] < 0)
    assert np.all(c[:, 3] == 0) and np.all(np.signbit(c[:, 3]))
    f = g["fan1025/cost"]
    assert np.all(f[:, 1] == -np.inf) and np.all(f[:, 3] == 0) and np.all(np.signbit(f[:, 3])) and np.all(np.isfinite(f[:, [0, 2]]))
    assert float(g["n2_w0/x"]) == 8.0 and np.isnan(float(g["n2_w0/fun"]))
    assert 0 < float(g["n1025/x"]) < 16 and 0 < float(g["fan1025/x"]) < 16   # two unclipped solutions
    assert fc.n_px_for(2_249_999) == 101 and fc.n_px_for(2_250_000) == 201 and fc.n_px_for(2) == 101
