"""tests/golden/image_convert.npz without a GPU: its inputs are what tests/image_convert_cases.py builds today, and
the branch counts its generator recorded (tests/golden/generate_golden_image_convert.py) still meet the conditions the
GPU tests rest on.  A regenerated fixture that quietly lost a branch fails here."""
import numpy as np
import pytest

from helpers import load
from image_convert_cases import image_convert_cases, srgb_keys, SCALAR_MODES

CASES = image_convert_cases()


@pytest.fixture(scope="module")
def g():
    return load("image_convert.npz")


def test_inputs_are_rebuilt_bit_for_bit(g):
    assert sum(c.shape[0] * c.shape[1] for c in CASES.values()) <= 1500
    for name, xyzw in CASES.items():
        assert xyzw.dtype == np.float64 and xyzw.ndim == 3 and xyzw.shape[2] == 4
        assert g[f"{name}/xyzw"].tobytes() == xyzw.tobytes() and g[f"{name}/xyzw"].shape == xyzw.shape, name
        assert np.all(xyzw[:, :, 3] > 0), "any positive power"
    assert CASES["spectral"].shape[:2] == (17, 23) and CASES["in_gamut"].shape[:2] == (5, 13)
    assert CASES["px1_in_gamut"].shape[:2] == CASES["px1_spectral"].shape[:2] == (1, 1)
    assert not np.any(CASES["dark"][:, :, :3])


def test_every_mode_and_variant_is_recorded(g):
    for name, xyzw in CASES.items():
        for key, _, _ in srgb_keys():
            assert g[f"{name}/{key}"].shape == (*xyzw.shape[:2], 3)
        for mode in SCALAR_MODES:
            assert g[f"{name}/{mode}"].shape == xyzw.shape[:2]
        assert g[f"{name}/keep"].shape == xyzw.shape[:2] and g[f"{name}/keep"].dtype == bool


def test_branch_coverage_and_drop_shares(g):
    cov = lambda name, k: int(g[f"coverage/{name}/{k}"])  # noqa: E731
    for k in ("xy_bg", "xy_gr", "xy_br", "uv_bg", "uv_gr", "uv_br"):   # every side of both gamut triangles
        assert cov("spectral", k) >= 20, k
    for k in ("t_above", "t_below", "L_above", "L_below"):             # both Luv branches, both ways
        assert cov("spectral", k) >= 20, k
    assert cov("spectral", "gamma_above") >= 20 and cov("spectral", "gamma_below") >= 20
    # the odd arm of the gamma curve below the negative knee, which only clip=False reaches: most of the case's 15 pixels
    assert cov("invalid_only", "gamma_negative") >= 10
    neg = [g[f"invalid_only/{key}"] for key, _, _ in srgb_keys() if "noclip" in key]
    assert max(np.count_nonzero(np.any(a < -12.92 * 0.0031308, axis=2)) for a in neg) == cov("invalid_only", "gamma_negative")
    for name, xyzw in CASES.items():
        lit = np.count_nonzero(np.any(xyzw[:, :, :3] != 0, axis=2))
        dropped = np.count_nonzero(~g[f"{name}/keep"])
        assert cov(name, "lit") == lit and cov(name, "dropped") == dropped
        assert dropped <= 0.01 * lit, f"{name}: {dropped} of {lit} lit pixels dropped"


def test_image_wide_branches(g):
    sc = lambda name, k: float(g[f"scalars/{name}/{k}"])  # noqa: E731
    # the clamp of the chroma factor: active / inactive with a factor strictly inside (0.32, 1) / the empty set
    assert sc("dim_outlier", "raw") < 0.32 and sc("dim_outlier", "fact") == 0.32
    assert sc("dim_outlier", "raw|Lth0.05") >= 1 and sc("dim_outlier", "fact|Lth0.05") == 1
    assert np.isnan(sc("dim_outlier", "raw|Lth1")) and sc("dim_outlier", "fact|Lth1") == 1
    for name in ("spectral", "px1_spectral"):
        assert 0.32 < sc(name, "raw") < 1 and sc(name, "fact") == sc(name, "raw")
    assert sc("spectral", "fact|Lth0.02") != sc("spectral", "fact"), "L_th changes the result"
    # no pixel inside the human gamut and no black pixel: the all-ones branch
    assert sc("invalid_only", "any_valid") == 0 and sc("invalid_only", "any_inv") == 1
    assert np.all(CASES["invalid_only"][:, :, 1] > 0)
    # nothing out of gamut: only a given chroma_scale takes the long way
    assert sc("in_gamut", "any_inv") == 0 and sc("px1_in_gamut", "any_inv") == 0
    assert sc("dark", "rgbmax") == 0 and sc("dark", "Lmax") == 0
    # degenerate pixels are there, and NaN positions (if the reference has any) are part of the record
    d = CASES["degenerate"].reshape(-1, 4)
    assert np.any((d[:, 1] == 0) & (d[:, 0] > 0) & (d[:, 2] > 0)) and np.any((d[:, 0] == 0) & (d[:, 2] == 0) & (d[:, 1] > 0))
    assert np.any(np.all(d[:, :3] == 0, axis=1))
    # X + Y + Z <= 0 with a negative linear sRGB value: the whitepoint arm of the Absolute intent
    assert np.any((d[:, :3].sum(axis=1) <= 0) & np.any(d[:, :3] < 0, axis=1))
    assert not any(np.any(np.isnan(g[f"degenerate/{key}"])) for key, _, _ in srgb_keys())
    # the picture convolve() is tested with: every colour argument it passes on changes the expected result
    w = [g[f"wide_gamut/{k}"] for k in ("sRGB (Absolute RI)", "sRGB (Absolute RI)|nonorm", "sRGB (Perceptual RI)",
                                        "sRGB (Perceptual RI)|Lth0.02")]
    assert all(np.abs(a - b).max() > 1e-3 for i, a in enumerate(w) for b in w[:i])
    assert sc("wide_gamut", "fact") != sc("wide_gamut", "fact|Lth0.02") and sc("wide_gamut", "any_inv") == 1
