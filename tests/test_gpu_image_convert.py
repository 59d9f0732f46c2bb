"""ot_image_convert (csrc/ot_image.hpp, the kernels behind RenderImage.get and the colour mapping of convolve())
branch by branch: the synthetic XYZW images of tests/image_convert_cases.py against what the reference's colour functions
give for them (tests/golden/image_convert.npz, generator: tests/golden/generate_golden_image_convert.py).

The cases reach what a traced image reaches only by luck: all three sides of the gamut triangle in xy (Absolute intent)
and in u'v' (Perceptual intent), an image with no pixel inside the human gamut, the clamp of the chroma factor at 0.32,
the lightness threshold dropping the one pixel that decides the factor, the empty set, degenerate pixels (Y = 0, X = Z = 0,
all zero among lit ones, X + Y + Z < 0 -> whitepoint; the `y <= 0` arm beside it cannot be reached), an all-dark image, 1 x 1 images, both branches of Luv in both directions, the linear segment of the gamma curve, the NO_NORMALIZE and
NO_CLIP flags, pixel counts that fill neither a wave nor a workgroup.  tests/test_image_convert_fixture.py checks, without a
GPU, that the fixture really covers them.

Tolerances are those of tests/test_gpu_image_modes.py: rtol 1e-9 with atol 1e-12, hue on the circle below 1e-6 where the
chroma exceeds 1e-6, NaN positions equal.  Every pixel is compared, black ones included, except those the generator dropped
because the reference's own answer there is rounding noise (a one-ulp change of the input moves it by more than 1e-10 of
the image maximum: a sector boundary of the triangle, a chroma of noise size).  The generator records them in `<case>/keep`
and caps them at 1 % of a case's lit pixels; this fixture has none."""
import re

import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd._device import require_device, stream_ptr, ptr, to_dev
from optrace_amd.image import srgb_linear_to_srgb
from helpers import load, assert_close
from image_convert_cases import (image_convert_cases, in_gamut_linear, srgb_keys, SCALAR_MODES, PERCEPTUAL_VARIANTS,
                                 APX, K, RGBL_TO_XYZ, XYZ_TO_RGBL)

pytestmark = pytest.mark.gpu
CASES = image_convert_cases()
SRGB = {key: (mode, kw) for key, mode, kw in srgb_keys()}
KEYS = list(SRGB) + SCALAR_MODES


@pytest.fixture(scope="module")
def g():
    return load("image_convert.npz")


def convert(xyzw, mode, fact=1, L_th=0.0, chroma_scale=None, normalize=True, clip=True, rendering_intent=None):
    """One ot_image_convert call on a host (Ny, Nx, 4) image, as RenderImage.get and convolve() make it (the mode carries
    the rendering intent; the keyword is accepted so that the reference's argument sets can be passed as they are)."""
    lib = _capi.load_library()
    dev = require_device()
    Ny, Nx = xyzw.shape[:2]
    ny, nx = Ny // fact, Nx // fact
    rgb = mode.startswith("sRGB")
    code = ot.RenderImage._MODES[mode] | (0 if normalize else 0x100) | (0 if clip else 0x200)
    hist = to_dev(xyzw, np.float64)
    out = torch.full((ny * nx * (3 if rgb else 1),), float("nan"), dtype=torch.float64, device=dev)
    ws = torch.empty(4 * nx * ny + 8, dtype=torch.float64, device=dev)
    cs = float("nan") if chroma_scale is None else float(chroma_scale)
    _capi.check(lib.ot_image_convert(ptr(hist), Nx, Ny, fact, code, APX, K, float(L_th), cs, ptr(out), ptr(ws), stream_ptr()))
    return out.cpu().numpy().reshape((ny, nx, 3) if rgb else (ny, nx))


def convert_key(xyzw, key, fact=1):
    if key in SRGB:
        mode, kw = SRGB[key]
        return convert(xyzw, mode, fact, **kw)
    return convert(xyzw, key, fact)


def compare(got, ref, keep, key, chroma, what):
    assert got.shape == ref.shape, what
    if key.startswith("Hue"):  # an angle: on the circle, where a hue exists
        assert np.array_equal(np.isnan(got), np.isnan(ref)), what
        sel = keep & (chroma > 1e-6)
        diff = np.abs((got[sel] - ref[sel] + 180) % 360 - 180)
        assert diff.size == 0 or diff.max() < 1e-6, f"{what}: hue off by {diff.max()}"
    else:
        assert_close(got[keep], ref[keep], rtol=1e-9, atol=1e-12, what=what)


@pytest.mark.parametrize("key", KEYS)
@pytest.mark.parametrize("name", sorted(CASES))
def test_convert_matches_reference(g, name, key):
    xyzw = CASES[name]
    assert g[f"{name}/xyzw"].tobytes() == xyzw.tobytes(), "fixture inputs = rebuilt inputs"
    got = convert_key(xyzw, key)
    compare(got, g[f"{name}/{key}"], g[f"{name}/keep"], key, g[f"{name}/Chroma (CIELUV)"], f"{name} {key}")


def test_lightness_threshold_and_clamp_change_the_picture(g):
    """The three L_th values of `dim_outlier` give three different decisions (factor clamped at 0.32; the dim pixel dropped,
    no scaling; the empty set), and the first differs from the others where it must: in the bright pixels' saturation."""
    xyzw = CASES["dim_outlier"]
    a, b, c = (convert(xyzw, "sRGB (Perceptual RI)", L_th=v) for v in (0.0, 0.05, 1.0))
    assert np.abs(a - b).max() > 0.05 and np.abs(b - c).max() < 1e-12
    assert float(g["scalars/dim_outlier/raw"]) < 0.32 and float(g["scalars/dim_outlier/fact"]) == 0.32


@pytest.mark.parametrize("shape", [(1, 391), (391, 1), (23, 17), (16, 64)])
def test_result_does_not_depend_on_the_layout(shape):
    """The `spectral` pixels as a row, a column, transposed counts and padded with black to 16 x 64: every pixel gets the
    value it has in the 17 x 23 image, bit for bit (the image-wide quantities are maxima and minima, which no order of
    the waves changes), wherever it sits in its wave or workgroup."""
    flat = CASES["spectral"].reshape(-1, 4)
    n = flat.shape[0]
    laid = np.zeros((shape[0] * shape[1], 4))
    laid[:, 3] = 1.0
    laid[:n] = flat
    for key in KEYS:
        base = convert_key(CASES["spectral"], key)
        got = convert_key(laid.reshape(*shape, 4), key)
        ch = base.shape[2:]
        base, got = base.reshape(n, *ch), got.reshape(-1, *ch)
        if key == "Irradiance":
            assert np.array_equal(got[:n], base)
            continue
        assert np.array_equal(got[:n], base, equal_nan=True), f"{key} {shape}: {np.argwhere(got[:n] != base)[:4]}"
        assert np.all(got[n:] == base[0]), f"{key} {shape}: black padding"  # pixel 0 of the case is black


@pytest.mark.parametrize("fact", [1, 3])
def test_bin_joining_with_colour_modes(fact):
    """fact x fact bins joined before a colour mode: the result is the fact = 1 conversion of the block means.  The means
    themselves agree with NumPy's to rtol 1e-12 (Irradiance and Illuminance show W and Y); carried through one mode each
    of the sRGB, Luv and gamut families at the tolerances above.  With fact = 1 the means are the image itself: that leg
    shows only that fact = 1 joins nothing and that a second call gives the same; fact = 3 is the check of the joining."""
    flat = CASES["spectral"].reshape(-1, 4)
    img = np.resize(flat, (18 * 27, 4)).reshape(18, 27, 4)
    means = img.reshape(18 // fact, fact, 27 // fact, fact, 4).mean(axis=(1, 3))
    assert_close(convert(img, "Irradiance", fact), means[:, :, 3] / APX, rtol=1e-12, what="W means")
    assert_close(convert(img, "Illuminance", fact), K / APX * means[:, :, 1], rtol=1e-12, what="Y means")
    chroma = convert(means, "Chroma (CIELUV)")
    keep = np.ones(means.shape[:2], dtype=bool)
    for key in ("sRGB (Perceptual RI)", "sRGB (Absolute RI)", "Chroma (CIELUV)", "Hue (CIELUV)", "Outside sRGB Gamut"):
        compare(convert_key(img, key, fact), convert_key(means, key), keep, key, chroma, f"fact={fact} {key}")
    assert convert(img, "Outside sRGB Gamut", fact).sum() > 0


CARGS = {"sRGB (Absolute RI)": {},
         "sRGB (Perceptual RI)|Lth0.02": dict(rendering_intent="Perceptual", L_th=0.02),
         "sRGB (Absolute RI)|nonorm": dict(normalize=False)}


def xyz_picture(xyz):
    """(RGBImage, three PSFs) whose convolution holds exactly the XYZ colours `xyz` (n, 3), n <= 3000, repeated over
    50 x 60 pixels.  The picture carries xyz / max as its linear sRGB values; the three PSFs are single pixels whose XYZ
    (kept with their negative linear sRGB values, convolve.py:204-208) send the R, G, B channels back to max * X, Y, Z.
    convolve() goes XYZ -> linear sRGB -> XYZ with two seven-digit matrices that are inverses to 1e-7 only, so the PSF
    colours carry the inverse of that product."""
    top = xyz.max()
    lin = np.resize(xyz / top, (3000, 3)).reshape(50, 60, 3)
    img = ot.RGBImage(srgb_linear_to_srgb(lin), [0.59, 0.49])
    x2r = np.linalg.inv(RGBL_TO_XYZ @ XYZ_TO_RGBL) * top
    psfs = []
    for c in range(3):
        data = np.zeros((51, 51, 4))
        data[25, 25, :3] = x2r[:, c]
        data[25, 25, 3] = 1.0
        psf = ot.RenderImage([-0.25, 0.25, -0.25, 0.25])
        psf._data = data
        psfs.append(psf)
    return img, psfs


@pytest.mark.parametrize("key", sorted(CARGS))
def test_convolve_passes_its_colour_arguments(g, key):
    """convolve() end to end: a 50 x 60 picture of the `wide_gamut` colours comes back mapped with `cargs` -- the
    fixture's value for the same XYZ (the picture has the case's image-wide quantities; what the FFTs add, about 1e-15
    of the largest component, is far below the tolerances).  Half of the colours lie outside the sRGB gamut and the
    two dim ones decide the chroma factor, so the three expected pictures differ pairwise by far more than the tolerance
    and a rendering intent, an L_th or a normalize flag that did not reach the kernel fails here."""
    want = {k: g[f"wide_gamut/{k}"] for k in CARGS}
    for k in CARGS:
        for other in CARGS:
            assert k == other or np.abs(want[k] - want[other]).max() > 1e-3, f"{k} and {other} expect the same picture"
    img, psfs = xyz_picture(CASES["wide_gamut"][:, :, :3].reshape(-1, 3))
    with ot.global_options.no_warnings():
        res = ot.convolve(img, psfs, keep_size=True, cargs=CARGS[key])
    ref = np.resize(want[key].reshape(-1, 3), (3000, 3)).reshape(50, 60, 3)
    assert_close(res.data, ref, rtol=1e-9, atol=1e-12, what=f"convolve {key}")


def test_convolve_passes_clip(g):
    """clip=False.  An RGBImage holds values in [0, 1] only, so convolve() can return an unclipped picture only where
    clipping would have changed nothing; as in the reference, it raises otherwise.  Both halves: the lit `in_gamut`
    colours against a delta PSF come back as the fixture has them (no black pixel: round-off below zero there would
    raise), and the `invalid_only` colours, which the Perceptual intent leaves far below zero, raise with the
    smallest value the fixture holds for them unclipped -- while the same call with clip=True returns the clipped one."""
    lit = np.any(in_gamut_linear() != 0, axis=2)
    lin = np.resize(in_gamut_linear()[lit], (3000, 3)).reshape(50, 60, 3)
    img = ot.RGBImage(srgb_linear_to_srgb(lin), [0.59, 0.49])
    delta = np.zeros((51, 51))
    delta[25, 25] = 1.0
    with ot.global_options.no_warnings():
        res = ot.convolve(img, ot.GrayscaleImage(delta, [0.5, 0.5]), keep_size=True, cargs=dict(clip=False))
    ref = np.resize(g["in_gamut/sRGB (Absolute RI)|noclip"][lit], (3000, 3)).reshape(50, 60, 3)
    assert_close(res.data, ref, rtol=1e-9, atol=1e-12, what="convolve clip=False, in gamut")

    img, psfs = xyz_picture(CASES["invalid_only"][:, :, :3].reshape(-1, 3))
    clipped, unclipped = g["invalid_only/sRGB (Perceptual RI)"], g["invalid_only/sRGB (Perceptual RI)|noclip"]
    assert unclipped.min() < -0.5 and clipped.min() == 0
    with ot.global_options.no_warnings():
        res = ot.convolve(img, psfs, keep_size=True, cargs=dict(rendering_intent="Perceptual"))
        with pytest.raises(ValueError, match="negative value of") as err:
            ot.convolve(img, psfs, keep_size=True, cargs=dict(rendering_intent="Perceptual", clip=False))
    ref = np.resize(clipped.reshape(-1, 3), (3000, 3)).reshape(50, 60, 3)
    assert_close(res.data, ref, rtol=1e-9, atol=1e-12, what="convolve clip=True, invalid colours")
    low = float(re.search(r"negative value of (\S+) inside", str(err.value)).group(1))
    assert abs(low - unclipped.min()) <= 1e-9 * abs(unclipped.min()), (low, unclipped.min())


@pytest.mark.parametrize("mode", ot.RenderImage.image_modes)
def test_get_on_a_tiled_image(g, mode):
    """RenderImage.get itself, at full size: a 945 x 945 image tiled from the `spectral` case has the case's image-wide
    quantities, so every pixel reproduces its fixture value."""
    tile = lambda a: np.tile(a, (56, 42) + (1,) * (a.ndim - 2))[:945, :945]  # noqa: E731
    img = ot.RenderImage(extent=[0, 472.5, 0, 472.5])  # Apx = 0.25, as recorded
    img._data = np.ascontiguousarray(tile(CASES["spectral"]))
    assert img.Apx == APX and img.K == K
    keep, chroma = tile(g["spectral/keep"]), tile(g["spectral/Chroma (CIELUV)"])
    variants = PERCEPTUAL_VARIANTS if mode == "sRGB (Perceptual RI)" else {"": {}}
    for tag, kw in variants.items():
        res = img.get(mode, 945, **kw)
        assert type(res).__name__ == ("RGBImage" if mode.startswith("sRGB") else "ScalarImage")
        compare(res._data, tile(g[f"spectral/{mode}{tag}"]), keep, mode, chroma, f"get {mode}{tag}")
