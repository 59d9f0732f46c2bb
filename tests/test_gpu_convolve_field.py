"""Field-dependent convolution on the device: the kernel behind `ot_convolve_field` through ctypes against the NumPy oracle of
tests/convolve_field_cases.py (written from the definition in DESIGN.md, "Field-dependent convolution"), and `ot.convolve_field`
against `ot.convolve`, the reference's fixtures and the oracle.

Tolerance of the kernel tests: all terms are non-negative, so a sum of n = 4 py px + 8 rounded terms lies within n 2^-53 of
the exact one, 7.1e-13 for the largest case (40 x 40 taps); device and oracle may each use that much: rtol 2e-12, atol 0."""
import numpy as np
import pytest
import torch

import optrace_amd as ot
from optrace_amd import _capi
from optrace_amd._device import ptr, stream_ptr
import convolve_field_cases as fc
from convolve_cases import convolve_cases, build_convolve_inputs
from helpers import load

pytestmark = pytest.mark.gpu
RTOL = 2e-12


def run_kernel(img: np.ndarray, interior, psf: np.ndarray) -> torch.Tensor:
    dev = torch.device("cuda")
    d_img, d_psf = torch.from_numpy(np.ascontiguousarray(img)).to(dev), torch.from_numpy(np.ascontiguousarray(psf)).to(dev)
    n_ch, ny, nx = img.shape
    gy, gx, py, px = psf.shape
    out = torch.full((n_ch, ny + py - 1, nx + px - 1), float("nan"), dtype=torch.float64, device=dev)  # (every element is written)
    _capi.check(_capi.load_library().ot_convolve_field(ptr(d_img), n_ch, ny, nx, *[int(v) for v in interior], ptr(d_psf), gy, gx,
                                                       py, px, ptr(out), stream_ptr()))
    torch.cuda.synchronize()
    return out


def close(got: np.ndarray, want: np.ndarray, what: str) -> None:
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.where(want != 0, np.abs(got - want) / np.abs(want), np.where(got == 0, 0.0, np.inf))
    print(what, "largest relative deviation", float(rel.max()), "of", RTOL)
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=0)


# ---- the kernel through ctypes -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(fc.KERNEL_CASES))
def test_kernel_matches_the_oracle(name):
    img, interior, psf = fc.kernel_inputs(name)
    close(run_kernel(img, interior, psf).cpu().numpy(), fc.oracle(img, interior, psf), name)


@pytest.mark.parametrize("name", ["many_tiles_wide", "more_nodes_than_pixels", "rim_large"])
def test_delta_psfs_pin_the_node_of_a_source_pixel(name):
    """Every node's PSF is a single 1 at a tap of its own: the output is a sum of at most four shifted, weighted copies of every
    source pixel, and a pixel that took its PSF from the wrong node lands at the wrong place."""
    img, interior, psf = fc.kernel_inputs(name, delta=True)
    close(run_kernel(img, interior, psf).cpu().numpy(), fc.oracle(img, interior, psf), name)


def test_same_call_same_bits():
    img, interior, psf = fc.kernel_inputs("many_tiles_wide")
    assert torch.equal(run_kernel(img, interior, psf), run_kernel(img, interior, psf))


@pytest.mark.parametrize("axis", [1, 2])
def test_flip_symmetry(axis):
    """Flipping the image, the order of the nodes and every PSF along an axis flips the output along it."""
    img, interior, psf = fc.kernel_inputs("rim_large")
    out = run_kernel(img, interior, psf).cpu().numpy()
    g_axis, p_axis = (0, 2) if axis == 1 else (1, 3)
    flipped = run_kernel(np.flip(img, axis), interior, np.flip(psf, (g_axis, p_axis))).cpu().numpy()
    close(np.flip(flipped, axis), out, f"flip along axis {axis}")


# ---- the public function --------------------------------------------------------------------------------------------------------------
GRAY_PSF_CASES = ["gray_gray", "gray_gray_flip_scale", "rgb_gray_edge_keep", "rgb_gray_padvalue"]


@pytest.mark.parametrize("name", GRAY_PSF_CASES)
def test_one_node_is_convolve(name):
    """`convolve_field(img, [[psf]])` against `ot.convolve(img, psf)` and against the reference's own result
    (tests/golden/convolve.npz, the assertions of tests/test_gpu_convolve.py)."""
    g = load("convolve.npz")
    case = convolve_cases()[name]
    img, psf = build_convolve_inputs(ot, case)
    with ot.global_options.no_warnings():
        want = ot.convolve(img, psf, m=case["m"], **case["kwargs"])
        res = ot.convolve_field(img, [[psf]], m=case["m"], **case["kwargs"])
    assert type(res) is type(want) and res.shape == want.shape
    np.testing.assert_allclose(res.extent, want.extent, rtol=1e-15, atol=0)
    print(name, "largest deviation from convolve", float(np.abs(res.data - want.data).max()))
    np.testing.assert_allclose(res.data, want.data, rtol=0, atol=1e-9)
    d = res.data
    assert tuple(d.shape) == tuple(g[f"{name}/shape"])
    np.testing.assert_allclose(res.extent, g[f"{name}/extent"], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(d[1::4, 2::4], g[f"{name}/grid4"], rtol=0, atol=1e-9)
    np.testing.assert_allclose(d.sum(axis=(0, 1)), g[f"{name}/sum"], rtol=1e-9)
    np.testing.assert_allclose(d.max(axis=(0, 1)), g[f"{name}/max"], rtol=0, atol=1e-9)


# Bruce Lindbloom's sRGB (D65) matrices, to seven digits as published: the result of a colour image passes through XYZ, and the two are
# inverses of each other to about 1e-7 only
RGBL_TO_XYZ = np.array([[0.4124564, 0.3575761, 0.1804375], [0.2126729, 0.7151522, 0.0721750], [0.0193339, 0.1191920, 0.9503041]])
XYZ_TO_RGBL = np.array([[3.2404542, -1.5371385, -0.4985314], [-0.9692660, 1.8760108, 0.0415560], [0.0556434, -0.2040259, 1.0572252]])


def expected_field(data: np.ndarray, psf_lin: np.ndarray, m: float, keep_size: bool, padding_mode: str) -> np.ndarray:
    """What `convolve_field` returns, un-gamma'd, from the definition: image planes with padding and flip, the oracle, the PSF's rim
    of 4 zero pixels, convolve's slicing."""
    planes = fc.to_linear(data)
    planes = planes[None] if planes.ndim == 2 else np.moveaxis(planes, 2, 0)
    ny, nx = planes.shape[1:]
    py, px = psf_lin.shape[2:]
    rim_y, rim_x = (0, 0) if padding_mode == "constant" else (py + 8, px + 8)
    if rim_y:
        planes = np.pad(planes, ((0, 0), (rim_y, rim_y), (rim_x, rim_x)), mode=padding_mode)
    if m < 0:
        planes = planes[:, ::-1, ::-1]
    full = np.pad(fc.oracle(planes, (rim_y, rim_x, ny, nx), psf_lin), ((0, 0), (4, 4), (4, 4)))
    full = full[:, rim_y:full.shape[1] - rim_y, rim_x:full.shape[2] - rim_x]
    if keep_size:
        oy, ox = (py + 8 - 1) // 2, (px + 8 - 1) // 2
        full = full[:, oy:oy + ny, ox:ox + nx]
    if full.shape[0] == 1:
        return full[0]
    rgb = np.moveaxis(full, 0, 2)
    return (rgb @ RGBL_TO_XYZ.T) @ XYZ_TO_RGBL.T  # (in gamut with a margin: the colour mapping changes nothing else)


@pytest.fixture(scope="module")
def blobs():
    lin = np.stack([np.stack([fc.to_linear(fc.blob(b, a)) for a in range(2)]) for b in range(3)])
    return lin / lin.sum(axis=(2, 3), keepdims=True)


@pytest.mark.parametrize("color,m,keep_size,padding_mode", [(False, 1.0, False, "constant"), (True, 1.0, False, "constant"),
                                                            (False, -2.0, True, "constant"), (True, 1.0, False, "edge")])
def test_grid_of_distinct_psfs(blobs, color, m, keep_size, padding_mode):
    img_s, psf_s = fc.field_sizes(m)
    data = fc.field_image(color)
    img = (ot.RGBImage if color else ot.GrayscaleImage)(data, img_s)
    psfs = [[ot.GrayscaleImage(fc.blob(b, a), psf_s) for a in range(2)] for b in range(3)]
    with ot.global_options.no_warnings():
        res = ot.convolve_field(img, psfs, m=m, keep_size=keep_size, padding_mode=padding_mode, cargs=dict(normalize=False))
    want = expected_field(data, blobs, m, keep_size, padding_mode)
    assert isinstance(res, ot.RGBImage if color else ot.GrayscaleImage) and res.data.shape == want.shape
    assert want.max() <= 1 and want.min() >= 0
    got = fc.to_linear(res.data)
    print("largest deviation from the oracle", float(np.abs(got - want).max()))
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)


def test_node_weights():
    img_s, psf_s = fc.field_sizes(1.0)
    lin = fc.to_linear(fc.field_image(False))
    img = ot.GrayscaleImage(fc.field_image(False), img_s)
    psf = ot.GrayscaleImage(fc.blob(1, 1), psf_s)
    opts = dict(cargs=dict(normalize=False))
    with ot.global_options.no_warnings():
        one = fc.to_linear(ot.convolve_field(img, [[psf]], **opts).data)
        equal = fc.to_linear(ot.convolve_field(img, [[psf, psf], [psf, psf], [psf, psf]], node_weights=np.ones((3, 2)), **opts).data)
        falling = fc.to_linear(ot.convolve_field(img, [[psf, psf]], node_weights=[[1, 0.25]], **opts).data)
        # the same picture with the illumination in the image: I (1 - 0.75 t_x), t_x = i / (nx - 1), convolved once
        t_x = np.arange(fc.NX) / (fc.NX - 1)
        from optrace_amd.image import srgb_linear_to_srgb
        shaded = ot.GrayscaleImage(srgb_linear_to_srgb(lin * (1 - 0.75 * t_x)[None, :]), img_s)
        want = fc.to_linear(ot.convolve(shaded, psf, **opts).data)
    print("equal nodes against one node", float(np.abs(equal - one).max()), "falling weights", float(np.abs(falling - want).max()))
    np.testing.assert_allclose(equal, one, rtol=0, atol=1e-12)
    np.testing.assert_allclose(falling, want, rtol=0, atol=1e-9)


def test_end_to_end_from_two_traced_field_points():
    """Plumbing, not physics: Huygens PSFs of a singlet on the axis and one degree off it, handed to `convolve_field` as they are."""
    RT = ot.Raytracer(outline=[-6, 6, -6, 6, -1, 60], no_pol=True, seed=11)
    mono = ot.LightSpectrum("Monochromatic", wl=550.0)
    RT.add(ot.RaySource(ot.CircularSurface(r=2.5), divergence="None", spectrum=mono, pos=[0, 0, 0]))
    RT.add(ot.RaySource(ot.CircularSurface(r=2.5), divergence="None", spectrum=mono, pos=[0, 0, 0], s_sph=[1.0, 90.0]))
    RT.add(ot.Lens(ot.SphericalSurface(r=4, R=30), ot.SphericalSurface(r=4, R=-25), n=ot.presets.refraction_index.BK7, pos=[0, 0, 8], d=1.5))
    with ot.global_options.no_warnings():
        RT.trace(40000)
        on = RT.huygens_psf(0, n_px=64)
        off = RT.huygens_psf(1, n_px=64, size=on.size)
    assert on.N > 15000 and off.N > 15000 and off.size == on.size
    yy, xx = np.mgrid[0:64, 0:64]
    pix = ((xx // 8 + yy // 8) % 2).astype(np.float64)
    img = ot.GrayscaleImage(pix, s=[2 * on.size, 2 * on.size])
    with ot.global_options.no_warnings():
        res = ot.convolve_field(img, [[on, off]], cargs=dict(normalize=False))
        want = ot.convolve(img, on.to_image(), cargs=dict(normalize=False))
    assert isinstance(res, ot.GrayscaleImage) and res.shape == want.shape and np.all(np.isfinite(res.data))
    np.testing.assert_allclose(res.extent, want.extent, rtol=1e-15, atol=0)
    assert fc.to_linear(res.data).sum() == pytest.approx(fc.to_linear(pix).sum(), rel=1e-9)
