"""ot_image_convolve (img_convolve_kernel, csrc/ot_image.hpp), the direct kernel of the resolution filter, called on
its own with kernels that have no symmetry: include/optrace_amd.h publishes it as a convolution, and the Airy discs of
tests/test_gpu_image_modes.py look the same flipped or transposed.

Reference: the zero-padded "same"-size convolution out[y, x] = sum_jk g[j, k] f[y + ps - j, x + ps - k], summed on the host
in np.longdouble and clamped at 0 like the kernel.  Tolerance, derived: the kernel forms an f64 sum of at most n_taps
products, each product and each addition rounding by at most 2^-53 relative, so per pixel and channel
|got - ref| <= 2 n_taps 2^-53 sum |g| |f| over that pixel's window (the clamp does not widen it)."""
import numpy as np
import pytest
import torch

from optrace_amd import _capi
from optrace_amd._device import require_device, stream_ptr, ptr, to_dev
from optrace_amd.render_image import RenderImage

pytestmark = pytest.mark.gpu
OK, ERR_INVALID, ERR_UNSUPPORTED = 0, -1, -3   # OT_OK, OT_ERR_INVALID, OT_ERR_UNSUPPORTED (include/optrace_amd.h)


def gpu_convolve(img, psf, ps):
    """-> (status, out): the raw call, so that refusals can be looked at."""
    lib = _capi.load_library()
    require_device()
    Ny, Nx = img.shape[:2]
    assert psf.shape == (2 * ps + 1, 2 * ps + 1) and img.shape[2] == 4
    src, taps = to_dev(img, np.float64), to_dev(psf, np.float64)
    out = torch.full_like(src, float("nan"))
    rc = lib.ot_image_convolve(ptr(src), Nx, Ny, ptr(taps), ps, ptr(out), stream_ptr())
    return rc, out.cpu().numpy().reshape(Ny, Nx, 4)


def host_convolve(img, psf, ps):
    """-> (reference, sum |g| |f|) per pixel and channel."""
    Ny, Nx = img.shape[:2]
    pad = np.zeros((Ny + 4 * ps, Nx + 4 * ps, 4), dtype=np.longdouble)
    pad[2 * ps:2 * ps + Ny, 2 * ps:2 * ps + Nx] = img
    apad = np.abs(pad).astype(np.float64)
    ref, mass = np.zeros(img.shape, dtype=np.longdouble), np.zeros(img.shape)
    for j, k in zip(*np.nonzero(psf)):
        ys, xs = slice(3 * ps - j, 3 * ps - j + Ny), slice(3 * ps - k, 3 * ps - k + Nx)
        ref += np.longdouble(psf[j, k]) * pad[ys, xs]
        mass += abs(psf[j, k]) * apad[ys, xs]
    return np.maximum(ref, 0), mass


def random_image(rng, Ny, Nx):
    img = rng.random((Ny, Nx, 4)) * 10.0 ** rng.uniform(-3, 0, (Ny, Nx, 1))
    img[rng.random((Ny, Nx)) < 0.1] *= -1.0   # some negative pixels: the clamp at 0 has something to do (ps <= 7)
    return img


def random_taps(rng, ps):
    side = 2 * ps + 1
    return rng.random((side, side)) * (rng.random((side, side)) >= 0.3)  # 30 % exact zeros: the `g == 0.0` skip


SHAPES = [(1, 1), (3, 70), (65, 5), (40, 23)]


@pytest.mark.parametrize("Ny,Nx,ps", [(*s, ps) for s in SHAPES for ps in (0, 1, 7)] + [(40, 23, 68)])
def test_asymmetric_kernel_against_host_sum(Ny, Nx, ps):
    rng = np.random.default_rng(1000 * Ny + 10 * Nx + ps)
    img, psf = random_image(rng, Ny, Nx), random_taps(rng, ps)
    assert not np.array_equal(psf, psf[::-1]) or ps == 0
    rc, got = gpu_convolve(img, psf, ps)
    assert rc == OK
    ref, mass = host_convolve(img, psf, ps)
    bound = 2 * psf.size * 2.0 ** -53 * mass
    err = np.abs(got - ref).astype(np.float64)
    assert np.all(np.isfinite(got)) and got.min() >= 0
    assert np.all(err <= bound), f"max err / bound = {np.max(err / np.maximum(bound, 1e-300)):.3g} at {np.unravel_index(np.argmax(err - bound), err.shape)}"


@pytest.mark.parametrize("Ny,Nx,ps,j,k", [(40, 23, 7, 2, 12), (3, 70, 7, 14, 0), (65, 5, 1, 0, 2), (40, 23, 68, 70, 131),
                                          (1, 1, 1, 1, 1), (1, 1, 1, 0, 1)])
def test_single_off_centre_tap_shifts_the_image(Ny, Nx, ps, j, k):
    """One tap of 1.0 at (j, k): the output is the input moved by (j - ps, k - ps) rows and columns, zero where it came
    from outside, bit for bit.  A flipped or transposed index moves it elsewhere."""
    rng = np.random.default_rng(7)
    img = rng.random((Ny, Nx, 4))
    psf = np.zeros((2 * ps + 1, 2 * ps + 1))
    psf[j, k] = 1.0
    rc, got = gpu_convolve(img, psf, ps)
    assert rc == OK
    dy, dx = j - ps, k - ps
    want = np.zeros_like(img)
    ys = slice(max(dy, 0), min(Ny + dy, Ny))
    xs = slice(max(dx, 0), min(Nx + dx, Nx))
    if ys.start < ys.stop and xs.start < xs.stop:
        want[ys, xs] = img[ys.start - dy:ys.stop - dy, xs.start - dx:xs.stop - dx]
    assert np.array_equal(got, want)


def test_return_codes():
    img = np.ones((2, 3, 4))
    lib = _capi.load_library()
    rc, _ = gpu_convolve(img, np.ones((139, 139)), 69)
    assert rc == ERR_UNSUPPORTED and b"137" in lib.ot_last_error()
    src, taps = to_dev(img, np.float64), to_dev(np.ones((3, 3)), np.float64)
    out = torch.zeros_like(src)
    assert lib.ot_image_convolve(ptr(src), 3, 2, ptr(taps), 1, ptr(src), stream_ptr()) == ERR_INVALID   # in == out
    assert lib.ot_image_convolve(ptr(src), 3, 2, ptr(taps), -1, ptr(out), stream_ptr()) == ERR_INVALID  # ps < 0
    assert lib.ot_image_convolve(ptr(src), 0, 2, ptr(taps), 1, ptr(out), stream_ptr()) == ERR_INVALID
    torch.cuda.synchronize()
    assert torch.equal(out, torch.zeros_like(out)), "a refused call writes nothing"
    # what RenderImage sends to the direct kernel, the library accepts
    ps = RenderImage._DIRECT_PSF_MAX
    rc, got = gpu_convolve(img, np.full((2 * ps + 1, 2 * ps + 1), 0.5), ps)
    assert rc == OK and np.array_equal(got, np.full_like(img, 3.0))
