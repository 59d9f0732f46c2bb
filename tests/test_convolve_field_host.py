"""Field-dependent convolution without a device: the oracle of tests/convolve_field_cases.py against the definition's own
consequences, the argument checks of `ot.convolve_field` (all raised before a device is asked for), and the refusals of the C
entry `ot_convolve_field` (all before any device call)."""
import ctypes as C
import pathlib
import re

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi
import convolve_field_cases as fc


# ---- the oracle against itself ----------------------------------------------------------------------------------------------------
def _oracle_inputs():
    rng = np.random.default_rng(5)
    img = rng.uniform(0.0, 1.0, (1, 53, 67))
    psf = rng.uniform(0.0, 1.0, (51, 51))
    return img, psf / psf.sum()


def test_oracle_equal_psfs_are_one_node():
    """Partition of unity: the same PSF at all nodes of a 3 x 2 grid is the one-node sum."""
    img, psf = _oracle_inputs()
    one = fc.oracle(img, (0, 0, 53, 67), psf[None, None])
    grid = fc.oracle(img, (0, 0, 53, 67), np.broadcast_to(psf, (3, 2, 51, 51)).copy())
    dev = float(np.abs(grid - one).max())
    print("equal PSFs against one node: largest deviation", dev)
    assert dev <= 1e-13


def test_oracle_keeps_the_sum_for_unit_sum_psfs():
    img, psf = _oracle_inputs()
    rng = np.random.default_rng(6)
    psfs = rng.uniform(0.0, 1.0, (3, 2, 51, 51))
    psfs /= psfs.sum(axis=(2, 3), keepdims=True)
    out = fc.oracle(img, (0, 0, 53, 67), psfs)
    print("sum out", out.sum(), "sum img", img.sum())
    assert out.sum() == pytest.approx(img.sum(), rel=1e-12)
    # with sums s[b][a]: sum out = sum_{j,i} I sum_{b,a} W[b][a] s[b][a]
    s = rng.uniform(0.5, 2.0, (3, 2))
    wy, wx = fc.node_weights_1d(53, 0, 53, 3), fc.node_weights_1d(67, 0, 67, 2)
    want = sum(s[b, a] * (img[0] * wy[b][:, None] * wx[a][None, :]).sum() for b in range(3) for a in range(2))
    assert fc.oracle(img, (0, 0, 53, 67), psfs * s[:, :, None, None]).sum() == pytest.approx(want, rel=1e-12)


def test_oracle_weights():
    """Nodes sit at the interior's edges and fractions; rim pixels take the nearest edge's weights; degenerate axes give t = 0."""
    w = fc.node_weights_1d(9 + 4, 2, 9, 3)  # interior [2, 11), nodes at pixels 2, 6, 10
    assert np.array_equal(w[:, 2], [1, 0, 0]) and np.array_equal(w[:, 6], [0, 1, 0]) and np.array_equal(w[:, 10], [0, 0, 1])
    assert np.array_equal(w[:, 0], w[:, 2]) and np.array_equal(w[:, 12], w[:, 10])
    assert np.allclose(w.sum(axis=0), 1, atol=1e-15) and np.allclose(w[:, 4], [0.5, 0.5, 0])
    assert np.array_equal(fc.node_weights_1d(5, 0, 1, 3), [[1] * 5, [0] * 5, [0] * 5])
    assert np.array_equal(fc.node_weights_1d(5, 0, 5, 1), [[1] * 5])


# ---- ot.convolve_field: every error on the host -------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    import sys

    def reached():
        pytest.fail("require_device() reached: the check was to be made on the host")
    monkeypatch.setattr(sys.modules["optrace_amd.convolve"], "require_device", reached)


def _gray(n=60, s=(0.5, 0.5), **kw):
    return ot.GrayscaleImage(np.full((n, n) if isinstance(n, int) else n, 0.5), list(s), **kw)


def test_convolve_field_argument_errors(no_device):
    img = _gray(60, (1, 1))
    rgb = ot.RGBImage(np.full((60, 60, 3), 0.5), [1, 1])
    psf = _gray()
    ri = ot.RenderImage([-0.25, 0.25, -0.25, 0.25])
    cf = ot.convolve_field
    with ot.global_options.no_warnings():
        # the grid
        for bad in ([], [[]], [[psf, psf], [psf]], [[psf], []]):
            with pytest.raises(ValueError):
                cf(img, bad)
        with pytest.raises(TypeError):
            cf(img, psf)                          # a single PSF is [[psf]]
        with pytest.raises(TypeError):
            cf(img, [psf, psf])
        with pytest.raises(TypeError):
            cf(img, [[psf, 3.0]])
        # PSFs of unequal shape or extent, in the reference's words
        with pytest.raises(ValueError, match="All PSF sizes need to be the same"):
            cf(img, [[psf, _gray(61)]])
        with pytest.raises(ValueError, match="All PSF sizes need to be the same"):
            cf(img, [[psf], [_gray(60, (0.4, 0.5))]])
        with pytest.raises(ValueError, match="All PSF sizes need to be the same"):
            cf(img, [[psf, ot.GrayscaleImage(np.full((60, 60), 0.5), extent=[-0.2, 0.3, -0.25, 0.25])]])
        # colour PSFs
        with pytest.raises(TypeError, match="not supported by convolve_field"):
            cf(img, [[ri]])
        with pytest.raises(TypeError, match="not supported by convolve_field"):
            cf(rgb, [[psf, [ri, ri, ri]]])
        # node_weights
        for bad in (np.ones((2, 1)), [1.0, 1.0], [[1.0, -0.5]], [[np.nan, 1.0]], [[np.inf, 1.0]], [[0.0, 0.0]]):
            with pytest.raises(ValueError, match="node_weights"):
                cf(img, [[psf, psf]], node_weights=bad)
        # the caps, named
        with pytest.raises(ValueError, match=str(_capi.CONVF_MAX_GRID)):
            cf(img, [[psf] * (_capi.CONVF_MAX_GRID + 1)])
        with pytest.raises(ValueError, match=str(_capi.CONVF_MAX_GRID)):
            cf(img, [[psf]] * (_capi.CONVF_MAX_GRID + 1))
        big = ot.GrayscaleImage(np.full((1200, 1200), 0.5), [1, 1])  # pitch of the PSF at 600 pixels per half the image: 600 > 512
        with pytest.raises(ValueError, match=str(_capi.CONVF_MAX_PSF)):
            cf(big, [[_gray()]])
        # convolve's own checks of the arguments, the image and a single PSF
        with pytest.raises(TypeError):
            cf(img, [[psf]], m="1")
        with pytest.raises(ValueError):
            cf(img, [[psf]], m=0)
        with pytest.raises(TypeError):
            cf(img, [[psf]], keep_size=1)
        with pytest.raises(TypeError):
            cf(img, [[psf]], cargs=None)
        with pytest.raises(TypeError):
            cf(np.zeros((60, 60)), [[psf]])
        with pytest.raises(ValueError):
            cf(rgb, [[psf]], padding_value=[0.1, 0.2])
        with pytest.raises(ValueError):
            cf(img, [[psf]], padding_value=-1.0)
        with pytest.raises(ValueError, match="two times"):
            cf(img, [[_gray(60, (3, 3))]])
        with pytest.raises(ValueError, match="at least 50"):
            cf(img, [[_gray((40, 60))]])
        with pytest.raises(ValueError, match="at least 50"):
            cf(_gray((40, 60), (1, 1)), [[psf]])
        with pytest.raises(ValueError, match="4MP"):
            cf(img, [[_gray((2001, 2000))]])
        with pytest.raises(ValueError, match="4MP"):
            cf(_gray((2001, 2000), (1, 1)), [[psf]])


def test_convolve_field_takes_a_huygens_psf_through_its_image(no_device):
    """A HuygensPSF node is its `to_image()`: one without a usable ray has none, and says so before a device is asked for."""
    from optrace_amd.psf import _empty
    with pytest.raises(RuntimeError, match="No usable ray"):
        ot.convolve_field(_gray(60, (1, 1)), [[_empty(0, None, None, 8, None, 0.0)]])


# ---- the C entry ---------------------------------------------------------------------------------------------------------------------
def test_c_entry_checks_its_arguments_before_anything_else():
    """`ot_convolve_field` (include/optrace_amd.h): null pointers, n_ch outside 1..3, sizes below 1 and an interior outside the
    plane are OT_ERR_INVALID, sizes above the caps OT_ERR_UNSUPPORTED, each with the entry's name in `ot_last_error`, all before
    a device is looked for (the pointers are host memory that is never dereferenced)."""
    lib = _capi.load_library()
    buf = (C.c_double * 8)()
    p = C.c_void_p(C.addressof(buf))
    st = C.c_void_p()
    good = dict(img=p, n_ch=1, ny=8, nx=8, y0=0, x0=0, ny_in=8, nx_in=8, psf=p, gy=1, gx=1, py=3, px=3, out=p)

    def call(**kw):
        a = good | kw
        rc = lib.ot_convolve_field(a["img"], a["n_ch"], a["ny"], a["nx"], a["y0"], a["x0"], a["ny_in"], a["nx_in"], a["psf"], a["gy"],
                                   a["gx"], a["py"], a["px"], a["out"], st)
        assert b"ot_convolve_field" in lib.ot_last_error(), (kw, lib.ot_last_error())
        return rc

    for name in ("img", "psf", "out"):
        assert call(**{name: None}) == -1 and b"null argument" in lib.ot_last_error()
    for n_ch in (0, 4, -1):
        assert call(n_ch=n_ch) == -1 and b"n_ch" in lib.ot_last_error()
    for name in ("ny", "nx", "ny_in", "nx_in", "gy", "gx", "py", "px"):
        for v in (0, -3):
            assert call(**{name: v}) == -1, (name, v)
    for kw in (dict(y0=-1), dict(x0=-1), dict(y0=1), dict(x0=1), dict(ny_in=9), dict(nx_in=9), dict(y0=2, ny_in=7), dict(x0=2**31 - 1)):
        assert call(**kw) == -1 and b"interior" in lib.ot_last_error(), kw
    assert call(y0=1, x0=2, ny_in=7, nx_in=6, py=_capi.CONVF_MAX_PSF + 1) == _capi.ERR_UNSUPPORTED
    assert call(px=_capi.CONVF_MAX_PSF + 1) == _capi.ERR_UNSUPPORTED and b"512" in lib.ot_last_error()
    assert call(gy=_capi.CONVF_MAX_GRID + 1) == _capi.ERR_UNSUPPORTED and b"64" in lib.ot_last_error()
    assert call(gx=_capi.CONVF_MAX_GRID + 1) == _capi.ERR_UNSUPPORTED
    assert call(ny=2**20, ny_in=2**20, nx=2**11, nx_in=2**11) == _capi.ERR_UNSUPPORTED and b"2^31" in lib.ot_last_error()


def test_capi_constants_are_the_headers():
    header = (pathlib.Path(ot.__file__).resolve().parent.parent / "include" / "optrace_amd.h").read_text()
    value = lambda name: int(re.search(rf"#define {name}\s+(\d+)", header).group(1))
    assert _capi.CONVF_MAX_PSF == value("OT_CONVF_MAX_PSF") >= 256
    assert _capi.CONVF_MAX_GRID == value("OT_CONVF_MAX_GRID") == 64
    assert _capi.ABI_VERSION == value("OT_ABI_VERSION") == 9, "entries were added, none changed"
    assert "ot_convolve_field" in _capi.SIGNATURES and re.search(r"\bint ot_convolve_field\(", header)
