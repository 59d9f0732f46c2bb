"""Inputs and a NumPy oracle of the field-dependent convolution ("Field-dependent convolution"), shared by
tests/test_convolve_field_host.py and tests/test_gpu_convolve_field.py.  The oracle is written from the definition: a loop over
nodes and taps that adds shifted, weighted planes.  No FFT, nothing of the package."""
import numpy as np


def node_weights_1d(n: int, j0: int, n_in: int, G: int) -> np.ndarray:
    """(G, n): hat(t(j) - b) with t(j) = clamp((j - j0) / (n_in - 1), 0, 1) (G - 1), 0 when G = 1 or n_in = 1."""
    if G == 1 or n_in == 1:
        t = np.zeros(n)
    else:
        t = np.clip((np.arange(n) - j0) / (n_in - 1), 0.0, 1.0) * (G - 1)
    return np.maximum(0.0, 1.0 - np.abs(t[None, :] - np.arange(G, dtype=np.float64)[:, None]))


def oracle(img: np.ndarray, interior, psf: np.ndarray) -> np.ndarray:
    """img (n_ch, ny, nx), interior (y0, x0, ny_in, nx_in), psf (gy, gx, py, px) -> out (n_ch, ny + py - 1, nx + px - 1)."""
    n_ch, ny, nx = img.shape
    gy, gx, py, px = psf.shape
    y0, x0, ny_in, nx_in = interior
    wy, wx = node_weights_1d(ny, y0, ny_in, gy), node_weights_1d(nx, x0, nx_in, gx)
    out = np.zeros((n_ch, ny + py - 1, nx + px - 1))
    for b in range(gy):
        for a in range(gx):
            w = wy[b][:, None] * wx[a][None, :]
            if not w.any():
                continue
            src = img * w[None]
            for dy, dx in zip(*np.nonzero(psf[b, a])):
                out[:, dy:dy + ny, dx:dx + nx] += psf[b, a, dy, dx] * src
    return out


# ---- kernel cases: interior ny x nx with a rim of `rim` pixels around it, PSFs py x px on a gy x gx grid -----------------------
# The kernel's tiling (csrc/ot_convolve.hpp): output tiles of 16 rows x 128 columns, 8 neighbouring columns per lane; taps in
# chunks of 16 rows x 32 columns, run in blocks of 8; per chunk the nodes whose weight is not zero on the chunk's source window.
KERNEL_CASES = {
    # name: (ny, nx, py, px, gy, gx, n_ch, rim)                   which edge it crosses
    "one_pixel": (1, 1, 1, 1, 1, 1, 1, 0),                        # everything degenerate: t = 0, one tap, one lane with work
    "more_nodes_than_pixels": (7, 7, 3, 3, 9, 9, 1, 0),           # nodes between pixels never reach weight 1
    "psf_larger_than_image": (7, 33, 17, 40, 1, 2, 3, 0),         # 2 x 2 tap chunks, most of each source window outside the image
    "psf_taller_than_tiles": (33, 7, 40, 17, 2, 1, 1, 0),         # 3 tap chunks in y, 40 > 16 rows: source windows above the tile
    "exactly_one_tile": (14, 112, 3, 17, 3, 4, 1, 0),             # output 16 x 128
    "one_tile_plus_one": (15, 113, 3, 17, 3, 4, 3, 0),            # output 17 x 129: tiles with one row / one column
    "image_of_one_tile": (16, 128, 3, 3, 1, 2, 1, 0),             # the image is a tile: the output's second tiles hold 2 rows / columns
    "image_of_one_tile_plus_one": (17, 129, 3, 3, 2, 1, 1, 0),
    "many_tiles_wide": (65, 130, 17, 40, 3, 4, 3, 0),             # 6 x 2 tiles, 2 x 2 chunks, up to 4 nodes per chunk
    "many_tiles_tall": (130, 65, 40, 17, 3, 4, 1, 0),             # 11 x 1 tiles, 3 chunks in y
    "one_tap_chunk": (33, 33, 16, 32, 3, 4, 1, 0),                # taps fill one chunk exactly
    "one_tap_chunk_plus_one": (33, 33, 17, 33, 3, 4, 1, 0),       # a second chunk of one tap row / one tap column
    "tap_block_edges": (7, 130, 8, 9, 1, 2, 1, 0),                # 9 taps: a second block of 8 with one tap in it
    "one_row": (1, 130, 1, 40, 1, 2, 1, 0),                       # ny = 1: t_y = 0
    "one_column": (130, 1, 40, 1, 2, 1, 3, 0),                    # nx = 1
    "rim_small_psf": (33, 65, 1, 3, 1, 2, 1, 5),                  # interior strictly inside: clamped weights on the rim
    "rim_tall": (65, 33, 3, 1, 2, 1, 3, 5),
    "rim_large": (130, 130, 40, 40, 3, 4, 1, 5),                  # the largest: 4 * 40 * 40 + 8 terms per output
}


def kernel_inputs(name: str, delta: bool = False):
    """-> (img (n_ch, ny + 2 rim, nx + 2 rim), interior, psf (gy, gx, py, px)), non-negative, from a seed per case.  delta: every
    node's PSF is a single 1, at a tap of its own."""
    ny, nx, py, px, gy, gx, n_ch, rim = KERNEL_CASES[name]
    rng = np.random.default_rng(sorted(KERNEL_CASES).index(name) + 1000)
    img = rng.uniform(0.0, 1.0, (n_ch, ny + 2 * rim, nx + 2 * rim))
    if delta:
        psf = np.zeros((gy, gx, py, px))
        taps = rng.permutation(py * px)[:gy * gx]
        for n, t in enumerate(taps):
            psf[n // gx, n % gx, t // px, t % px] = 1.0
    else:
        psf = rng.uniform(0.0, 1.0, (gy, gx, py, px))
    return img, (rim, rim, ny, nx), psf


# ---- public function: image 56 x 72, PSFs 51 x 51 at the image's pitch ---------------------------------------------------------
NY, NX, PN = 56, 72, 51


def field_image(color: bool) -> np.ndarray:
    """sRGB values in [0.2, 0.9]: inside the gamut with a margin, so that the colour mapping of the result changes nothing."""
    yy, xx = np.mgrid[0:NY, 0:NX]
    base = 0.55 + 0.3 * np.sin(xx / 5.0) * np.cos(yy / 4.0) + 0.05 * ((xx // 9 + yy // 7) % 2)
    if not color:
        return base
    return np.stack([base, 0.55 + 0.3 * np.cos(xx / 6.0 + yy / 9.0), 0.9 - 0.7 * (xx / NX) * (yy / NY)], axis=2)


def field_sizes(m: float):
    """Side lengths of the image, and of PSFs that have the pitch of the m-scaled image."""
    img_s = [0.01 * (NX - 1), 0.01 * (NY - 1)]
    ip = np.array(img_s) * abs(m) / (np.array([NX, NY]) - 1)
    return img_s, list(ip * (PN - 1))


def blob(b: int, a: int) -> np.ndarray:
    """PSF values in [0, 1] (sRGB, as a GrayscaleImage holds them): offset and width vary with the node.  (Offsets that vary over
    the field move the light of neighbouring source pixels together or apart: a result can exceed the image's largest value, by
    13 % at the most for these offsets of 2 to 4 pixels per node, which keeps a picture of 0.79 linear below 1.)"""
    yy, xx = np.mgrid[0:PN, 0:PN]
    r2 = (xx - 25.0 - 4 * a + 2 * b) ** 2 + (yy - 25.0 + 2 * b - 2 * a) ** 2
    v = np.exp(-r2 / (14.0 + 9 * a + 5 * b))
    return v / v.max()


def to_linear(v: np.ndarray) -> np.ndarray:
    """sRGB gamma removed (IEC 61966-2-1)."""
    return np.where(v <= 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
