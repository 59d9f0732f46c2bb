"""Image presets (presets/image.py).  Only the procedural one: the photographs and charts of the reference are image files
that this package does not carry."""
from __future__ import annotations

import numpy as np

from ..image import GrayscaleImage


def grid(s=None, extent=None) -> GrayscaleImage:
    """White grid of 10 x 10 cells on black, 301 px, for judging distortion.  `s`: side lengths [mm], or `extent`."""
    pixels = np.zeros((301, 301))
    pixels[::30] = 1
    pixels[:, ::30] = 1
    return GrayscaleImage(pixels, s, extent, desc="Grid")
