"""Preset catalogue: media, PSFs, light spectra, observer curves, spectral lines, eye models and a test image.

One module per group, with the names and list orders of optrace/tracer/presets/*.py.  The numbers are the published
coefficients and tables those files cite, restated as data tables from which the objects are built.  The photographic
and chart images of the reference are image files and are not part of this package.
"""
from . import spectral_lines
from . import refraction_index
from . import light_spectrum
from . import spectrum
from . import psf
from . import image
from . import geometry
