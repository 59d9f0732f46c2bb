"""Spectrum presets: the CIE 1931 2° colour matching functions (presets/spectrum.py)."""
from __future__ import annotations

import numpy as np

from ..spectrum import Spectrum, _tables

_observers = _tables["observers"]   # columns: wavelength [nm], x, y, z


def _observer(column: int):
    def f(wl):
        return np.interp(wl, _observers[:, 0], _observers[:, column], left=0, right=0)
    f.__name__ = f"{'xyz'[column - 1]}_observer"
    return f


for _column, _name in enumerate("xyz", start=1):
    globals()[_name] = Spectrum("Function", func=_observer(_column), desc=_name, quantity="Relative Response", unit="",
                                long_desc=f"CIE 1931 2° {_name} observer")

xyz_observers: list = [x, y, z]   # noqa: F821 (set in the loop above)

#: every spectrum preset
all_presets: list = [*xyz_observers]
