"""Light spectrum presets: CIE standard illuminants, sRGB primary spectra, line combinations (presets/light_spectrum.py)."""
from __future__ import annotations

from . import spectral_lines as _lines
from ..image import SRGB_PRIMARY_POWER_FACTORS, srgb_r_primary, srgb_g_primary, srgb_b_primary
from ..spectrum import LightSpectrum, illuminant


def _srgb_white(wl):
    return srgb_r_primary(wl) + srgb_g_primary(wl) + srgb_b_primary(wl)


# ---- standard illuminants: (family, CIE name); the attribute is the lower-case name with "_" for "-"
_ILLUMINANTS = [("standard_natural", "A"), ("standard_natural", "C"), ("standard_natural", "D50"),
                ("standard_natural", "D55"), ("standard_natural", "D65"), ("standard_natural", "D75"),
                ("standard_natural", "E"),
                ("standard_f", "F2"), ("standard_f", "F7"), ("standard_f", "F11"),
                ("standard_led", "LED-B1"), ("standard_led", "LED-B2"), ("standard_led", "LED-B3"),
                ("standard_led", "LED-B4"), ("standard_led", "LED-B5"), ("standard_led", "LED-BH1"),
                ("standard_led", "LED-RGB1"), ("standard_led", "LED-V1"), ("standard_led", "LED-V2")]

#: illuminants A, C, E and the daylight series
standard_natural: list = []
#: fluorescent lamps
standard_f: list = []
#: LED lamps
standard_led: list = []

for _family, _name in _ILLUMINANTS:
    _spec = LightSpectrum("Function", func=illuminant(_name), desc=_name,
                          long_desc=f"Illuminant {_name}")
    globals()[_name.lower().replace("-", "_")] = _spec
    globals()[_family].append(_spec)

standard: list = [*standard_natural, *standard_f, *standard_led]

# ---- one possible set of sRGB primary spectra, and their sum
_SRGB = [("srgb_r", srgb_r_primary, "R", "sRGB R Primary"), ("srgb_g", srgb_g_primary, "G", "sRGB G Primary"),
         ("srgb_b", srgb_b_primary, "B", "sRGB B Primary"), ("srgb_w", _srgb_white, "W", "sRGB White Spectrum")]

srgb: list = []
for _attr, _func, _desc, _long_desc in _SRGB:
    globals()[_attr] = LightSpectrum("Function", func=_func, desc=_desc, long_desc=_long_desc)
    srgb.append(globals()[_attr])

#: power ratios with which the three primaries mix to white
srgb_r_power_factor, srgb_g_power_factor, srgb_b_power_factor = SRGB_PRIMARY_POWER_FACTORS

# ---- line combinations: (attribute, lines, powers, desc, long_desc); rgb_lines mixes to D65 white
_LINES = [("FDC", _lines.FDC, [1, 1, 1], "Lines FDC", "Spectral Lines F, D, C"),
          ("FdC", _lines.FdC, [1, 1, 1], "Lines FdC", "Spectral Lines F, d, C"),
          ("FeC", _lines.FeC, [1, 1, 1], "Lines Fec", "Spectral Lines F, e, C"),
          ("F_eC_", _lines.F_eC_, [1, 1, 1], "Lines F'eC'", "Spectral Lines F', e, C'"),
          ("rgb_lines", _lines.rgb, [0.5745000, 0.5985758, 0.3895581], "RGB Lines'", "sRGB Primary Dominant Wavelengths")]

lines: list = []
for _attr, _wls, _vals, _desc, _long_desc in _LINES:
    globals()[_attr] = LightSpectrum("Lines", lines=_wls, line_vals=_vals, desc=_desc, long_desc=_long_desc)
    lines.append(globals()[_attr])

#: every light spectrum preset
all_presets: list = [*standard, *lines, *srgb]
