"""Refractive index presets: 22 glasses, 14 plastics, 9 other media (presets/refraction_index.py).

The coefficients are those of the sources named per entry (refractiveindex.info pages of the SCHOTT catalogue and of the
cited papers, eyewiki.org/Lens_Material_Properties for the Abbe media).  Every entry of `_TABLE` is
(name, group, model, parameters, desc, long_desc); the objects are built from it below and become module attributes.
"""
from __future__ import annotations

import numpy as np

from ..refraction_index import RefractionIndex


def _resonances(*pairs) -> list:
    """Sellmeier1 coefficients from (B, resonance wavelength in um) pairs: the sources give the wavelength, the formula
    takes its square."""
    return [v for B, lam in pairs for v in (B, lam ** 2)]


def _soda_lime(wl):
    """Clear soda lime silica, refractiveindex.info 3d/glass/soda-lime-clear (wl in nm)."""
    um = wl * 1e-3
    return 1.5130 - 0.003169 * um ** 2 + 0.003962 * um ** -2


#: wavelengths of the tabulated media [nm]
_TABLE_WLS = 380 + 10 * np.arange(41)

_PEI = [1.66217, 1.65853, 1.65489, 1.65125, 1.64792, 1.64503, 1.64280, 1.64096, 1.63893, 1.63755, 1.63586, 1.63415,
        1.63333, 1.63220, 1.63076, 1.62948, 1.62900, 1.62795, 1.62746, 1.62653, 1.62629, 1.62609, 1.62439, 1.62401,
        1.62392, 1.62250, 1.62273, 1.62204, 1.62185, 1.62057, 1.62139, 1.62040, 1.62058, 1.61972, 1.61996, 1.61953,
        1.61865, 1.61865, 1.61975, 1.61784, 1.61865]
_PET = [1.61891, 1.61459, 1.61027, 1.60595, 1.60212, 1.59847, 1.59528, 1.59247, 1.58988, 1.58716, 1.58496, 1.58304,
        1.58111, 1.57927, 1.57769, 1.57630, 1.57470, 1.57333, 1.57194, 1.57086, 1.56993, 1.56904, 1.56811, 1.56696,
        1.56627, 1.56527, 1.56478, 1.56368, 1.56317, 1.56225, 1.56199, 1.56131, 1.56052, 1.56013, 1.55933, 1.55868,
        1.55854, 1.55817, 1.55795, 1.55723, 1.55583]
_PVC = [1.56439, 1.56287, 1.56135, 1.55983, 1.55812, 1.55625, 1.55491, 1.55388, 1.55236, 1.55145, 1.55010, 1.54940,
        1.54850, 1.54761, 1.54692, 1.54626, 1.54533, 1.54493, 1.54389, 1.54325, 1.54275, 1.54238, 1.54137, 1.54114,
        1.54073, 1.54004, 1.53987, 1.53987, 1.53946, 1.53880, 1.53812, 1.53791, 1.53754, 1.53727, 1.53732, 1.53674,
        1.53593, 1.53544, 1.53569, 1.53528, 1.53526]
_ICE = [1.32145, 1.3203, 1.3194, 1.3185, 1.3177, 1.3170, 1.3163, 1.3157, 1.3151, 1.3145, 1.3140, 1.3135, 1.3130, 1.3126,
        1.3121, 1.3117, 1.3114, 1.3110, 1.3106, 1.3103, 1.3100, 1.3097, 1.3094, 1.3091, 1.3088, 1.3085, 1.3083, 1.3080,
        1.3078, 1.3076, 1.3073, 1.3071, 1.3069, 1.3067, 1.3065, 1.3062, 1.3060, 1.3059, 1.3057, 1.3055, 1.3053]

_S1 = "Sellmeier1"

# (attribute, group, model, parameters, desc, long_desc), alphabetical inside each group (the order of the lists)
_TABLE = [
    # ---- glasses: SCHOTT catalogue; fused silica after Malitson 1965
    ("BAF10", "glasses", _S1, dict(coeff=[1.5851495, 0.00926681282, 0.143559385, 0.0424489805, 1.08521269, 105.613573]),
     "BAF10", "N_BAF10 (SCHOTT)"),
    ("BAK1", "glasses", _S1, dict(coeff=[1.12365662, 0.00644742752, 0.309276848, 0.0222284402, 0.881511957, 107.297751]),
     "BAK1", "N-BAK1 (SCHOTT)"),
    ("BASF64", "glasses", _S1, dict(coeff=[1.65554268, 0.0104485644, 0.17131977, 0.0499394756, 1.33664448, 118.961472]),
     "BASF64", "N-BASF64 (SCHOTT)"),
    ("BK7", "glasses", _S1, dict(coeff=[1.03961212, 0.00600069867, 0.231792344, 0.0200179144, 1.01046945, 103.560653]),
     "BK7", "N-BK7 (SCHOTT)"),
    ("F2", "glasses", _S1, dict(coeff=[1.39757037, 0.00995906143, 0.159201403, 0.0546931752, 1.2686543, 119.248346]),
     "F2", "N-F2 (SCHOTT)"),
    ("FK51A", "glasses", _S1, dict(coeff=[0.971247817, 0.00472301995, 0.216901417, 0.0153575612, 0.904651666, 168.68133]),
     "FK51A", "N-FK51A (SCHOTT)"),
    ("fused_silica", "glasses", _S1,
     dict(coeff=_resonances((0.6961663, 0.0684043), (0.4079426, 0.1162414), (0.8974794, 9.896161))),
     "Fused_Silica", "Fused silica (fused quartz)"),
    ("K5", "glasses", _S1, dict(coeff=[1.08511833, 0.00661099503, 0.199562005, 0.024110866, 0.930511663, 111.982777]),
     "K5", "N-K5 (SCHOTT)"),
    ("LAF2", "glasses", _S1, dict(coeff=[1.80984227, 0.0101711622, 0.15729555, 0.0442431765, 1.0930037, 100.687748]),
     "LAF2", "N-LAF2 (SCHOTT)"),
    ("LAK8", "glasses", _S1, dict(coeff=[1.33183167, 0.00620023871, 0.546623206, 0.0216465439, 1.19084015, 82.5827736]),
     "LAK8", "N-LAK8 (SCHOTT)"),
    ("LAK22", "glasses", _S1, dict(coeff=[1.14229781, 0.00585778594, 0.535138441, 0.0198546147, 1.04088385, 100.834017]),
     "LAK22", "N-LAK22 (SCHOTT)"),
    ("LASF9", "glasses", _S1, dict(coeff=[2.00029547, 0.0121426017, 0.298926886, 0.0538736236, 1.80691843, 156.530829]),
     "LASF9", "N-LASF9 (SCHOTT)"),
    ("LASF44", "glasses", _S1, dict(coeff=[1.78897105, 0.00872506277, 0.38675867, 0.0308085023, 1.30506243, 92.7743824]),
     "LASF44", "N-LASF44 (SCHOTT)"),
    ("LF5", "glasses", _S1, dict(coeff=[1.28035628, 0.00929854416, 0.163505973, 0.0449135769, 0.893930112, 110.493685]),
     "LF5", "N-LF5 (SCHOTT)"),
    ("SF5", "glasses", _S1, dict(coeff=[1.52481889, 0.011254756, 0.187085527, 0.0588995392, 1.42729015, 129.141675]),
     "SF5", "N-SF5 (SCHOTT)"),
    ("SF6", "glasses", _S1, dict(coeff=[1.72448482, 0.0134871947, 0.390104889, 0.0569318095, 1.04572858, 118.557185]),
     "SF6", "N-SF6 (SCHOTT)"),
    ("SF10", "glasses", _S1, dict(coeff=[1.62153902, 0.0122241457, 0.256287842, 0.0595736775, 1.64447552, 147.468793]),
     "SF10", "N-SF10 (SCHOTT)"),
    ("SF11", "glasses", _S1, dict(coeff=[1.73759695, 0.013188707, 0.313747346, 0.0623068142, 1.89878101, 155.23629]),
     "SF11", "N-SF11 (SCHOTT)"),
    ("SF66", "glasses", _S1, dict(coeff=[2.0245976, 0.0147053225, 0.470187196, 0.0692998276, 2.59970433, 161.817601]),
     "SF66", "N-SF66 (SCHOTT)"),
    ("SK14", "glasses", _S1, dict(coeff=[0.936155374, 0.00461716525, 0.594052018, 0.016885927, 1.04374583, 103.736265]),
     "SK14", "N-SK14 (SCHOTT)"),
    ("soda_lime", "glasses", "Function", dict(func=_soda_lime), "Soda Lime", "Clear soda lime silica window glass"),
    ("SSK8", "glasses", _S1, dict(coeff=[1.44857867, 0.00869310149, 0.117965926, 0.0421566593, 1.06937528, 111.300666]),
     "SSK8", "N-SSK8 (SCHOTT)"),
    # ---- plastics: COC after Khanarian (Topas 5013, 25 degrees C); COP, PC, PS after Sultanova; PDSM after Schneider;
    #      PMMA after Szczurowski; CR39 Conrady fit of the ZEMAX ophthalmic catalogue; PEI, PET, PVC after Zhang (tables)
    ("COC", "plastics", "Sellmeier2", dict(coeff=[1.045, 0.266, 0.206, 0, 0]), "COC", "Topas COC 5013 at 25°C"),
    ("COP", "plastics", _S1, dict(coeff=[1.2969, 0.011721, 0, 0, 0, 0]), "COP", "COP (Zeonex E48R)"),
    ("CR39", "plastics", "Conrady", dict(coeff=[1.471862713E+000, 1.520790642E-002, 3.555509148E-005]),
     "CR39", "CR-39, PADC, Poly(allyl diglycol carbonate)"),
    ("Finalite", "plastics", "Abbe", dict(n=1.600, V=42), "Finalite", "Sola Finalite"),
    ("MR7", "plastics", "Abbe", dict(n=1.660, V=32), "MR-7", "MR-7"),
    ("Ormex", "plastics", "Abbe", dict(n=1.558, V=32), "Ormex", "Essilor Ormex"),
    ("PC", "plastics", _S1, dict(coeff=[1.4182, 0.021304, 0, 0, 0, 0]), "PC", "Polycarbonate"),
    ("PDSM", "plastics", _S1, dict(coeff=[1.0057, 0.013217, 0, 0, 0, 0]), "PDSM", "Polydimethylsiloxane"),
    ("PEI", "plastics", "Data", dict(wls=_TABLE_WLS, vals=_PEI), "PEI", "Polyetherimide"),
    ("PET", "plastics", "Data", dict(wls=_TABLE_WLS, vals=_PET), "PET", "Polyethylene terephthalate"),
    ("PMMA", "plastics", _S1, dict(coeff=[0.99654, 0.00787, 0.18964, 0.02191, 0.00411, 3.85727]),
     "PMMA", "Poly(methyl methacrylate)"),
    ("PS", "plastics", _S1, dict(coeff=[1.4435, 0.020216, 0, 0, 0, 0]), "PS", "Polystyren"),
    ("PVC", "plastics", "Data", dict(wls=_TABLE_WLS, vals=_PVC), "PVC", "Polyvinyl chloride"),
    ("Spectralite", "plastics", "Abbe", dict(n=1.537, V=47), "Spectralite", "Sola Spectralite"),
    # ---- other media: air after Ciddor (550 nm, no dispersion); BaF2, CaF2 after Malitson; diamond after Peter;
    #      ethanol after Sani; ice from the crystals table; MgF2 after Dodge (ordinary ray); water after Daimon, 20 degrees C
    ("air", "misc", "Constant", dict(n=1.00027784), "Air", "Air at 550nm, 15°C, 1013.25hPa"),
    ("BaF2", "misc", _S1, dict(coeff=_resonances((0.643356, 0.057789), (0.506762, 0.10968), (3.8261, 46.3864))),
     "BaF2", "BaF2 (Barium fluoride)"),
    ("CaF2", "misc", _S1, dict(coeff=_resonances((0.5675888, 0.050263605), (0.4710914, 0.1003909), (3.8484723, 34.649040))),
     "CaF2", "CaF2 (Calcium fluoride)"),
    ("diamond", "misc", _S1, dict(coeff=[*_resonances((0.3306, 0.1750), (4.3356, 0.1060)), 0, 0]), "Diamond", "Diamond"),
    ("ethanol", "misc", _S1, dict(coeff=[0.0165, 9.08, 0.8268, 0.01039, 0, 0]), "Ethanol", "C2H5OH (Ethanol)"),
    ("ice", "misc", "Data", dict(wls=_TABLE_WLS, vals=_ICE), "Ice", "Water Ice at -7°C"),
    ("MgF2", "misc", _S1, dict(coeff=_resonances((0.48755108, 0.04338408), (0.39875031, 0.09461442), (2.3120353, 23.793604))),
     "MgF2", "MgF2 (Magnesium fluoride)"),
    ("vacuum", "misc", "Constant", dict(n=1.0), "Vacuum", "Vacuum"),
    ("water", "misc", "Sellmeier3",
     dict(coeff=[5.684027565E-1, 5.101829712E-3, 1.726177391E-1, 1.821153936E-2, 2.086189578E-2, 2.620722293E-2,
                 1.130748688E-1, 1.069792721E1]), "Water", "Water at 20.0°C"),
]

glasses: list = []
plastics: list = []
misc: list = []

for _name, _group, _model, _params, _desc, _long_desc in _TABLE:
    _medium = RefractionIndex(_model, desc=_desc, long_desc=_long_desc, **_params)
    globals()[_name] = _medium
    globals()[_group].append(_medium)

#: every refractive index preset
all_presets: list = [*glasses, *plastics, *misc]
