#!/usr/bin/env python3
"""Golden values for the preset catalogue, from the upstream NumPy reference.  Like generate_golden.py this runs only where
the reference is installed; the fixtures are committed, the reference is not.
    python tests/golden/generate_golden_presets.py

presets.npz
  wl                                   scenes_presets.WL, 81 wavelengths
  media/names, media/list/<list>       attribute names of all media and of the lists' members, in list order
  media/n, /abbe, /type, /desc, /long_desc     per medium, in the order of media/names
  media/n_lines                        n at spectral_lines.all_lines: wavelengths that are no float32 numbers
  light/..., spectrum/...              the same for light spectra and observer curves: names, lists, type, desc, long_desc,
                                       values (NaN rows for line spectra), <name>/lines and /line_vals for those
  light/power_factors                  the three sRGB power factors
  spectrum/quantity, /unit             of the observer curves
  lines/<list>                         spectral line lists;  lines/combinations: names of all_line_combinations's members
  geometry/list/<list>                 function names;  geometry/<case>/...: scenes_presets.group_state
  psf/<case>/...                       scenes_presets.psf_record
  raises/names, raises/raised          scenes_presets.argument_cases and the class name raised, or "none"
  convolve/<psf>/...                   sparse image convolved with the preset PSF: shape, extent, every 4th row and column, sum
trace_legrand_eye.npz, trace_presets_achromat.npz     as generate_golden.gen_trace writes them
"""
from __future__ import annotations

import numpy as np

import generate_golden as gg  # (imports the reference, tests/scenes.py and the oracle loader)

import scenes_presets as sp

ot = gg.ot
HERE = gg.HERE


def _strings(values) -> np.ndarray:
    return np.array([str(v) for v in values])


def gen_media(out: dict) -> None:
    mod = ot.presets.refraction_index
    media = mod.all_presets
    out["media/names"] = _strings(sp.names_of(mod, media))
    for name in sp.MEDIA_LISTS:
        out[f"media/list/{name}"] = _strings(sp.names_of(mod, getattr(mod, name)))
    out["media/n"] = np.array([m(sp.WL) for m in media], dtype=np.float64)
    out["media/abbe"] = np.array([m.abbe_number() for m in media], dtype=np.float64)
    out["media/n_lines"] = np.array([m(np.array(ot.presets.spectral_lines.all_lines)) for m in media], dtype=np.float64)
    out["media/type"] = _strings(m.spectrum_type for m in media)
    out["media/desc"], out["media/long_desc"] = _strings(m.desc for m in media), _strings(m.long_desc for m in media)
    types, counts = np.unique(out["media/type"], return_counts=True)
    print("media:", len(media), dict(zip(types, counts)))


def gen_spectra(out: dict, prefix: str, mod, lists: tuple) -> None:
    members = mod.all_presets
    names = sp.names_of(mod, members)
    out[f"{prefix}/names"] = _strings(names)
    for name in lists:
        out[f"{prefix}/list/{name}"] = _strings(sp.names_of(mod, getattr(mod, name)))
    out[f"{prefix}/type"] = _strings(s.spectrum_type for s in members)
    out[f"{prefix}/desc"], out[f"{prefix}/long_desc"] = _strings(s.desc for s in members), _strings(s.long_desc for s in members)
    out[f"{prefix}/quantity"], out[f"{prefix}/unit"] = _strings(s.quantity for s in members), _strings(s.unit for s in members)
    values = np.full((len(members), len(sp.WL)), np.nan)
    for j, (name, s) in enumerate(zip(names, members)):
        if s.is_continuous():
            values[j] = s(sp.WL)
        else:
            out[f"{prefix}/{name}/lines"] = np.array(s.lines, dtype=np.float64)
            out[f"{prefix}/{name}/line_vals"] = np.array(s.line_vals, dtype=np.float64)
    out[f"{prefix}/values"] = values
    print(f"{prefix}:", len(members))


def gen_lines(out: dict) -> None:
    mod = ot.presets.spectral_lines
    for name in sp.LINE_LISTS:
        out[f"lines/{name}"] = np.array(getattr(mod, name), dtype=np.float64)
    out["lines/names"] = _strings(sp.names_of(mod, mod.all_lines))
    out["lines/combinations"] = _strings(sp.names_of(mod, mod.all_line_combinations))


def gen_geometry(out: dict) -> None:
    mod = ot.presets.geometry
    for name in sp.GEOMETRY_LISTS:
        out[f"geometry/list/{name}"] = _strings(f.__name__ for f in getattr(mod, name))
    for case in sp.GEOMETRY_ARGS:
        G = sp.geometry(ot, case)
        assert len(G.volumes) == 1 and len(G.elements) == len(G.lenses) + len(G.apertures) + len(G.detectors) + 1
        for k, v in sp.group_state(G).items():
            out[f"geometry/{case}/{k}"] = v
        print(f"geometry {case}:", list(out[f"geometry/{case}/classes"]))


def gen_psfs(out: dict) -> None:
    for case in sp.PSF_ARGS:
        img = sp.psf(ot, case)
        assert type(img) is ot.GrayscaleImage
        for k, v in sp.psf_record(img).items():
            out[f"psf/{case}/{k}"] = v
        print(f"psf {case}: shape {img.shape}, s {img.s}, sum {img.data.sum():.12g}")


def gen_raises(out: dict) -> None:
    cases = sp.argument_cases(ot)
    out["raises/names"] = _strings(cases)
    out["raises/raised"] = _strings(sp.outcome(c) for c in cases.values())
    for name, raised in zip(out["raises/names"], out["raises/raised"]):
        print(f"  raises/{name}: {raised}")


def gen_convolve(out: dict) -> None:
    """The refload stand-in for cv2.resize raises for anything but the identity, so a pitch mismatch cannot pass silently."""
    for case in sp.CONVOLVE_CASES:
        psf = sp.psf(ot, case)
        img = sp.sparse_image(ot, psf)
        res = ot.convolve(img, psf)
        d = res.data
        out[f"convolve/{case}/shape"], out[f"convolve/{case}/extent"] = np.array(d.shape), np.array(res.extent)
        out[f"convolve/{case}/grid4"] = d[::4, ::4].astype(np.float64)
        out[f"convolve/{case}/sum"] = d.sum()
        print(f"convolve {case}: shape {d.shape}, sum {d.sum():.12g}, max {d.max():.6g}")


if __name__ == "__main__":
    out = {"wl": sp.WL}
    gen_media(out)
    gen_spectra(out, "light", ot.presets.light_spectrum, sp.LIGHT_LISTS)
    out["light/power_factors"] = np.array([getattr(ot.presets.light_spectrum, k) for k in sp.POWER_FACTORS])
    gen_spectra(out, "spectrum", ot.presets.spectrum, sp.SPECTRUM_LISTS)
    gen_lines(out)
    gen_geometry(out)
    gen_psfs(out)
    gen_raises(out)
    gen_convolve(out)
    np.savez_compressed(HERE / "presets.npz", **out)
    print("presets.npz", len(out))
    for j, (name, (builder, N)) in enumerate(sp.SCENES.items()):
        gg.gen_trace(name, builder, N, seed=1400 + j)
