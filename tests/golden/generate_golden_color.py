#!/usr/bin/env python3
"""tests/golden/color.npz: what the reference's color module and the colour figures of its spectrum classes give for the
inputs of tests/image_convert_cases.py and tests/color_cases.py.

Runs only where the reference is installed (imported through oracle/refload.py); the .npz is committed, the reference is
not.  Re-run with
    python tests/golden/generate_golden_color.py [output.npz]
The archive is written with fixed zip time stamps, so a second run reproduces the file byte for byte.

Keys
  const/<NAME>                       the module's constants
  <case>/xyz                         the input (the XYZ planes of image_convert_cases()[case])
  <case>/<key>                       the reference's result; chained functions take the recorded array as their input:
                                     xyY_to_xyz <- xyz_to_xyY; luv_* <- xyz_to_luv; get_chroma_scale <- xyz_to_luv|nonorm;
                                     srgb_to_xyz, log_srgb|Absolute <- xyz_to_srgb; log_srgb|Perceptual <- xyz_to_srgb|Perceptual;
                                     srgb_linear_to_xyz <- xyz_to_srgb_linear|Absolute
  <case>/<key>/keep                  False for pixels the reference cannot decide (below); the tests compare the rest
  <case>/get_chroma_scale|Lth<v>     the factor; <case>/get_chroma_scale|full the per-pixel factors
  log_extra/<name>/in, /out          the two early returns of log_srgb
  colormap/<name>/wl, /rgba          spectral_colormap
  observers/wl, /x, /y, /z;  xyz_from_spectrum/wl, /spec, /sum, /trapz
  wavelengths/<set>/xyz, /dominant, /complementary      sets: the lit pixels of `spectral`, the hue ring
  light/<name>/xyz, /dominant, /complementary, /color|<args>;  transmission/<name>/xyz, /color|<args>

Pixels the reference cannot decide: the method of generate_golden_image_convert.py, applied to each function's own input.
Every non-zero input component is moved by one ulp (14 sign patterns) and the function is evaluated again; a pixel whose
result moves by more than 1e-10 of the output's maximum is dropped here -- never in a test.  At most 1 % of a case's lit
pixels may go that way per output.  The chroma factors (image-wide scalars) must not move when the XYZ image they stem from is
perturbed.  (The Luv array itself is not perturbed for them: `degenerate` has pixels with X = Z = 0, whose u' is an exact zero
that `u' > 0` decides the same way on both sides, as in image_convert.npz; one ulp on u would turn it into noise.)
"""
from __future__ import annotations

import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(HERE))
from generate_golden_image_convert import ot, color, perturbed, SIGNS, SENS, write_npz  # noqa: E402  (loads the reference)
import color_cases as cc  # noqa: E402

CONSTANTS = ["WP_D65_XY", "WP_D65_XYZ", "WP_D65_LUV", "WP_D65_UV", "SRGB_R_XY", "SRGB_G_XY", "SRGB_B_XY", "SRGB_R_UV",
             "SRGB_G_UV", "SRGB_B_UV", "SRGB_PRIMARY_POWER_FACTORS"]


def movement(key: str, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """(Ny, Nx): how far a pixel's result moved, as a share of the output's maximum (inf where a NaN came or went)."""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    d = np.abs(a - b)
    if key == "luv_hue":
        d = np.minimum(d, 360 - d)
        scale = 360.0
    else:
        scale = np.nanmax(np.abs(a)) if np.any(np.isfinite(a)) else 0.0
    d = d / scale if scale else np.where(d > 0, np.inf, 0.0)
    d = np.where(np.isnan(a) != np.isnan(b), np.inf, np.where(np.isnan(a), 0.0, d))
    return d if d.ndim == 2 else d.max(axis=2)


def record(out: dict, case: str, key: str, fn, inp: np.ndarray, lit: int) -> np.ndarray:
    """Evaluate fn(inp), find the pixels it cannot decide, store both; -> the result."""
    with np.errstate(all="ignore"):
        before = inp.copy()
        res = np.asarray(fn(inp))
        assert np.array_equal(before, inp, equal_nan=True), f"{key} modifies its input"
        worst = np.zeros(inp.shape[:2])
        for signs in SIGNS:
            worst = np.maximum(worst, movement(key, res, fn(perturbed(inp, signs))))
    keep = worst <= SENS
    dropped = int(np.count_nonzero(~keep))
    assert dropped <= 0.01 * lit, f"{case} {key}: {dropped} of {lit} lit pixels undecidable"
    assert not np.any(np.isnan(np.asarray(res, dtype=np.float64))), f"{case} {key}: NaN"
    out[f"{case}/{key}"] = res
    out[f"{case}/{key}/keep"] = keep
    return res


def image_cases(out: dict) -> None:
    for case, xyz in cc.xyz_cases().items():
        lit = int(np.count_nonzero(np.any(xyz != 0, axis=2)))
        rec = lambda key, fn, inp: record(out, case, key, fn, inp, lit)  # noqa: E731
        out[f"{case}/xyz"] = xyz
        xyY = rec("xyz_to_xyY", color.xyz_to_xyY, xyz)
        rec("xyY_to_xyz", color.xyY_to_xyz, xyY)
        luv = rec("xyz_to_luv", color.xyz_to_luv, xyz)
        luv1 = rec("xyz_to_luv|nonorm", lambda a: color.xyz_to_luv(a, normalize=False), xyz)
        for name in ("luv_to_xyz", "luv_to_u_v_l", "luv_hue", "luv_chroma", "luv_saturation"):
            rec(name, getattr(color, name), luv)
        for key, kw in cc.linear_keys():
            rec(key, lambda a, kw=kw: color.xyz_to_srgb_linear(a, **kw), xyz)
        srgb = rec("xyz_to_srgb", color.xyz_to_srgb, xyz)
        srgb_p = rec("xyz_to_srgb|Perceptual", lambda a: color.xyz_to_srgb(a, rendering_intent="Perceptual"), xyz)
        rec("srgb_to_xyz", color.srgb_to_xyz, srgb)
        rec("srgb_linear_to_xyz", color.srgb_linear_to_xyz, out[f"{case}/xyz_to_srgb_linear|Absolute"])
        rec("outside_srgb_gamut", color.outside_srgb_gamut, xyz)
        rec("log_srgb|Absolute", color.log_srgb, srgb)
        rec("log_srgb|Perceptual", color.log_srgb, srgb_p)
        # the chroma factor: a scalar per L_th that must not move, and the per-pixel factors
        clipped = xyz.clip(0)
        for L_th in cc.L_THS:
            fact = color.get_chroma_scale(color.xyz_to_luv(clipped, normalize=False), L_th)
            assert fact == color.get_chroma_scale(luv1, L_th)
            for signs in SIGNS:
                moved = color.get_chroma_scale(color.xyz_to_luv(perturbed(clipped, signs), normalize=False), L_th)
                assert abs(moved - fact) <= SENS * fact, f"{case}: chroma factor at L_th={L_th} moves: {fact!r} -> {moved!r}"
            out[f"{case}/get_chroma_scale|Lth{L_th:g}"] = np.float64(fact)
        rec("get_chroma_scale|full", lambda a: color.get_chroma_scale(a, 0.0, return_full=True)[1], luv1)
        print(case, xyz.shape[:2], "lit", lit, "dropped",
              {k.split("/")[1]: int(np.count_nonzero(~v)) for k, v in out.items() if k.startswith(case + "/") and k.endswith("/keep") and not v.all()})


def tables_and_figures(out: dict) -> None:
    for name in CONSTANTS:
        out[f"const/{name}"] = np.array(getattr(color, name), dtype=np.float64)
    out["const/SRGB_RENDERING_INTENTS"] = np.array(color.SRGB_RENDERING_INTENTS)

    for name, img in cc.log_extra_images().items():
        res = color.log_srgb(img)
        assert res is not img and np.array_equal(res, img), f"log_srgb {name}: not the early return"
        out[f"log_extra/{name}/in"], out[f"log_extra/{name}/out"] = img, res

    for name, wl in cc.colormap_wavelengths().items():
        res = color.spectral_colormap(wl)
        for s in (1, -1):  # every wavelength one ulp up, one ulp down
            moved = color.spectral_colormap(np.nextafter(wl, s * np.inf))
            assert np.abs(moved - res).max() <= SENS, f"colormap {name} moves by {np.abs(moved - res).max()}"
        out[f"colormap/{name}/wl"], out[f"colormap/{name}/rgba"] = wl, res

    wl = cc.observer_wavelengths()
    out["observers/wl"] = wl
    for c in "xyz":
        out[f"observers/{c}"] = getattr(color, f"{c}_observer")(wl)
    assert wl.shape == (64,) and np.count_nonzero((wl < 360) | (wl > 830)) >= 2 and 360.0 in wl and 830.0 in wl
    wl, spec = cc.spectrum_samples()
    out["xyz_from_spectrum/wl"], out["xyz_from_spectrum/spec"] = wl, spec
    out["xyz_from_spectrum/sum"] = color.xyz_from_spectrum(wl, spec)
    out["xyz_from_spectrum/trapz"] = color.xyz_from_spectrum(wl, spec, method="trapz")

    spectral = cc.xyz_cases()["spectral"].reshape(-1, 3)
    sets = {"spectral": spectral[np.any(spectral != 0, axis=1)], "ring": cc.hue_ring()}
    for name, xyz in sets.items():
        both = lambda v: np.array([[color.dominant_wavelength(p), color.complementary_wavelength(p)] for p in v])  # noqa: E731
        res = both(xyz)
        for signs in SIGNS:
            moved = both(perturbed(xyz[None], signs)[0])
            assert np.array_equal(np.isnan(moved), np.isnan(res)), f"wavelengths {name}: a NaN comes or goes"
            # the tests allow rtol 1e-9, about 5e-7 nm: one ulp of the input has to stay well below that
            assert np.nanmax(np.abs(moved - res)) < 1e-7, f"wavelengths {name} move by {np.nanmax(np.abs(moved - res))} nm"
        out[f"wavelengths/{name}/xyz"] = xyz
        out[f"wavelengths/{name}/dominant"], out[f"wavelengths/{name}/complementary"] = res[:, 0], res[:, 1]
        print("wavelengths", name, xyz.shape[0], "NaN", np.isnan(res).sum(axis=0))
    ring = out["wavelengths/ring/dominant"], out["wavelengths/ring/complementary"]
    assert all(np.isnan(r).any() and np.isfinite(r).any() for r in ring)

    for name, spec in cc.light_spectra(ot).items():
        out[f"light/{name}/xyz"] = spec.xyz()
        if name not in cc.NO_WAVELENGTHS:
            out[f"light/{name}/dominant"] = np.float64(spec.dominant_wavelength())
            out[f"light/{name}/complementary"] = np.float64(spec.complementary_wavelength())
        for tag, kw in cc.LIGHT_COLOR_ARGS.items():
            out[f"light/{name}/color|{tag}"] = np.array(spec.color(**kw), dtype=np.float64)
        print("light", name, out[f"light/{name}/xyz"], out.get(f"light/{name}/dominant"), out.get(f"light/{name}/complementary"))
    for name, spec in cc.transmission_spectra(ot).items():
        out[f"transmission/{name}/xyz"] = spec.xyz()
        for tag, kw in cc.TRANSMISSION_COLOR_ARGS.items():
            out[f"transmission/{name}/color|{tag}"] = np.array(spec.color(**kw), dtype=np.float64)
        print("transmission", name, out[f"transmission/{name}/color|default"])


def main(path) -> None:
    out = {}
    image_cases(out)
    tables_and_figures(out)
    assert sum(v.shape[0] * v.shape[1] for k, v in out.items() if k.endswith("/xyz") and v.ndim == 3) <= 1500
    write_npz(path, out)
    size = pathlib.Path(path).stat().st_size
    print(path, len(out), "arrays,", size, "bytes")
    assert size < 1_000_000


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE / "color.npz")
