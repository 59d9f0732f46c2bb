#!/usr/bin/env python3
"""tests/golden/image_convert.npz: what the reference's colour functions give for the synthetic XYZW images of
tests/image_convert_cases.py, for every entry of RenderImage.image_modes and every variant convolve() can request.

Runs only where the reference is installed (imported through oracle/refload.py); the .npz is committed, the reference
is not.  Re-run with
    python tests/golden/generate_golden_image_convert.py [output.npz]
The archive is written with fixed zip time stamps, so a second run reproduces the file byte for byte.

Every value is computed by the functions RenderImage.get calls (render_image.py:178-219), in its order, on the array
itself: color.xyz_to_srgb, color.outside_srgb_gamut, color.xyz_to_luv with luv_hue / luv_chroma / luv_saturation.
Nothing is resized.

Keys
  <case>/xyzw                        the input (equal to what image_convert_cases() builds)
  <case>/<mode><variant>             the reference's result, all pixels (NaN where the reference gives NaN)
  <case>/keep                        False for pixels the reference cannot decide (see below); the tests compare the rest
  coverage/<case>/...                pixel counts per branch, taken from the reference's own results
  scalars/<case>/...                 the image-wide quantities: chroma factor before and after its clamp, flags

Pixels the reference cannot decide.  Every non-zero input component is moved by one ulp up or down (14 sign patterns:
each component alone, and all eight combinations) and everything is evaluated again.  A pixel whose result, in any
output, moves by more than 1e-10 of that output's maximum sits on a sector boundary of the gamut triangle or has a
chroma of rounding-noise size: there the reference's own answer is noise, and the pixel is dropped here -- never in a
test.  At most 1 % of a case's lit pixels may go that way; more than that means the inputs have to move.  Exact zeros
stay exact zeros: both sides see the same zero, and `Y > 0` decides the same way for both.
The image-wide quantities must not move under the same perturbations (flags equal, factors within 1e-10), and no pixel
may lie within 1e-10 of the lightness threshold L_th * max(L) for 0 < L_th < 1.  (L_th = 1 compares the maximum with
itself, which no rounding can turn true; L_th = 0 compares with an exact zero.)
"""
from __future__ import annotations

import io
import pathlib
import sys
import zipfile

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))

import refload  # noqa: E402
from image_convert_cases import (image_convert_cases, srgb_keys, PERCEPTUAL_VARIANTS, SCALAR_MODES, APX, K)  # noqa: E402

ot = refload.load(0)
color = ot.color
import optrace.tracer.color.srgb as rsrgb  # noqa: E402  (the chroma helpers behind color.xyz_to_srgb)

SENS = 1e-10
E_LUV = 0.008856
KNEE_SRGB = 12.92 * 0.0031308


def reference_outputs(xyzw: np.ndarray) -> dict:
    img = xyzw.copy()
    xyz = img[:, :, :3]
    out = {}
    with np.errstate(all="ignore"):
        for key, _, kw in srgb_keys():
            out[key] = color.xyz_to_srgb(xyz, **kw)
        out["Outside sRGB Gamut"] = np.array(color.outside_srgb_gamut(xyz), dtype=np.float64)
        out["Irradiance"] = 1 / APX * img[:, :, 3]
        out["Illuminance"] = K / APX * img[:, :, 1]
        out["Lightness (CIELUV)"] = color.xyz_to_luv(xyz)[:, :, 0]
        out["Hue (CIELUV)"] = color.luv_hue(color.xyz_to_luv(xyz))
        out["Chroma (CIELUV)"] = color.luv_chroma(color.xyz_to_luv(xyz))
        out["Saturation (CIELUV)"] = color.luv_saturation(color.xyz_to_luv(xyz))
    assert {k.split("|")[0] for k in out} == set(ot.RenderImage.image_modes)
    return out


def reference_scalars(xyzw: np.ndarray) -> dict:
    """The image-wide quantities behind the results, from the reference's own functions."""
    xyz = xyzw[:, :, :3]
    sc = {}
    with np.errstate(all="ignore"):
        rgbl = color.xyz_to_srgb_linear(xyz, normalize=False, rendering_intent="Ignore")
        sc["any_inv"] = float(np.any(rgbl < 0))
        sc["rgbmax"] = float(np.nanmax(rgbl))
        luv = color.xyz_to_luv(xyz.clip(0), normalize=False)
        valid, cr2 = rsrgb._get_chroma_scale(luv)
        sc["any_valid"] = float(np.any(valid))
        sc["Lmax"] = float(luv[:, :, 0].max())
        for tag, kw in PERCEPTUAL_VARIANTS.items():
            if "chroma_scale" in kw:
                continue
            L_th = kw.get("L_th", 0.0)
            sel = cr2[valid & (luv[:, :, 0] > L_th * luv[:, :, 0].max())]
            sc[f"raw{tag}"] = float(np.sqrt(sel.min())) if sel.size else np.nan  # NaN: the empty set
            sc[f"fact{tag}"] = color.get_chroma_scale(luv, L_th)
            if 0 < L_th < 1 and sc["Lmax"] > 0:
                gap = np.abs(luv[:, :, 0] - L_th * sc["Lmax"])[valid]
                assert not np.any(gap <= SENS * sc["Lmax"]), "a pixel sits on the lightness threshold"
    return sc


def perturbed(xyzw: np.ndarray, signs) -> np.ndarray:
    p = xyzw.copy()
    for c, s in enumerate(signs):
        if s:
            v = p[:, :, c]
            p[:, :, c] = np.where(v != 0, np.nextafter(v, s * np.inf), v)
    return p


SIGNS = [tuple(s if i == c else 0 for i in range(3)) for c in range(3) for s in (1, -1)] + \
        [(a, b, c) for a in (1, -1) for b in (1, -1) for c in (1, -1)]


def movement(key: str, a: np.ndarray, b: np.ndarray) -> np.ndarray:
    """(Ny, Nx): how far a pixel's result moved, as a share of the output's maximum (inf where a NaN came or went)."""
    d = np.abs(a - b)
    if key.startswith("Hue"):
        d = np.minimum(d, 360 - d)
        scale = 360.0
    else:
        scale = np.nanmax(np.abs(a)) if np.any(np.isfinite(a)) else 0.0
    d = d / scale if scale else np.where(d > 0, np.inf, 0.0)
    d = np.where(np.isnan(a) != np.isnan(b), np.inf, np.where(np.isnan(a), 0.0, d))
    return d if d.ndim == 2 else d.max(axis=2)


def edge_of(x, y, r, g, b) -> np.ndarray:
    """Which side of the triangle r, g, b the projected points lie on: 0 blue-green, 1 green-red, 2 blue-red."""
    def dist(p, q):
        return np.abs((q[0] - p[0]) * (y - p[1]) - (q[1] - p[1]) * (x - p[0])) / np.hypot(q[0] - p[0], q[1] - p[1])
    return np.argmin(np.stack([dist(b, g), dist(g, r), dist(b, r)]), axis=0)


def coverage(xyzw: np.ndarray, outs: dict, keep: np.ndarray) -> dict:
    """Branch counts over the kept pixels, read off the reference's own results."""
    xyz = xyzw[:, :, :3]
    cov = {}
    with np.errstate(all="ignore"):
        # xy triangle: the out-of-gamut pixels of the Absolute intent (srgb.py:321-327), projected by the reference
        rgbl = color.xyz_to_srgb_linear(xyz, normalize=False, rendering_intent="Ignore")
        inv = np.any(rgbl < 0, axis=2) & keep
        xyY = color.xyz_to_xyY(np.array([xyz[inv]]))
        x, y = xyY[:, :, 0].copy(), xyY[:, :, 1].copy()
        rsrgb._triangle_intersect(color.SRGB_R_XY, color.SRGB_G_XY, color.SRGB_B_XY, color.WP_D65_XY, x, y)
        e = edge_of(x, y, color.SRGB_R_XY, color.SRGB_G_XY, color.SRGB_B_XY)
        for i, name in enumerate(("bg", "gr", "br")):
            cov[f"xy_{name}"] = int(np.count_nonzero(e == i))
        # u'v' triangle: every lit pixel of the Perceptual intent (srgb.py:204-231)
        luv = color.xyz_to_luv(xyz.clip(0), normalize=False)
        lit = (luv[:, :, 0] > 0) & keep
        uvl = color.luv_to_u_v_l(luv)
        u, v = uvl[:, :, 0].copy(), uvl[:, :, 1].copy()
        rsrgb._triangle_intersect(color.SRGB_R_UV, color.SRGB_G_UV, color.SRGB_B_UV, color.WP_D65_UV, u, v)
        e = edge_of(u, v, color.SRGB_R_UV, color.SRGB_G_UV, color.SRGB_B_UV)
        for i, name in enumerate(("bg", "gr", "br")):
            cov[f"uv_{name}"] = int(np.count_nonzero((e == i) & lit))
    Y, L = xyz[:, :, 1], luv[:, :, 0]
    cov["t_above"] = int(np.count_nonzero((Y > E_LUV) & keep))          # xyz_to_luv with Yn = 1: t = Y
    cov["t_below"] = int(np.count_nonzero((Y > 0) & (Y <= E_LUV) & keep))
    cov["L_above"] = int(np.count_nonzero((L > 903.3 * E_LUV) & keep))  # luv_to_xyz
    cov["L_below"] = int(np.count_nonzero((L > 0) & (L <= 903.3 * E_LUV) & keep))
    rgb = outs["sRGB (Absolute RI)"]
    cov["gamma_above"] = int(np.count_nonzero(np.any(rgb > KNEE_SRGB, axis=2) & keep))
    cov["gamma_below"] = int(np.count_nonzero(np.any((rgb > 0) & (rgb <= KNEE_SRGB), axis=2) & keep))
    # the odd arm of the gamma curve, sg * (...) for values below the negative knee: only clip=False lets them through
    cov["gamma_negative"] = max(int(np.count_nonzero(np.any(val < -KNEE_SRGB, axis=2) & keep))
                                for key, val in outs.items() if "noclip" in key)
    cov["lit"] =int(np.count_nonzero(np.any(xyz != 0, axis=2)))
    cov["dropped"] = int(np.count_nonzero(~keep))
    return cov


def write_npz(path, arrays: dict) -> None:
    """np.savez_compressed with fixed time stamps: the same arrays give the same bytes."""
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as zf:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            zf.writestr(info, buf.getvalue())


def main(path) -> None:
    out = {}
    for name, xyzw in image_convert_cases().items():
        outs, sc = reference_outputs(xyzw), reference_scalars(xyzw)
        worst = np.zeros(xyzw.shape[:2])
        for signs in SIGNS:
            p = perturbed(xyzw, signs)
            for key, val in reference_outputs(p).items():
                worst = np.maximum(worst, movement(key, outs[key], val))
            for k, v in reference_scalars(p).items():
                same = (np.isnan(v) and np.isnan(sc[k])) or abs(v - sc[k]) <= SENS * abs(sc[k])
                assert same, f"{name}: image-wide quantity {k} moves under a one-ulp perturbation: {sc[k]!r} -> {v!r}"
        keep = worst <= SENS
        cov = coverage(xyzw, outs, keep)
        assert cov["dropped"] <= 0.01 * cov["lit"], f"{name}: {cov['dropped']} of {cov['lit']} lit pixels undecidable"
        out[f"{name}/xyzw"] = xyzw
        out[f"{name}/keep"] = keep
        for key, val in outs.items():
            out[f"{name}/{key}"] = val
        for k, v in cov.items():
            out[f"coverage/{name}/{k}"] = np.int64(v)
        for k, v in sc.items():
            out[f"scalars/{name}/{k}"] = np.float64(v)
        print(name, xyzw.shape[:2], "coverage", cov)
        print("   scalars", {k: round(v, 6) for k, v in sc.items()})
        nan = sorted(k for k, v in outs.items() if np.any(np.isnan(v)))
        if nan:
            print("   NaN in", nan)

    # the conditions the suite rests on (tests/test_image_convert_fixture.py checks the recorded numbers again)
    cov = {k.split("/")[-1]: int(v) for k, v in out.items() if k.startswith("coverage/spectral/")}
    for k in ("xy_bg", "xy_gr", "xy_br", "uv_bg", "uv_gr", "uv_br", "t_above", "t_below", "L_above", "L_below",
              "gamma_above", "gamma_below"):
        assert cov[k] >= 20, (k, cov[k])
    assert 0.32 < out["scalars/spectral/raw"] < 1 and out["scalars/spectral/fact"] == out["scalars/spectral/raw"]
    assert 0.32 < out["scalars/px1_spectral/raw"] < 1 and out["scalars/px1_spectral/fact"] == out["scalars/px1_spectral/raw"]
    d = {t: (float(out[f"scalars/dim_outlier/raw{t}"]), float(out[f"scalars/dim_outlier/fact{t}"])) for t in ("", "|Lth0.05", "|Lth1")}
    assert d[""][0] < 0.32 and d[""][1] == 0.32 and d["|Lth0.05"][0] >= 1 and d["|Lth0.05"][1] == 1 \
        and np.isnan(d["|Lth1"][0]) and d["|Lth1"][1] == 1, d
    assert out["scalars/invalid_only/any_valid"] == 0 and not np.any(out["invalid_only/xyzw"][:, :, 1] <= 0)
    assert out["coverage/invalid_only/gamma_negative"] >= 10  # most of its 15 pixels, in one clip=False output
    # the picture of the convolve() test: each colour argument changes its result
    w = [out[f"wide_gamut/sRGB (Absolute RI){t}"] for t in ("", "|nonorm")] + [out[f"wide_gamut/sRGB (Perceptual RI){t}"] for t in ("", "|Lth0.02")]
    assert all(np.abs(a - b).max() > 1e-3 for i, a in enumerate(w) for b in w[:i])
    assert sum(v.shape[0] * v.shape[1] for k, v in out.items() if k.endswith("/xyzw")) <= 1500
    write_npz(path, out)
    print(path, len(out), "arrays,", pathlib.Path(path).stat().st_size, "bytes")


if __name__ == "__main__":
    main(sys.argv[1] if len(sys.argv) > 1 else HERE / "image_convert.npz")
