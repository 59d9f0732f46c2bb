#!/usr/bin/env python3
"""tests/golden/wavelength_step.npz: what the reference gives for the cases of tests/outline_cases.py (rays that miss an
element: where they are left, the outline clip, the counters) and of tests/wavelength_cases.py (refractive indices and
filter transmissions value by value, with the exact values of the same formulas).

Runs only where the reference is installed (imported through oracle/refload.py) and mpmath is; the .npz is committed, the
reference is not.  Re-run with
    python tests/golden/generate_golden_wavelength.py [output.npz]
The archive is written with fixed zip time stamps, so a second run reproduces the file byte for byte.

The inputs are not stored: outline_cases.inputs(scene) and wavelength_cases regenerate them, the checksums tie them to the
archive.  Keys:
  outline/<scene>/checksum      outline_cases.checksum of the inputs
  outline/<scene>/p (n, nt - 1, 3) f64    the reference's p_list, sections 1 .. nt - 1 (section 0 is the input)
  outline/<scene>/w (n, nt) f32           its w_list
  outline/<scene>/msgs (5, nt) i64        its counter table (Raytracer.INFOS rows)
The rays enter the reference's own Raytracer.trace through the source's create_rays; nothing of its loop is restated.
The keys of the wavelength part are listed in tests/wavelength_cases.py.
"""
from __future__ import annotations

import pathlib
import sys

import numpy as np

HERE = pathlib.Path(__file__).resolve().parent
ROOT = HERE.parent.parent
sys.path.insert(0, str(ROOT / "oracle"))
sys.path.insert(0, str(ROOT / "tests"))
sys.path.insert(0, str(ROOT))

import refload  # noqa: E402
import outline_cases as oc  # noqa: E402
import wavelength_cases as wc  # noqa: E402

ot = refload.load(0)


def outline_scene(name: str) -> dict:
    inp = oc.inputs(name)
    n = inp["s0"].shape[0]
    RT = oc.raytracer(ot, name)
    src = RT.ray_sources[0]

    def create_rays(N, no_pol=False, power=None):
        assert N == n and not no_pol
        return inp["p0"], inp["s0"], inp["pol0"], inp["w0"], inp["wl"]

    src.create_rays = create_rays
    with np.errstate(all="ignore"):
        RT.trace(n)
    assert not RT.geometry_error
    rays = RT.rays
    assert np.array_equal(rays.p_list[:, 0], inp["p0"]) and np.array_equal(rays.w_list[:, 0], inp["w0"])
    msgs = np.asarray(RT._msgs, dtype=np.int64)
    # the classes do what outline_cases says of them
    e = oc.expected(name, inp)
    sc = oc.scene(name)
    flat = ot.CircularSurface(r=oc.R_EL)
    flat.move_to([sc.centre[0], sc.centre[1], sc.z])
    c, _, _ = flat.find_hit(np.asfortranarray(inp["p0"]), np.asfortranarray(inp["s0"]))
    assert oc.bits(np.ascontiguousarray(c), e["c"]), "flat_hit_point restates the reference's find_hit"
    bad = oc.rule_violations(name, inp, rays.p_list, rays.w_list, msgs, rays.pol_list)
    assert not bad, (name, bad)
    k = f"outline/{name}"
    print(f"{k:18s} {n} rays, counters\n{msgs}", flush=True)
    return {f"{k}/checksum": np.array(oc.checksum(inp)), f"{k}/p": np.ascontiguousarray(rays.p_list[:, 1:]),
            f"{k}/w": np.ascontiguousarray(rays.w_list), f"{k}/msgs": msgs}


def wavelength_part() -> dict:
    import optrace_amd   # the product's host classes: coefficient records and table nodes (no device is used)
    out, worst = {}, 0
    for case in wc.media_names():
        mine, ref = wc.medium(optrace_amd, case), wc.medium(ot, case)
        wl = wc.medium_wavelengths(case, mine)
        n_ref = np.array(ref(wl), dtype=np.float64)
        table = (np.asarray(mine._wls, dtype=np.float64), np.asarray(mine._vals, dtype=np.float64)) if mine.spectrum_type == "Data" else None
        pairs = [wc.split(wc.exact_index(wc.model_of(mine), wc.coefficients(mine), w, table)) for w in wl]
        hi, lo = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs], dtype=np.float32)
        out.update({f"n/{case}/wl": wl, f"n/{case}/ref": n_ref, f"n/{case}/hi": hi, f"n/{case}/lo": lo})
        err = np.abs(n_ref.astype(wc.LD) - wc.join(hi, lo))
        print(f"n/{case:24s} {mine.spectrum_type:22s} the reference is {float(err.max()):.2e} from the truth", flush=True)
    for case in wc.FILTER_CASES:
        kw = wc.FILTER_CASES[case][0]
        ref = wc.filter_spectrum(ot, case)
        wl = wc.filter_wavelengths(case)
        T_ref = np.array(ref(wl), dtype=np.float64)
        pairs = [wc.split(wc.exact_transmission(kw, w)) for w in wl]
        hi, lo = np.array([a for a, _ in pairs]), np.array([b for _, b in pairs], dtype=np.float32)
        out.update({f"T/{case}/wl": wl, f"T/{case}/ref": T_ref, f"T/{case}/hi": hi, f"T/{case}/lo": lo})
        if kw["spectrum_type"] == "Gaussian" and not kw.get("inverse"):
            d = int(wc.ulp32(T_ref, hi).max())
            worst = max(worst, d)
            print(f"T/{case:24s} the reference's exp is up to {d} float32 units from the truth, {int(np.count_nonzero(T_ref == 0))} zeros")
        else:
            print(f"T/{case:24s} the reference is {float(np.abs(T_ref - hi).max()):.2e} from the truth")
    out["gauss_ulp"] = np.int64(worst)
    print("gauss_ulp", worst)
    return out


def main(path) -> None:
    out = {}
    for name in oc.SCENES:
        out.update(outline_scene(name))
    out.update(wavelength_part())
    oc.write_npz(path, out)
    print(pathlib.Path(path).stat().st_size, "bytes")


if __name__ == "__main__":
    import warnings
    warnings.simplefilter("ignore")
    main(sys.argv[1] if len(sys.argv) > 1 else HERE / "wavelength_step.npz")
