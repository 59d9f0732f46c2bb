#!/usr/bin/env python3
"""Fixtures for the import of ZEMAX files (optrace_amd.load), from the upstream NumPy reference.  Like generate_golden.py
this runs only where the reference is installed; what it writes under tests/golden/ is committed, the reference is not.
    python tests/golden/generate_golden_load.py

tests/golden/load/
  *.zmx, *.agf, *.AGF     prescription and catalogue files of the reference's test and example data, copied unchanged
  subset.agf              line for line the records of exactly the glasses the copied prescriptions name (taken from the
                          four large example catalogues, which are too large to copy), plus one glass of every formula
                          number that occurs in any catalogue of the reference
tests/golden/load.npz     agf/<file>/...: names in order, modes, coefficients, number and text of the warnings
                          zmx/<file>/<marker|no_marker>/...: load_cases.load_outcome (state of the group incl. TMA values at
                          587.56 nm, or class and message of what was raised), warn: number of warnings
                          focus/achromat/...: focus_search("RMS Spot Size") on the rays of trace_zmx_achromat.npz
                          oracle/<fixture>: largest position deviation of the C oracle from the reference [mm]
tests/golden/trace_zmx_<name>.npz   injected initial rays, every ray section and the counters, in the format of the
                          trace_<scene>.npz of generate_golden.py (without the detector stage), for load_cases.TRACE_FIXTURES

The reference decides the text encoding with the `chardet` package, which oracle/refload.py replaces by an empty stand-in.
Its `detect` is filled in here by byte-order mark, else UTF-8, else Latin-1.  Every fixture file is ASCII text with or
without a mark, so the stand-in decides nothing that reaches a golden value; `check_plain_text` asserts that.

Printed: per traced fixture the share of rays the reference delivers through the last surface, the seed used, and the
largest deviation of the C oracle's positions from the reference's -- the yardstick for the position tolerances of
tests/test_gpu_load.py -- together with the same figure for trace_double_gauss."""
from __future__ import annotations

import shutil
import sys
import types
import warnings

import numpy as np

import generate_golden as gg  # (imports the reference, tests/scenes.py and the oracle loader)

import load_cases as lc

sys.path.insert(0, str(gg.ROOT))  # optrace_amd itself: its loader and scene compiler feed the C oracle

ot = gg.ot
HERE = gg.HERE
REF = gg.refload.REFERENCE_ROOT
FILES = REF + "/tests/test_files"
RES = REF + "/examples/resources"

SOURCES = {
    "zmax_49360.zmx": FILES + "/edmund_zmx/files", "Smith1998b.zmx": FILES + "/LensLibrary/files",
    "Liang2006d.zmx": FILES + "/LensLibrary/files", "7558005b.zmx": FILES + "/LensLibrary/files",
    "1843519.zmx": FILES + "/LensLibrary/files", "UK565851-1.zmx": RES + "/eyepiece",
    "Nikon_1p25NA_60x_US7889433B2_MultiConfig_v2.zmx": RES + "/microscope",
    **{f: FILES + "/edge_cases_zmx" for f in ("minimal.zmx", "zmx_invalid_material.zmx", "zmx_invalid_mode.zmx",
                                               "zmx_invalid_surface_type.zmx", "zmx_invalid_unit.zmx",
                                               "zmx_special_cases.zmx")},
    "error.agf": FILES + "/edge_cases_agf", "EYE.AGF": FILES + "/eye_zemax/files",
    **{f: FILES + "/zemaxglass/files" for f in ("topas.agf", "zeon.agf", "heraeus.agf", "isuzu.agf", "liebetraut.agf",
                                                 "umicore.agf", "arton.agf", "rad_hard.agf", "misc.agf")},
}
LARGE = [RES + f"/materials/{name}.agf" for name in ("schott", "ohara", "hikari", "hoya")]  # later ones win, as in
# the reference's microscope example (schott | ohara | hikari | hoya)


def _decode(raw: bytes) -> tuple:
    for mark, enc in ((b"\xff\xfe\x00\x00", "utf-32"), (b"\x00\x00\xfe\xff", "utf-32"), (b"\xef\xbb\xbf", "utf-8-sig"),
                      (b"\xff\xfe", "utf-16"), (b"\xfe\xff", "utf-16")):
        if raw.startswith(mark):
            return enc, raw.decode(enc)
    try:
        return "utf-8", raw.decode("utf-8")
    except UnicodeDecodeError:
        return "latin-1", raw.decode("latin-1")


def install_chardet() -> None:
    ch = sys.modules["chardet"]
    ch.detect = lambda raw, **kw: {"encoding": _decode(raw)[0]}
    ch.EncodingEra = types.SimpleNamespace(MODERN_WEB=0)


def check_plain_text(path) -> None:
    """ASCII with or without a mark: the same text whatever decoder a detector could pick, and it round-trips."""
    raw = open(path, "rb").read()
    enc, text = _decode(raw)
    assert text.isascii(), path
    if enc in ("utf-8", "latin-1"):
        assert raw.decode("utf-8") == raw.decode("latin-1") == raw.decode("ascii") == text
    base = enc.replace("-sig", "")
    assert text.encode(base).decode(base) == text, path


def records(path: str) -> dict:
    """name -> (formula number, lines) of every record of a catalogue."""
    out, cur = {}, None
    for line in _decode(open(path, "rb").read())[1].replace("\r\n", "\n").split("\n"):
        if line[:2] == "NM":
            w = line.split()
            cur = out[w[1]] = (int(float(w[2])), [])
        if cur is not None and line.strip():
            cur[1].append(line)
    return out


def glasses_named(path) -> list:
    text = _decode(open(path, "rb").read())[1]
    return sorted({l.split()[1] for l in text.splitlines() if l[2:6] == "GLAS"} - {"___BLANK"})


def copy_files() -> None:
    (HERE / "load").mkdir(exist_ok=True)
    for name, src in SOURCES.items():
        shutil.copyfile(f"{src}/{name}", HERE / "load" / name)
        (HERE / "load" / name).chmod(0o644)
        check_plain_text(HERE / "load" / name)


def write_subset() -> None:
    import glob
    large = {}
    for path in LARGE:
        large.update({name: (num, lines, path) for name, (num, lines) in records(path).items()})
    chosen, missing = {}, []
    for zmx in lc.PRESCRIPTIONS:
        if not (HERE / "load" / zmx).exists():
            continue
        for name in glasses_named(HERE / "load" / zmx):
            if name in large:
                chosen[name] = large[name]
            else:
                missing.append(f"{zmx}: {name}")
    print("glasses named by the prescriptions and absent from the four example catalogues:", missing)
    # one glass of every formula number that occurs anywhere in the reference's catalogues
    have = {num for num, _, _ in chosen.values()}
    seen = set(have)
    everywhere = sorted(glob.glob(REF + "/**/*.agf", recursive=True) + glob.glob(REF + "/**/*.AGF", recursive=True))
    for path in LARGE + everywhere:
        for name, (num, lines) in records(path).items():
            seen.add(num)
            if num not in have and 1 <= num <= 13 and name not in chosen:
                have.add(num)
                chosen[name] = (num, lines, path)
    print("formula numbers in the reference's catalogues:", sorted(seen), "- in subset.agf:", sorted(have),
          "- in no catalogue:", sorted(set(range(1, 14)) - seen))
    with open(HERE / "load" / lc.SUBSET, "w", encoding="ascii", newline="\n") as f:
        f.write("CC Records of single glasses taken line for line from larger catalogues (test data)\n")
        for name, (num, lines, path) in chosen.items():
            f.write("\n".join(lines) + "\n")
    check_plain_text(HERE / "load" / lc.SUBSET)
    print(f"subset.agf: {len(chosen)} glasses, {(HERE / 'load' / lc.SUBSET).stat().st_size} bytes")


def counted(call):
    """(result, warning texts) of a call with the reference's warnings switched on."""
    ot.global_options.show_warnings = True
    try:
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            res = call()
    finally:
        ot.global_options.show_warnings = False
    return res, [str(w.message) for w in caught]


def gen_load(out: dict) -> None:
    for file in lc.CATALOGUES:
        state, texts = counted(lambda: lc.catalogue_state(ot, file, f"agf/{file}"))
        out.update(state)
        out[f"agf/{file}/warn"] = np.array(texts) if texts else np.zeros(0, dtype="U1")
        print(f"  {file}: {len(state[f'agf/{file}/names'])} glasses, {len(texts)} warnings")
    n_dict = lc.media(ot)
    for file in lc.PRESCRIPTIONS:
        for no_marker in (False, True):
            prefix = f"zmx/{file}/{'no_marker' if no_marker else 'marker'}"
            state, texts = counted(lambda: lc.load_outcome(ot, file, n_dict, no_marker, prefix))
            out.update(state)
            out[f"{prefix}/warn"] = np.array(texts) if texts else np.zeros(0, dtype="U1")
        print(f"  {file}: {state[f'{prefix}/raised']}, {len(texts)} warnings",
              state.get(f"{prefix}/counts", ""), state.get(f"{prefix}/tma", "")[:2])


def oracle_positions(fixture: str, g: dict) -> np.ndarray:
    """p_list of the C oracle for a fixture, traced through optrace_amd's own loader and scene compiler."""
    import optrace_amd as amd
    from optrace_amd.scene import CompiledScene
    import oracle_bridge as ob
    system, no_pol = lc.TRACE_FIXTURES[fixture]
    with amd.global_options.no_warnings():
        RT = lc.traced_scene(amd, system, no_pol=no_pol)
        RT._geometry_checks()
    assert not RT.geometry_error
    sc = CompiledScene(RT)
    rays = ob.HostRays(int(g["N"]), sc.nt, no_pol)
    rays.set_initial(g["p0"], g["s0"], None if no_pol else g["pol0"], g["w0"], g["wl"])
    msgs, st = ob.trace(sc.desc, rays, None)
    assert st == 0
    return rays, msgs


def record_trace(system: str, no_pol: bool, N: int, seed: int):
    RT, rec, normals = gg.trace_recorded(lambda ot_, **kw: lc.traced_scene(ot_, system, **kw), N, seed, no_pol=no_pol)
    assert not normals
    g = dict(N=N, seed=seed)
    g["p0"], g["s0"] = np.vstack([r[0] for r in rec]), np.vstack([r[1] for r in rec])
    g["w0"] = np.concatenate([r[3] for r in rec])
    g["wl"] = np.concatenate([r[4] for r in rec]).astype(np.float32)
    if not no_pol:
        g["pol0"] = np.vstack([r[2] for r in rec])
    g["N_list"] = RT.rays.N_list
    g["p_list"], g["w_list"], g["n_list"] = np.array(RT.rays.p_list), np.array(RT.rays.w_list), np.array(RT.rays.n_list)
    g["s_final"] = np.array(RT.rays.s0_list)
    assert np.array_equal(g["wl"], RT.rays.wl_list)
    if not no_pol:
        g["pol_list"] = np.array(RT.rays.pol_list)
    g["msgs"] = np.array(RT._msgs)
    return RT, g


def deviation(rays, msgs, g: dict) -> float:
    """Largest position deviation oracle - reference [mm]; inf where masks or counters differ."""
    if not (np.array_equal(msgs, g["msgs"]) and np.array_equal(rays.w_list > 0, g["w_list"] > 0)):
        return np.inf
    return float(np.abs(rays.p_list - g["p_list"]).max())


def gen_traces(out: dict) -> None:
    for j, (fixture, (system, no_pol)) in enumerate(lc.TRACE_FIXTURES.items()):
        N = lc.TRACED[system][-1]
        for seed in range(1400 + 10 * j, 1410 + 10 * j):  # the next seed where oracle and reference disagree on a mask
            RT, g = record_trace(system, no_pol, N, seed)
            rays, msgs = oracle_positions(fixture, g)
            dev = deviation(rays, msgs, g)
            if np.isfinite(dev):
                break
            print(f"  {fixture}: seed {seed} puts a ray within rounding of an edge (oracle and reference differ), next")
        else:
            raise AssertionError(fixture)
        nt = g["p_list"].shape[1]
        through = float(np.count_nonzero(g["w_list"][:, nt - 2] > 0)) / N  # alive behind the last surface
        if system == "nikon60x":
            assert through >= 0.5, through
        out[f"oracle/{fixture}"] = dev
        np.savez_compressed(HERE / f"trace_zmx_{fixture}.npz", **g)
        size = (HERE / f"trace_zmx_{fixture}.npz").stat().st_size
        assert size < 1024 * 1024, size
        print(f"trace_zmx_{fixture}.npz: seed {seed}, N={N}, {nt} sections, {through:.1%} of the rays pass the last "
              f"surface, {size} bytes, oracle - reference: {dev:.3g} mm, msgs={g['msgs'].sum(axis=1)}")
        if fixture == "achromat":
            F2 = RT.tma().focal_points[1]
            with ot.global_options.no_warnings():
                res, d = RT.focus_search("RMS Spot Size", z_start=F2)
            k = "focus/achromat"
            out[f"{k}/F2"], out[f"{k}/x"], out[f"{k}/fun"] = F2, float(res.x), float(res.fun)
            out[f"{k}/bounds"], out[f"{k}/N"] = np.array(d["bounds"]), d["N"]
            print(f"focus achromat: focal_points[1]={F2:.9g}, RMS focus {float(res.x):.9g}, residual "
                  f"{float(res.x) - F2:+.3g} mm (search span {d['bounds'][1] - d['bounds'][0]:.4g} mm, {d['N']} rays)")


def yardstick_double_gauss() -> None:
    """The oracle's deviation on an existing fixture: the margin the project's 1e-11 mm has at 17 sections."""
    import test_oracle_golden as tog
    g, RT, sc, rays, msgs = tog.oracle_trace("double_gauss")
    print(f"trace_double_gauss ({sc.nt} sections): oracle - reference: {np.abs(rays.p_list - g['p_list']).max():.3g} mm")


if __name__ == "__main__":
    install_chardet()
    copy_files()
    write_subset()
    out = {}
    gen_load(out)
    gen_traces(out)
    yardstick_double_gauss()
    np.savez_compressed(HERE / "load.npz", **out)
    print("load.npz", len(out))
