"""optrace_amd.load and the markers on the host: every record of tests/golden/load.npz (the reference's load_agf /
load_zmx on the files under tests/golden/load, written by tests/golden/generate_golden_load.py) reproduced.  CPU only.

Tolerances.  Names, order, modes, classes, texts, exception classes and messages, warning counts: equal.  Numbers that are
parsed (coefficients, radii of apertures, conic constants, thicknesses): bit-equal.  Numbers the loader computes
(R = 1 / CURV, z positions as sums of thicknesses, the Abbe model's n at three lines): 1e-15 relative.  TMA values: as
tests/test_tma_host.py holds the same quantities -- abcd 1e-13 of max |abcd|, efl and bfl rtol 1e-12, bfl (a difference
of z positions) additionally atol 1e-12 times the largest |z| of the system."""
import warnings

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi, base as _base, load as _load

import load_cases as lc
from helpers import load, assert_close

RTOL, ABCD_TOL, COMPUTED_RTOL = 1e-12, 1e-13, 1e-15


@pytest.fixture(scope="module")
def golden():
    return load("load.npz")


@pytest.fixture()
def no_device(monkeypatch):
    """Any use of the native library fails the test."""
    def refuse(*a, **k):
        raise AssertionError("the loader must not touch the device")
    monkeypatch.setattr(_capi, "load_library", refuse)


def recorded(call):
    """(result, warning texts) of a call with warnings switched on."""
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        res = call()
    return res, [str(w.message) for w in caught if issubclass(w.category, ot.OptraceWarning)]


def same_strings(got, want, what):
    assert [str(v) for v in got] == [str(v) for v in want], what


# ---- catalogues ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("file", lc.CATALOGUES)
def test_catalogue_matches_reference(golden, no_device, file):
    k = f"agf/{file}"
    state, texts = recorded(lambda: lc.catalogue_state(ot, file, k))
    for key in ("names", "modes", "descs"):
        same_strings(state[f"{k}/{key}"], golden[f"{k}/{key}"], key)
    assert np.array_equal(state[f"{k}/sizes"], golden[f"{k}/sizes"])
    assert state[f"{k}/coeff"].tobytes() == golden[f"{k}/coeff"].tobytes(), "coefficients are parsed: bit-equal"
    want = [str(v) for v in golden[f"{k}/warn"]]
    assert len(texts) == len(want), (texts, want)
    # the texts agree up to the digits of the computed n and V in them
    assert [t.split(":")[0] for t in texts] == [t.split(":")[0] for t in want]


def test_subset_catalogue_loads_without_a_device_and_covers_the_formulas(no_device):
    with ot.global_options.no_warnings():
        d = ot.load_agf(str(lc.LOAD / lc.SUBSET))
    assert len(d) >= 30 and all(isinstance(n, ot.RefractionIndex) for n in d.values())
    modes = {n.spectrum_type for n in d.values()}
    # every formula number that occurs in a catalogue of the reference (4 and 10 occur in none)
    assert modes == set(_load._AGF_FORMULAS) - {"Sellmeier2", "Extended"}
    assert d["N-BK7"].desc == "N-BK7" and d["N-BK7"].spectrum_type == "Sellmeier1"


def test_catalogue_warnings_use_the_reference_thresholds(tmp_path, no_device):
    rec = ("NM {name} 1 0 {n} {V} 0 0 0\nCD 2.2718929 -1.0108077E-2 1.0592509E-2 2.0816965E-4 -7.6472538E-6 4.9240991E-7\n"
           "LD {lo} 2.5\n")
    nd = 1.5167997  # of these Schott-formula coefficients (BK7) at 587.5618 nm
    text = (rec.format(name="FINE", n=nd + 0.9e-4, V=64.17 + 0.25, lo=0.3) + rec.format(name="INDEX", n=nd + 1.2e-4, V=64.17, lo=0.3)
            + rec.format(name="ABBE", n=nd, V=64.17 + 0.4, lo=0.3) + rec.format(name="INFRARED", n=nd, V=64.17, lo=0.9)
            + "NM LOW 1 0 1.5 60 0 0 0\nCD 0.5 0 0 0 0 0\nLD 0.3 2.5\n" + "NM SHORT 2 0 1.5 60 0 0 0\nCD 1.0 0.01\nLD 0.3 2.5\n")
    path = tmp_path / "made.agf"
    path.write_text(text)
    d, texts = recorded(lambda: ot.load_agf(str(path)))
    assert list(d) == ["FINE", "INDEX", "ABBE", "INFRARED", "SHORT"]
    assert len(texts) == 5
    assert texts[0].startswith("INDEX: Index from file is") and texts[1].startswith("ABBE: The Abbe number from file is")
    assert texts[2].startswith("INFRARED wavelength range [900.0, 2500.0]nm does not overlap")
    assert texts[3].startswith("Error for material LOW: Refraction index below 1")
    assert texts[4].startswith("SHORT: Index from file is 1.5, but calculated index is 1.42")
    assert d["SHORT"].coeff == [1.0, 0.01, 0., 0., 0., 0.], "missing coefficients are zeros"
    with pytest.raises(FileNotFoundError):
        ot.load_agf(str(tmp_path / "absent.agf"))


# ---- prescriptions -------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def n_dict():
    with ot.global_options.no_warnings():
        return lc.media(ot)


@pytest.mark.parametrize("no_marker", [False, True], ids=["marker", "no_marker"])
@pytest.mark.parametrize("file", lc.PRESCRIPTIONS)
def test_prescription_matches_reference(golden, n_dict, no_device, file, no_marker):
    k = f"zmx/{file}/{'no_marker' if no_marker else 'marker'}"
    state, texts = recorded(lambda: lc.load_outcome(ot, file, n_dict, no_marker, k))
    same_strings(state[f"{k}/raised"], golden[f"{k}/raised"], "exception class and message")
    assert len(texts) == len(golden[f"{k}/warn"]), (texts, golden[f"{k}/warn"])
    same_strings([t.split()[:2] for t in texts], [str(t).split()[:2] for t in golden[f"{k}/warn"]], "kinds of warnings")
    if str(golden[f"{k}/raised"][0]) != "none":
        return
    for key in ("cls", "texts"):
        same_strings(state[f"{k}/{key}"], golden[f"{k}/{key}"], key)
    assert np.array_equal(state[f"{k}/counts"], golden[f"{k}/counts"])
    assert np.array_equal(state[f"{k}/sizes"], golden[f"{k}/sizes"])
    assert state[f"{k}/parsed"].tobytes() == golden[f"{k}/parsed"].tobytes(), "parsed numbers: bit-equal"
    assert_close(state[f"{k}/computed"], golden[f"{k}/computed"], rtol=COMPUTED_RTOL, what="computed numbers")
    assert_close(state[f"{k}/extent"], golden[f"{k}/extent"], rtol=COMPUTED_RTOL, what="extent")
    assert (f"{k}/tma" in golden.files) == (f"{k}/tma" in state)
    if f"{k}/tma" in state:
        got, ref = state[f"{k}/tma"], golden[f"{k}/tma"]
        z_scale = float(np.abs(golden[f"{k}/extent"][4:]).max())
        assert_close(got[0], ref[0], rtol=RTOL, what="efl")
        assert_close(got[1], ref[1], rtol=RTOL, atol=RTOL * z_scale, what="bfl")
        assert np.abs(got[2:] - ref[2:]).max() <= ABCD_TOL * np.abs(ref[2:]).max(), "abcd"


def test_objective_has_the_depth_the_reference_counts(n_dict):
    with ot.global_options.no_warnings():
        G = ot.load_zmx(str(lc.LOAD / "Nikon_1p25NA_60x_US7889433B2_MultiConfig_v2.zmx"), n_dict)
    kinds = [type(s).__name__ for s in G.tracing_surfaces]
    assert len(G.lenses) == 38 and kinds.count("SphericalSurface") == 72 and kinds.count("CircularSurface") == 4
    gaps = [b.front.pos[2] - a.back.pos[2] for a, b in zip(G.lenses, G.lenses[1:])]
    assert sum(1 for g in gaps if abs(g - 1e-7) < 1e-12) >= 10, "cemented faces are doubled at a 1e-7 mm offset"


def test_marker_of_a_loaded_group_sits_beside_it(n_dict):
    with ot.global_options.no_warnings():
        G = ot.load_zmx(str(lc.LOAD / "zmax_49360.zmx"), n_dict)
        bare = ot.load_zmx(str(lc.LOAD / "zmax_49360.zmx"), n_dict, no_marker=True)
    assert len(G.markers) == 1 and not bare.markers
    m, ext = G.markers[0], bare.extent
    assert isinstance(m, ot.PointMarker) and m.label_only and m.desc == G.long_desc != ""
    assert np.array_equal(m.pos, [ext[0] - 1.5, (ext[2] + ext[3]) / 2, (ext[4] + ext[5]) / 2])


# ---- encoding ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("encoding,mark", [("utf-8", b""), ("utf-8", b"\xef\xbb\xbf"), ("utf-16-le", b"\xff\xfe"),
                                           ("utf-16-be", b"\xfe\xff"), ("utf-32-le", b"\xff\xfe\x00\x00"),
                                           ("utf-32-be", b"\x00\x00\xfe\xff"), ("latin-1", b"")])
@pytest.mark.parametrize("newline", ["\n", "\r\n"])
def test_text_encodings_give_the_same_lines(tmp_path, encoding, mark, newline):
    lines = ["MODE SEQ", "NAME Grün é µm", "UNIT MM X W X CM MR CPMM", "SURF 0", "  DISZ INFINITY", "last"]
    path = tmp_path / "file.zmx"
    path.write_bytes(mark + newline.join(lines).encode(encoding))
    assert _load._read_lines(str(path)) == [line + "\n" for line in lines[:-1]] + ["last"]


def test_invalid_utf8_without_mark_is_latin1(tmp_path):
    path = tmp_path / "file.agf"
    path.write_bytes(b"CC caf\xe9\nNM X 1\n")
    assert _load._read_lines(str(path)) == ["CC café\n", "NM X 1\n"]


# ---- markers -------------------------------------------------------------------------------------------------------
def test_marker_constructors_and_checks():
    p = ot.PointMarker("text", [1, 2, 3], text_factor=2, marker_factor=0.5, label_only=True, long_desc="long")
    assert (p.desc, p.long_desc, p.text_factor, p.marker_factor, p.label_only) == ("text", "long", 2, 0.5, True)
    assert isinstance(p.front, ot.Point) and not p.has_back() and np.array_equal(p.pos, [1, 2, 3])
    assert p.extent == (1, 1, 2, 2, 3, 3)
    q = ot.PointMarker("", [0, 0, 0])
    assert (q.text_factor, q.marker_factor, q.label_only) == (1., 1., False)
    m = ot.LineMarker(r=2, pos=[0, 1, 5], desc="line", angle=90, text_factor=1.5, line_factor=3)
    assert isinstance(m.front, ot.Line) and m.front.r == 2 and m.front.angle == 90 and m.desc == "line"
    assert (m.text_factor, m.line_factor) == (1.5, 3)
    assert_close(m.extent, [0, 0, -1, 3, 5, 5], rtol=0, atol=1e-15, what="extent")
    assert ot.geometry.PointMarker is ot.PointMarker and ot.geometry.LineMarker is ot.LineMarker
    for bad in (lambda: ot.PointMarker("a", [0, 0, 0], text_factor="2"), lambda: ot.PointMarker("a", [0, 0, 0], marker_factor=None),
                lambda: ot.PointMarker("a", [0, 0, 0], label_only=1), lambda: ot.PointMarker(5, [0, 0, 0]),
                lambda: ot.LineMarker(r=1, pos=[0, 0, 0], line_factor=[1]), lambda: ot.LineMarker(r=1, pos=[0, 0, 0], text_factor="1"),
                lambda: ot.LineMarker(r=1, pos=[0, 0, 0], desc=3), lambda: setattr(p, "text_factor", "big")):
        with pytest.raises(TypeError):
            bad()
    with pytest.raises(ValueError):
        ot.LineMarker(r=-1, pos=[0, 0, 0])
    with pytest.raises(ValueError):
        ot.PointMarker("a", [0, 0])
    with pytest.raises(RuntimeError):
        p.pos = [0, 0, 1]
    with pytest.raises(AttributeError):
        p.colour = "red"
    p.move_to([4, 5, 6])
    p.text_factor = 3
    assert np.array_equal(p.pos, [4, 5, 6]) and p.text_factor == 3


def test_group_routes_moves_and_flips_markers():
    n = ot.RefractionIndex("Constant", n=1.5)
    L = ot.Lens(ot.SphericalSurface(r=2, R=10), ot.SphericalSurface(r=2, R=-10), de=0.2, pos=[0, 0, 10], n=n)
    p, m = ot.PointMarker("p", [1, 2, 4]), ot.LineMarker(r=1, pos=[0, -1, 20], angle=30)
    G = ot.Group([L, p])
    G.add(m)
    assert G.markers == [p, m] and G.lenses == [L] and G.has(p) and [type(e) for e in G.elements] == [ot.PointMarker, ot.Lens, ot.LineMarker]
    assert G.extent[4] == 4 and G.extent[5] == 20 and len(G.tracing_surfaces) == 2
    G.move_to([1, 2, 5])  # the first element along z is the point marker
    assert np.array_equal(p.pos, [1, 2, 5]) and np.array_equal(m.pos, [0, -1, 21]) and L.pos[2] == 11
    G.rotate(90)
    assert_close(p.pos, [-2, 1, 5], rtol=0, atol=1e-15, what="rotated") and m.front.angle == 120
    assert m.front.angle == 120
    G.flip(y0=0, z0=10)
    assert_close(p.pos, [-2, -1, 15], rtol=0, atol=1e-15, what="flipped")
    assert m.pos[2] == -1 and m.front.angle == -120 and [type(e) for e in G.elements] == [ot.LineMarker, ot.Lens, ot.PointMarker]
    assert G.remove(p) and G.markers == [m] and not G.remove(p)
    H = ot.Group([G])
    assert H.markers == [m]
    G.clear()
    assert not G.markers


def test_markers_are_no_scene_change():
    with ot.global_options.no_warnings():
        RT = ot.Raytracer(outline=[-5, 5, -5, 5, -10, 40])
        RT.add(ot.RaySource(ot.CircularSurface(r=1), pos=[0, 0, -5]))
        RT.add(ot.Lens(ot.SphericalSurface(r=2, R=10), ot.SphericalSurface(r=2, R=-10), de=0.2, pos=[0, 0, 5],
                       n=ot.RefractionIndex("Constant", n=1.5)))
        snap, full, epoch = RT.tracing_snapshot(), RT.property_snapshot(), _base.mutation_epoch()
        m = ot.PointMarker("focus", [0, 0, 12.])
        RT.add(m)
        m.move_to([0, 0, 13.])
        m.text_factor = 2.
        RT.add(ot.LineMarker(r=2, pos=[0, 0, 20.]))
        assert _base.mutation_epoch() == epoch, "markers are untracked"
        assert RT.tracing_snapshot() == snap and len(RT.markers) == 2
        cmp = RT.compare_property_snapshot(full, RT.property_snapshot())
        assert cmp["Markers"] and not any(cmp[key] for key in ("Lenses", "Ambient", "RaySources", "Detectors"))
        RT.remove(m)
        assert _base.mutation_epoch() == epoch and len(RT.markers) == 1
        RT.add(ot.Aperture(ot.RingSurface(r=2, ri=1), pos=[0, 0, 9.]))
        assert _base.mutation_epoch() > epoch, "tracked elements still count"
        from optrace_amd.scene import CompiledScene
        assert CompiledScene(RT).nt == 5, "a marker is never compiled into a scene"
