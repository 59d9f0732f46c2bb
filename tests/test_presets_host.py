"""The preset catalogue against the reference's (tests/golden/presets.npz, generator: tests/golden/generate_golden_presets.py
with tests/scenes_presets.py): names, list memberships and orders, types and descriptions of media and spectra, host
values of the spectra, spectral lines, PSF samples, geometry presets and the exception classes of invalid arguments.
CPU only: what needs the device (indices, tracing, sampling, convolution) is in tests/test_gpu_presets.py."""
import types

import numpy as np
import pytest

import optrace_amd as ot
import scenes_presets as sp
from helpers import load


@pytest.fixture(scope="module")
def ref():
    return load("presets.npz")


def test_groups_are_modules():
    import optrace_amd.presets as presets
    from optrace_amd.presets import (geometry, image, light_spectrum, psf, refraction_index, spectral_lines,  # noqa: F401
                                     spectrum)
    assert presets is ot.presets
    for name in ("geometry", "image", "light_spectrum", "psf", "refraction_index", "spectral_lines", "spectrum"):
        assert isinstance(getattr(ot.presets, name), types.ModuleType), name
    assert ot.presets.light_spectrum.d65 is light_spectrum.d65
    assert ot.presets.refraction_index.BK7 is refraction_index.BK7
    assert ot.presets.geometry.arizona_eye is geometry.arizona_eye


def test_media_names_lists_and_descriptions(ref):
    mod = ot.presets.refraction_index
    names = [str(n) for n in ref["media/names"]]
    assert len(names) == 45 and sp.names_of(mod, mod.all_presets) == names
    for lst in sp.MEDIA_LISTS:
        assert sp.names_of(mod, getattr(mod, lst)) == [str(n) for n in ref[f"media/list/{lst}"]], lst
    assert [len(getattr(mod, lst)) for lst in sp.MEDIA_LISTS] == [22, 14, 9, 45]
    for j, name in enumerate(names):
        m = getattr(mod, name)
        assert type(m) is ot.RefractionIndex, name
        assert (m.spectrum_type, m.desc, m.long_desc) == tuple(str(ref[f"media/{k}"][j]) for k in ("type", "desc", "long_desc")), name
    assert callable(mod.soda_lime.func) and mod.soda_lime.spectrum_type == "Function"


def test_index_at_wavelengths_float32_cannot_hold(ref):
    """n(spectral line given as a double), as a lens design calculation asks for it (examples/achromat.py): evaluated in
    float64 on the host, no device needed.  The kernel's float32 wavelength would be off by up to 3e-5 nm, 1e-9 in n.
    Tolerances per model as tests/test_gpu_parity.py::test_refraction_index has them for the device formulas."""
    mod, lines = ot.presets.refraction_index, np.array(ot.presets.spectral_lines.all_lines)
    assert not np.array_equal(lines.astype(np.float32), lines)
    for j, name in enumerate(str(n) for n in ref["media/names"]):
        m = getattr(mod, name)
        exact = m.spectrum_type in ("Constant", "Abbe", "Data", "Sellmeier1", "Sellmeier3")
        np.testing.assert_allclose(m(lines), ref["media/n_lines"][j], rtol=4e-16 if exact else 1e-13, atol=0, err_msg=name)
    n_e = mod.LAK8(ot.presets.spectral_lines.e)   # a single wavelength, as the example passes it
    want = ref["media/n_lines"][list(ref["media/names"]).index("LAK8")][4]
    assert np.shape(n_e) == () and abs(float(n_e) - want) <= 4e-16 * want


@pytest.mark.parametrize("prefix,module,cls,lists", [("light", "light_spectrum", "LightSpectrum", sp.LIGHT_LISTS),
                                                     ("spectrum", "spectrum", "Spectrum", sp.SPECTRUM_LISTS)])
def test_spectra_names_lists_descriptions_and_values(ref, prefix, module, cls, lists):
    mod = getattr(ot.presets, module)
    names = [str(n) for n in ref[f"{prefix}/names"]]
    assert sp.names_of(mod, mod.all_presets) == names
    for lst in lists:
        assert sp.names_of(mod, getattr(mod, lst)) == [str(n) for n in ref[f"{prefix}/list/{lst}"]], lst
    for j, name in enumerate(names):
        s = getattr(mod, name)
        assert type(s) is getattr(ot, cls), name
        mine = (s.spectrum_type, s.desc, s.long_desc, s.quantity, s.unit)
        assert mine == tuple(str(ref[f"{prefix}/{k}"][j]) for k in ("type", "desc", "long_desc", "quantity", "unit")), name
        if s.is_continuous():
            # table interpolation and sums of Gaussians in float64 on both sides
            np.testing.assert_allclose(s(sp.WL), ref[f"{prefix}/values"][j], rtol=1e-13, atol=0, err_msg=name)
        else:
            assert np.isnan(ref[f"{prefix}/values"][j]).all()
            assert np.array_equal(np.asarray(s.lines, dtype=np.float64), ref[f"{prefix}/{name}/lines"]), name
            assert np.array_equal(np.asarray(s.line_vals, dtype=np.float64), ref[f"{prefix}/{name}/line_vals"]), name


def test_power_factors(ref):
    mine = [getattr(ot.presets.light_spectrum, k) for k in sp.POWER_FACTORS]
    assert all(type(v) is float for v in mine) and np.array_equal(mine, ref["light/power_factors"])


def test_spectral_lines(ref):
    mod = ot.presets.spectral_lines
    for lst in sp.LINE_LISTS:
        assert type(getattr(mod, lst)) is list and np.array_equal(getattr(mod, lst), ref[f"lines/{lst}"]), lst
    assert sp.names_of(mod, mod.all_lines) == [str(n) for n in ref["lines/names"]]
    assert sp.names_of(mod, mod.all_line_combinations) == [str(n) for n in ref["lines/combinations"]]
    assert all(type(v) is float for v in mod.all_lines)


@pytest.mark.parametrize("case", list(sp.PSF_ARGS))
def test_psf_matches_reference(ref, case):
    """Both sides are a handful of float64 NumPy operations on values in [0, 1]: 1e-12 absolute."""
    img = sp.psf(ot, case)
    assert type(img) is ot.GrayscaleImage
    mine = sp.psf_record(img)
    assert np.array_equal(mine["shape"], ref[f"psf/{case}/shape"])
    assert np.array_equal(mine["s"], ref[f"psf/{case}/s"]), (mine["s"], ref[f"psf/{case}/s"])
    for k in ("grid10", "centre_row"):
        np.testing.assert_allclose(mine[k], ref[f"psf/{case}/{k}"], rtol=0, atol=1e-12, err_msg=k)
    # a sum over n pixels of values that agree to 1e-12 each
    assert abs(mine["sum"] - float(ref[f"psf/{case}/sum"])) <= 1e-12 * img.data.size


def test_invalid_arguments_raise_what_the_reference_raises(ref):
    cases = sp.argument_cases(ot)
    assert list(cases) == [str(n) for n in ref["raises/names"]]
    raised = [sp.outcome(c) for c in cases.values()]
    wrong = [(n, a, str(b)) for n, a, b in zip(cases, raised, ref["raises/raised"]) if a != str(b)]
    assert not wrong, wrong
    assert sum(r != "none" for r in raised) >= 20


def test_geometry_lists(ref):
    mod = ot.presets.geometry
    for lst in sp.GEOMETRY_LISTS:
        assert [f.__name__ for f in getattr(mod, lst)] == [str(n) for n in ref[f"geometry/list/{lst}"]], lst
        assert all(getattr(mod, f.__name__) is f for f in getattr(mod, lst))


@pytest.mark.parametrize("case", list(sp.GEOMETRY_ARGS))
def test_geometry_presets_match_reference(ref, case):
    """Compared like tests/test_host_golden.py compares its states: strings equal, numbers to 1e-12 / 1e-13."""
    G = sp.geometry(ot, case)
    assert type(G) is ot.Group
    assert len(G.elements) == len(G.lenses) + len(G.apertures) + len(G.detectors), "optical elements only, no volume"
    for k, mine in sp.group_state(G).items():
        want = ref[f"geometry/{case}/{k}"]
        if want.dtype.kind in "US":
            assert list(mine) == list(want), k
        else:
            assert mine.shape == want.shape, k
            np.testing.assert_allclose(mine, want, rtol=1e-12, atol=1e-13, equal_nan=True, err_msg=k)


def test_grid_image():
    img = ot.presets.image.grid([3, 2])
    assert type(img) is ot.GrayscaleImage and img.shape == (301, 301) and img.desc == "Grid" and img.s == [3, 2]
    d = img.data
    assert set(np.unique(d)) == {0., 1.}
    lit = np.zeros(301, dtype=bool)
    lit[::30] = True
    assert np.array_equal(d == 1, lit[:, None] | lit[None, :])
    assert np.array_equal(ot.presets.image.grid(extent=[0, 2, -1, 1]).extent, [0, 2, -1, 1])
    with pytest.raises(ValueError):
        ot.presets.image.grid()
