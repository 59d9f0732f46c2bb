"""Refractive indices and filter transmissions on the host: the fixture tests/golden/wavelength_step.npz (the reference's
values and the exact ones, tests/golden/generate_golden_wavelength.py) against the regenerated wavelengths, the reference
against the bars of tests/wavelength_cases.py -- so that no bar asks more than the reference gives --, and the C oracle
(the yardstick of the GPU suites, and with libm's pow and expf the arithmetic of the host-built line tables) against the same
bars.  Prints the reference's and the oracle's distance from the truth per case and the float32 figure that became the
Gaussian bar.  CPU only."""
import numpy as np
import pytest

import optrace_amd as ot

import oracle_bridge as ob
import wavelength_cases as wc
from helpers import load

bits = wc.bits


@pytest.fixture(scope="module")
def g():
    return load("wavelength_step.npz")


def test_wavelengths_cover_the_edges(g):
    for case in wc.media_names():
        ri = wc.medium(ot, case)
        wl = wc.medium_wavelengths(case, ri)
        assert bits(wl, g[f"n/{case}/wl"]), case
        assert wl.shape[0] % 64 != 0 and wl.min() == 380 and wl.max() == 780
        assert np.float32(np.nextafter(np.float32(380), np.float32(400))) in wl and np.float32(np.nextafter(np.float32(780), np.float32(0))) in wl
        if ri.spectrum_type == "Data":
            for node in np.asarray(ri._wls):
                c = np.float32(node)
                assert c in wl and (c == 380 or np.nextafter(c, np.float32(0)) in wl) and (c == 780 or np.nextafter(c, np.float32(1e3)) in wl)
    assert any(not np.all(np.asarray(wc.medium(ot, c)._wls).astype(np.float32) == wc.medium(ot, c)._wls) for c in ("Data/odd_nodes",))
    # the table that is not equidistant: steps differ by 4e-5 nm and more, about a float32 spacing, so float32(node) lies
    # below some nodes and above others -- and the product's own check of the nodes accepts it
    u = np.asarray(wc.medium(ot, "Data/uneven")._wls)
    assert np.ptp(np.diff(u)) >= 7e-5 and np.std(np.diff(u)) < 1e-4
    r = u.astype(np.float32).astype(np.float64)
    assert np.count_nonzero(r < u) >= 3 and np.count_nonzero(r > u) >= 3
    for case, (kw, marks) in wc.FILTER_CASES.items():
        wl = wc.filter_wavelengths(case)
        assert bits(wl, g[f"T/{case}/wl"]), case
        if kw["spectrum_type"] == "Rectangle":
            for e in (kw["wl0"], kw["wl1"]):
                c = np.float32(e)
                assert {c, np.nextafter(c, np.float32(0)), np.nextafter(c, np.float32(1e3))} <= set(wl)
        if kw["spectrum_type"] == "Data":
            assert np.count_nonzero(wl < 400) >= 4 and np.count_nonzero(wl > 700) >= 4 and 400 in wl and 700 in wl
            assert np.all(g[f"T/{case}/ref"][(wl < 400) | (wl > 700)] == (1.0 if kw.get("inverse") else 0.0))
    assert float(np.float32(450.1)) != 450.1 and float(np.float32(550.123)) != 550.123


@pytest.mark.parametrize("case", wc.media_names())
def test_reference_and_oracle_indices_meet_the_bar(g, case, capsys):
    ri = wc.medium(ot, case)
    wl = g[f"n/{case}/wl"]
    pool: list = []
    md = ri._desc(pool)
    orc = ob.refraction_index(md, np.array(pool), wl)
    lines, ok = [], True
    for route, got in (("reference", g[f"n/{case}/ref"]), ("oracle", orc)):
        line, passes = wc.index_report(case, ri, wl, g, got, route)
        lines.append(line)
        ok &= passes
    with capsys.disabled():
        print("\n" + "\n".join(lines))
    assert ok, "\n".join(lines)
    assert wc.model_of(ri) in wc.BITWISE_MEDIA or wc.model_of(ri) in wc.POWER_MEDIA


def test_the_power_bound_bites():
    """One power off by one in Schott, or a dropped term, is far outside the bound; the bound itself is a few units of
    the last place."""
    ri = wc.medium(ot, "Schott")
    wl = wc.medium_wavelengths("Schott", ri)
    c = wc.coefficients(ri)
    bound = wc.power_bound("Schott", c, wl)
    um2 = (wl.astype(np.float64) * 1e-3) ** 2
    right = np.sqrt(c[0] + c[1] * um2 + c[2] / um2 + c[3] / um2 ** 2 + c[4] / um2 ** 3 + c[5] / um2 ** 4)
    wrong = np.sqrt(c[0] + c[1] * um2 + c[2] / um2 + c[3] / um2 ** 2 + c[4] / um2 ** 4 + c[5] / um2 ** 4)
    assert np.all(bound < 16 * 2.0 ** -53 * right) and np.all(np.abs(wrong - right) > 100 * bound)


@pytest.mark.parametrize("case", list(wc.FILTER_CASES))
def test_reference_and_oracle_transmissions_meet_the_bar(g, case, capsys):
    spec = wc.filter_spectrum(ot, case)
    wl = g[f"T/{case}/wl"]
    pool: list = []
    fd = spec._desc(pool, None)
    orc = ob.filter_T(fd, np.array(pool), wl)
    lines, ok = [], True
    for route, got in (("reference", g[f"T/{case}/ref"]), ("oracle", orc)):
        line, passes = wc.transmission_report(case, g, got, route)
        lines.append(line)
        ok &= passes
    if wc.FILTER_CASES[case][0]["spectrum_type"] != "Gaussian":
        ok &= bits(orc, g[f"T/{case}/ref"])   # the doubles, not only what a float32 weight shows of them
    with capsys.disabled():
        print("\n" + "\n".join(lines) + f"\n           the Gaussian bar: {wc.gaussian_bar(g)} float32 units (the reference: {int(g['gauss_ulp'])})")
    assert ok, "\n".join(lines)


def test_gaussian_underflows_where_the_reference_does(g):
    T = g["T/Gaussian5/ref"]
    assert np.count_nonzero(T == 0) >= 50 and np.count_nonzero((T > 0) & (T < 1e-30)) >= 1
    assert 2 <= wc.gaussian_bar(g) <= 3


def test_function_spectra_as_fine_tables_in_the_oracle():
    """A Function spectrum under a continuous source is the 65537-node table of wavelength_cases.function_table; the
    oracle's value is np.interp on it bit for bit, on nodes, next to them and between them, inverse folded in."""
    wl = wc.function_wavelengths()
    x = wl.astype(np.float64)
    grid = np.linspace(380.0, 780.0, wc.FUNCTION_GRID)
    assert np.count_nonzero(np.isin(x, grid)) >= 20 and np.count_nonzero(~np.isin(x, grid)) >= 150
    pool: list = []
    md = ot.RefractionIndex("Function", func=wc.index_function)._desc(pool)
    assert bits(np.array(pool[:wc.FUNCTION_GRID]), grid), "the table's nodes"
    assert bits(ob.refraction_index(md, np.array(pool), wl), np.interp(x, *wc.function_table(wc.index_function)))
    for inverse in (False, True):
        pool = []
        fd = ot.TransmissionSpectrum("Function", func=wc.transmission_function, inverse=inverse)._desc(pool, None)
        assert bits(ob.filter_T(fd, np.array(pool), wl), np.interp(x, *wc.function_table(wc.transmission_function, inverse)))
