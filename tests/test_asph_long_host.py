"""Aspheres with more than OT_MAX_ASPH = 12 coefficients, the part that needs no device: the C header defines
OT_SURF_FLAG_ASPH_TABLE as a flag of its own, the ctypes binding carries the same value, `AsphericSurface._desc()` hands
the coefficients over through `tab` instead of refusing (and a 12-coefficient surface is described as it always was),
and the host-side bookkeeping of a long asphere (z range, flip(), the host copy of `values`) equals the reference's
(tests/golden/leaf_surfaces_asph_long.npz)."""
import ctypes as C
import pathlib
import subprocess

import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd import _capi

import scenes_asph_long as sal
from helpers import load, assert_close

ROOT = pathlib.Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "optrace_amd.h"


def test_header_defines_the_flag_apart_from_the_other_surface_flags(tmp_path):
    src = tmp_path / "flag.c"
    src.write_text(f'#include <stdio.h>\n#include <stddef.h>\n#include "{HEADER}"\n'
                   '#ifndef OT_SURF_FLAG_ASPH_TABLE\n#error "OT_SURF_FLAG_ASPH_TABLE is not defined"\n#endif\n'
                   'int main(){printf("asph %d\\nderiv %d\\nmask %d\\nmax %d\\nabi %d\\nsize %zu\\ncoeff %zu\\n", '
                   'OT_SURF_FLAG_ASPH_TABLE, OT_SURF_FLAG_DERIV_UNROTATED, OT_SURF_FLAG_MASK_TABLE, OT_MAX_ASPH, '
                   'OT_ABI_VERSION, sizeof(ot_surface), sizeof(((ot_surface*)0)->coeff));return 0;}')
    exe = tmp_path / "flag"
    subprocess.run(["gcc", "-Wall", "-Werror", str(src), "-o", str(exe)], check=True)
    out = {k: int(v) for k, v in (l.split() for l in subprocess.run([str(exe)], capture_output=True, text=True,
                                                                    check=True).stdout.splitlines())}
    flag = out["asph"]
    assert flag > 0 and flag & (flag - 1) == 0, "one bit"
    assert flag & out["deriv"] == 0 and flag & out["mask"] == 0, "a bit of its own"
    assert flag == _capi.SURF_FLAG_ASPH_TABLE
    assert out["deriv"] == _capi.SURF_FLAG_DERIV_UNROTATED and out["mask"] == _capi.SURF_FLAG_MASK_TABLE
    # additive: same ABI number, same struct, same inline array
    assert out["abi"] == _capi.ABI_VERSION == 9
    assert out["max"] == _capi.OT_MAX_ASPH == 12
    assert out["size"] == C.sizeof(_capi.Surface) and out["coeff"] == 12 * 8


def test_desc_of_a_long_asphere_carries_the_coefficients_in_tab():
    coeff = sal.long_coeff(3.0, 16)
    with ot.global_options.no_warnings():
        sf = ot.AsphericSurface(r=3.0, R=10.0, k=-0.8, coeff=coeff)
    d = sf._desc()
    assert d.kind == _capi.SURF_ASPHERE and d.ncoeff == 16
    assert d.flags & _capi.SURF_FLAG_ASPH_TABLE
    assert d.tab_len == 16 and bool(d.tab)
    assert [d.tab[j] for j in range(16)] == [float(c) for c in coeff]
    # the descriptor owns what it points to: flip() replaces the surface's array
    sf.flip()
    assert [d.tab[j] for j in range(16)] == [float(c) for c in coeff]
    d2 = sf._desc()
    assert [d2.tab[j] for j in range(16)] == [-float(c) for c in coeff] and d2.R == -10.0


def test_desc_of_a_twelve_coefficient_asphere_is_what_it_was():
    coeff = sal.long_coeff(2.5, 12, -1)
    with ot.global_options.no_warnings():
        sf = ot.AsphericSurface(r=2.5, R=-9.0, k=0.6, coeff=coeff)
        sf.move_to([0.1, -0.2, 3.0])
    d = sf._desc()
    # the descriptor as the code before the flag built it: base fields, R, k, ncoeff, inline coefficients, nothing else
    e = _capi.Surface()
    e.kind = _capi.SURF_ASPHERE
    e.pos[:] = [float(v) for v in sf.pos]
    e.r = float(sf.r)
    e.z_min, e.z_max = float(sf.z_min), float(sf.z_max)
    e.R, e.k = float(sf.R), float(sf.k)
    e.ncoeff = 12
    e.coeff[:12] = [float(c) for c in coeff]
    assert bytes(d) == bytes(e)
    assert d.flags == 0 and not d.tab and d.tab_len == 0


@pytest.fixture(scope="module")
def zoo():
    with ot.global_options.no_warnings():
        return sal.surface_zoo_long(ot)


@pytest.fixture(scope="module")
def leaf():
    return load("leaf_surfaces_asph_long.npz")


def test_fixture_is_what_the_issue_asks_for(leaf):
    assert [str(n) for n in leaf["names"]] == sal.NAMES
    counts = {name: leaf[f"{name}/param/coeff"].shape[0] for name in sal.NAMES}
    assert sorted(set(counts.values())) == [13, 16, 24, 32]
    assert leaf["asph_n13_last_zero/param/coeff"][-1] == 0.0
    for name in sal.NAMES:
        hit = leaf[f"{name}/is_hit"]
        assert hit.shape == (1500,) and leaf[f"{name}/x"].shape == (1500,)
        assert hit.sum() >= 375 and (~hit).sum() >= 150


@pytest.mark.parametrize("name", sal.NAMES)
def test_host_bookkeeping_equals_the_reference(zoo, leaf, name):
    """Parameters after construction, move_to and (one surface) flip(); the z range from the 10 000-sample estimate; the
    host copy of Surface.values (np.polyval over all coefficients) at all 1500 points."""
    sf = zoo[name]
    assert np.array_equal(np.asarray(sf.coeff), leaf[f"{name}/param/coeff"])
    assert float(sf.R) == float(leaf[f"{name}/param/R"]) and float(sf.k) == float(leaf[f"{name}/param/k"])
    assert np.array_equal(np.asarray(sf.pos, dtype=np.float64), leaf[f"{name}/param/pos"])
    assert_close(sf.z_min, leaf[f"{name}/param/z_min"], rtol=1e-14, atol=1e-15, what="z_min")
    assert_close(sf.z_max, leaf[f"{name}/param/z_max"], rtol=1e-14, atol=1e-15, what="z_max")
    x, y = leaf[f"{name}/x"], leaf[f"{name}/y"]
    assert np.array_equal(sf._mask_host(x, y), leaf[f"{name}/mask"])
    assert_close(sf._values_host(x, y), leaf[f"{name}/values"], rtol=1e-13, atol=1e-14, what=f"{name} host values")
