"""The C oracle (oracle/oracle.c) on the systems `ot.load_zmx` builds, against the reference's rays
(tests/golden/trace_zmx_*.npz, tests/golden/generate_golden_load.py), by the rules of tests/test_oracle_golden.py.  CPU only.
The loader builds the scene; the fixture supplies rays and expectations.  The largest position deviation measured here is
the yardstick for the tolerances of tests/test_gpu_load.py (ORACLE_DEVIATION there)."""
import numpy as np
import pytest

import optrace_amd as ot
from optrace_amd.scene import CompiledScene

import load_cases as lc
import oracle_bridge as ob
from helpers import load, assert_close


@pytest.mark.parametrize("fixture", list(lc.TRACE_FIXTURES))
def test_oracle_trace_of_loaded_system(fixture):
    system, no_pol = lc.TRACE_FIXTURES[fixture]
    g = load(f"trace_zmx_{fixture}.npz")
    with ot.global_options.no_warnings():
        RT = lc.traced_scene(ot, system, no_pol=no_pol)
        RT._geometry_checks()
    assert not RT.geometry_error
    sc = CompiledScene(RT)
    assert sc.nt == g["p_list"].shape[1]
    rays = ob.HostRays(int(g["N"]), sc.nt, no_pol)
    rays.set_initial(g["p0"], g["s0"], None if no_pol else g["pol0"], g["w0"], g["wl"])
    msgs, st = ob.trace(sc.desc, rays, None)
    assert st == 0
    assert np.array_equal(msgs, g["msgs"]), f"counters differ:\n{msgs}\n{g['msgs']}"
    assert np.array_equal(rays.w_list > 0, g["w_list"] > 0)
    print(f"{fixture}: {sc.nt} sections, oracle - reference: {np.abs(rays.p_list - g['p_list']).max():.3g} mm")
    assert_close(rays.p_list, g["p_list"], rtol=1e-12, atol=1e-12, what="p_list")
    assert_close(rays.n_list, g["n_list"], rtol=1e-14, what="n_list")
    assert_close(rays.w_list, g["w_list"], rtol=2e-7, atol=1e-30, what="w_list")
    assert_close(rays.s_final, g["s_final"], rtol=1e-11, atol=1e-13, what="s_final")
    if not no_pol:
        assert_close(rays.pol_list, g["pol_list"], rtol=1e-5, atol=2e-7, what="pol_list")


def test_objective_fixture_reaches_the_last_surface():
    g = load("trace_zmx_nikon60x.npz")
    assert g["p_list"].shape[1] == 78
    assert np.count_nonzero(g["w_list"][:, -2] > 0) >= 0.5 * int(g["N"])
