"""bench.py's command line: a plain run times the headline only, `--full` adds the other measurements, and
`--dump-outputs DIR` writes what the last timed step computed -- the same arrays in every run with the same arguments."""
import json
import os
import pathlib
import subprocess
import sys

import numpy as np
import pytest

ROOT = pathlib.Path(__file__).resolve().parent.parent

FULL_ONLY = ("raw_kernel", "detector", "no_pol", "cpu_baseline", "configs", "c4_sharded", "c5_sharded")


def _env():
    return {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_PORT")}


def test_bench_options_and_step_count_check():
    """--full and --dump-outputs are options; a run without a timed step is refused before any GPU work."""
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--help"], env=_env(), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs" in r.stdout
    r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "0"], env=_env(), capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 2 and "--steps" in r.stderr, r.stderr


@pytest.mark.gpu
@pytest.mark.timeout(900)
def test_plain_bench_run_dumps_the_same_outputs_twice(tmp_path):
    outs = []
    for k in range(2):
        d = tmp_path / f"run{k}"
        r = subprocess.run([sys.executable, str(ROOT / "bench.py"), "--steps", "3", "--warmup", "2", "--rays", "1000000",
                            "--dump-outputs", str(d)], env=_env(), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
        lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
        assert len(lines) == 1
        line = json.loads(lines[0])
        assert line["metric"] == line["unit"] == "ray-surface-intersections/s" and line["higher_is_better"] is True
        assert line["dtype"] == "f64" and line["steps"] == 3 and line["value"] > 0 and line["ms_per_step"] > 0
        assert line["roofline"]["kernel_ms"] > 0
        assert not set(FULL_ONLY) & set(line), "a plain run measures the headline only"
        outs.append({f.stem: np.load(f) for f in sorted(d.glob("*.npy"))})
    a, b = outs
    base = {"msgs", "ray_index", "p", "s0", "pol", "w", "n", "wl"}
    assert base <= set(a) and set(a) == set(b)
    assert all(k[:-len("_nonfinite")] in base for k in set(a) - base), set(a) - base
    assert sum(v.nbytes for v in a.values()) <= 64 * 2 ** 20
    n, nt = a["ray_index"].shape[0], a["msgs"].shape[1]
    assert n == 32768 and a["p"].shape == (n, nt, 3) and a["w"].shape == (n, nt)
    for name in a:
        assert a[name].dtype in (np.float32, np.float64), name
        assert np.all(np.isfinite(a[name])), name
        assert np.array_equal(a[name], b[name]), name
    assert a["msgs"].sum() > 0 and a["w"][:, 0].max() > 0
    # direction and polarisation behind a total internal reflection are NaN: only on rays without power there
    if "pol_nonfinite" in a:
        bad = a["pol_nonfinite"].any(axis=2)
        assert np.all(a["w"][bad] == 0) and np.all(a["pol"][a["pol_nonfinite"] != 0] == 0)
    if "s0_nonfinite" in a:
        bad = a["s0_nonfinite"].any(axis=1)
        assert np.all(a["w"][bad, -1] == 0) and np.all(a["s0"][a["s0_nonfinite"] != 0] == 0)
