"""CPU-side unit test of the launch chunking (optrace_amd/csrc/ot_host.hpp::for_ray_chunks): the same header the HIP
library compiles, its plain C++ part driven by tests/cpp/ray_chunks_test.cpp -- the callback sees contiguous, non-overlapping
pieces that cover [first, first + count), none longer than 2^28 rays, none at all for count == 0; counts 0, 1, 2^28 - 1, 2^28,
2^28 + 1 and 3 * 2^28 + 5, each from first = 0 and first = 63.  The trace, the index fill and the polarisation fill launch
through it, and no GPU test of sensible size reaches its second piece."""
import pathlib
import subprocess

ROOT = pathlib.Path(__file__).resolve().parent.parent


def test_ray_chunks_cover_the_range(tmp_path):
    exe = tmp_path / "ray_chunks_test"
    cmd = ["g++", "-std=c++17", "-O2", "-Wall", "-I", str(ROOT / "optrace_amd" / "csrc"),
           str(ROOT / "tests" / "cpp" / "ray_chunks_test.cpp"), "-o", str(exe)]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, (r.stdout + r.stderr)[-3000:]
    assert r.stdout.startswith("ok 12 cases")
