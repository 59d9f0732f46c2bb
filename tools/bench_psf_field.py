"""Times `ot_psf_field_sum` on the five field points of the bench scene (double Gauss, spectral lines F, d, C): five fields x three
bands ("lines") x the planes in one launch, against the same sums as a loop of `ot_psf_stack` calls on the per-field slices of the
same grouped records -- what there was before the field call --; device events, seven samples after one warm-up call, both in
one process.  Then the whole `Raytracer.huygens_field` call.  Prints one JSON line.

    python tools/bench_psf_field.py [--rays 5000000] [--cases 64:21 128:5] [--span 0.05] [--repeat 7]

`--rays` is the whole trace; the scene's five sources share it evenly.  `--cases`: n_px:planes; the planes run from -span to +span
mm about each field's focus.  The f64 rate is that of tools/bench_psf.py: 53.5 f64 vector instructions per ray and image point
against 3.9e13 / s.  Beside the ratio of the medians stands the loop's own spread over its samples, (max - min) / median.
"""
import argparse
import ctypes as C
import json
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests"), str(ROOT / "tools")]

import optrace_amd as ot  # noqa: E402
from optrace_amd import _capi  # noqa: E402
from optrace_amd import psf_field as pf  # noqa: E402
from optrace_amd._device import ptr, stream_ptr  # noqa: E402
from bench_psf import F64_PEAK, F64_PER_RAY_POINT  # noqa: E402
import scenes  # noqa: E402


def samples(fn, repeat):
    """Milliseconds of fn() between two device events, `repeat` times after one warm-up call."""
    fn()
    out = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def grouped_records(RT, dz):
    """The grouped records, cell starts and radii that `psf_field.analyse` hands to the sum, taken from one small call."""
    seen = {}
    inner = pf.call_sum

    def keep(grouped, starts, radius, F, K, n_px, size, dz, field, sums):
        seen.update(grouped=grouped, starts=np.array(starts), radius=np.array(radius), F=F, K=K, size=size)
        inner(grouped, starts, radius, F, K, n_px, size, dz, field, sums)

    pf.call_sum = keep
    try:
        RT.huygens_field(n_px=8, dz=dz)
    finally:
        pf.call_sum = inner
    return seen


def passes(RT, n_px, dz, repeat):
    lib, st_ = _capi.load_library(), stream_ptr()
    g = grouped_records(RT, dz)
    grouped, starts, radius, F, K, size = g["grouped"], g["starts"], g["radius"], g["F"], g["K"], g["size"]
    n, Z, px, cells, dev = int(starts[-1]), len(dz), n_px * n_px, F * K, grouped.device
    c_dz = (C.c_double * Z)(*dz.tolist())
    ws = torch.empty(_capi.psf_field_ws(n, F, K, n_px, Z), dtype=torch.float64, device=dev)
    table = torch.empty(_capi.psf_field_table(cells), dtype=torch.int64, device=dev)
    field = torch.zeros(F * Z * K * 2 * px, dtype=torch.float64, device=dev)
    sums = torch.zeros(F * Z * K * 5, dtype=torch.float64, device=dev)
    c_starts, c_radius = (C.c_int64 * (cells + 1))(*starts.tolist()), (C.c_double * F)(*radius.tolist())

    def launch():
        _capi.check(lib.ot_psf_field_sum(n, ptr(grouped), F, K, c_starts, c_radius, n_px, size, Z, c_dz, ptr(table), ptr(ws), ptr(field),
                                         ptr(sums), st_))

    own = [starts[f * K:(f + 1) * K + 1] - starts[f * K] for f in range(F)]
    slices = [grouped.view(6, n)[:, starts[f * K]:starts[(f + 1) * K]].contiguous().view(-1) for f in range(F)]
    ws1 = [torch.empty(_capi.psf_stack_ws(int(o[-1]), K, n_px, Z), dtype=torch.float64, device=dev) for o in own]
    field1 = torch.zeros(F * Z * K * 2 * px, dtype=torch.float64, device=dev)
    sums1 = torch.zeros(F * Z * K * 5, dtype=torch.float64, device=dev)
    c_own = [(C.c_int64 * (K + 1))(*o.tolist()) for o in own]

    def loop():
        for f in range(F):
            _capi.check(lib.ot_psf_stack(int(own[f][-1]), ptr(slices[f]), K, c_own[f], float(radius[f]), n_px, size, Z, c_dz, ptr(ws1[f]),
                                         ptr(field1[f * Z * K * 2 * px:]), ptr(sums1[f * Z * K * 5:]), st_))

    t_launch, t_loop = samples(launch, repeat), samples(loop, repeat)
    pairs = n * (px + 1) * Z
    spread = lambda t: (max(t) - min(t)) / float(np.median(t))

    def rate(t):
        ms = float(np.median(t))
        return {"ms": ms, "samples_ms": t, "spread": spread(t), "ray_points_per_s": pairs / ms * 1e3,
                "f64_rate_of_peak": pairs * F64_PER_RAY_POINT / (ms * 1e-3) / F64_PEAK}

    scale = float(sums.view(F, Z, K, 5)[:, 0, :, 2].max())
    whole = samples(lambda: RT.huygens_field(n_px=n_px, dz=dz), repeat)
    return {"used": n, "fields": F, "bands": K, "planes": Z, "cell_N": np.diff(starts).tolist(), "size": size, "radius": radius.tolist(),
            "launch": rate(t_launch), "loop_of_ot_psf_stack": rate(t_loop),
            "launch_over_loop": float(np.median(t_launch)) / float(np.median(t_loop)), "loop_spread": spread(t_loop),
            "largest_difference_in_A": float((field - field1).abs().max()) / scale, "whole_call_ms": float(np.median(whole))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=5_000_000)
    ap.add_argument("--cases", nargs="+", default=["64:21", "128:5"])
    ap.add_argument("--span", type=float, default=0.05)
    ap.add_argument("--repeat", type=int, default=7)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "rays": args.rays}
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=1)
        RT.trace(args.rays)
        for case in args.cases:
            n_px, planes = (int(v) for v in case.split(":"))
            out[f"n_px_{n_px}_planes_{planes}"] = passes(RT, n_px, np.linspace(-args.span, args.span, planes), args.repeat)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
