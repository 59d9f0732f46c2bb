"""Timing of the wavefront across the field ("Wavefront across the field") on the benchmark's double-Gauss scene with
three of its sources (0, 10 and 20 degrees) at --rays rays and its three spectral lines as bands (K = 3).  Device events around
whole calls, median of --repeat after one warm-up, everything in one process.  At J = 15 and at J = 36:

  (a) every `ot_wavefield_*` entry alone, all three fields in the one call
  (b) the whole `RT.wavefront_field()`, and with bands=1 (one cell per field: the figures the loop of (c) gives)
  (c) what there was before: a loop of `RT.wavefront_analysis(source_index=f)` over the three sources, which has no band split

and the bytes per second of the paths pass over the bytes it requests -- 1 B of key for every ray of a field; for a ray with a band
4 B of weight, for a living one (k + 2) positions of 24 B and (k + 1) indices of 8 B; 28 B written for every ray of a field -- and
the f64 operations per second of the normal equations over the operations the definition asks for per counted entry:
J (J + 1) / 2 + J multiply-adds into the sums and J multiplies by the weight (the polynomials themselves, which the kernel forms
once per chunk of the triangle, are not counted).  (a) is checked before it is timed: the entry points' records are the
analysis'.  Needs a HIP device.  python tools/bench_wavefront_field.py [--out file.json]
"""
import argparse
import ctypes as C
import json
import pathlib
import sys

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]
import optrace_amd as ot  # noqa: E402
from optrace_amd import _capi  # noqa: E402
from optrace_amd import field as _field  # noqa: E402
from optrace_amd import wavefront_field as _wvf  # noqa: E402
from optrace_amd._device import ptr, stream_ptr, require_device  # noqa: E402
from optrace_amd.scene import SectionTable  # noqa: E402
import scenes  # noqa: E402

HBM_PEAK = 8e12  # bytes per second, the MI355X's specification
F64_PEAK = 78.6e12  # f64 vector operations per second, the MI355X's specification


def timed(fn, repeat: int) -> float:
    """Median of `repeat` device-event times of fn() in ms, after one warm-up."""
    fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(repeat):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        fn()
        t1.record()
        torch.cuda.synchronize()
        ms.append(t0.elapsed_time(t1))
    return float(np.median(ms))


def measure(RT, J: int, repeat: int) -> dict:
    dev = require_device()
    lib = _capi.load_library()
    rays = RT.rays
    n, nt = int(rays.N), int(rays.Nt)
    k = nt - 2
    F = len(RT.ray_sources)
    st = stream_ptr()
    ranges = [(int(rays.B_list[f]), int(rays.B_list[f + 1] - rays.B_list[f])) for f in range(F)]
    origin = np.array(SectionTable(RT).origin(k, None), dtype=np.float64)
    with ot.global_options.no_warnings():
        wf = RT.wavefront_field(n_zernike=J)
    front = _field.band_records(rays, ranges, k, origin, "lines", None)
    K, flat, key8, lo = front.K, front.flat, front.key8, front.lo
    assert K == wf.n_bands == 3 and lo == 0
    R = rays._rays_struct()
    rays._dev["n"]
    T = J * (J + 1) // 2 + J
    ws = torch.empty(lib.ot_wavefield_workspace(flat, F, K, J), dtype=torch.float64, device=dev)
    sums = torch.zeros(F * K * _capi.WF_FOCUS_M, dtype=torch.float64, device=dev)
    spheres = torch.as_tensor(np.concatenate([wf.focus, wf.radius[:, :, None]], axis=2).reshape(-1), device=dev)
    planes = torch.empty(3 * n, dtype=torch.float64, device=dev)
    u, v, opl = planes[:n], planes[n:2 * n], planes[2 * n:]
    w_out = torch.empty(n, dtype=torch.float32, device=dev)
    counts = torch.zeros(F * K * 2, dtype=torch.int64, device=dev)
    mom = torch.zeros(F * K * _capi.WFF_M, dtype=torch.float64, device=dev)
    pupil = torch.zeros(F * _capi.WFF_PUPIL_M, dtype=torch.float64, device=dev)
    out = torch.zeros(F * K * T, dtype=torch.float64, device=dev)
    wl = rays._dev["wl"][:n]
    d3 = (C.c_double * 3)(*origin)

    focus = lambda: _capi.check(lib.ot_wavefield_focus(C.byref(R), flat, F, k, ptr(key8), lo, K, d3, ptr(ws), ptr(sums), st))
    paths = lambda: _capi.check(lib.ot_wavefield_paths(C.byref(R), flat, F, k, ptr(key8), lo, K, ptr(spheres), ptr(u), ptr(v), ptr(opl),
                                                       ptr(w_out), ptr(counts), st))
    moments = lambda: _capi.check(lib.ot_wavefield_moments(flat, F, ptr(u), ptr(v), ptr(opl), ptr(w_out), ptr(wl), ptr(key8), lo, K,
                                                           ptr(ws), ptr(mom), ptr(pupil), st))
    zernike = lambda: _capi.check(lib.ot_wavefield_zernike(flat, F, ptr(u), ptr(v), ptr(opl), ptr(w_out), ptr(key8), lo, K, ptr(mom),
                                                           ptr(pupil), np.nan, J, ptr(ws), ptr(out), st))
    for fn in (focus, paths, moments, zernike):
        fn()
    assert np.array_equal(mom.cpu().numpy().reshape(F, K, -1), wf.moments) and np.array_equal(out.cpu().numpy().reshape(F, K, -1), wf.normal), \
        "the analysis' records are the entry points'"
    assert np.array_equal(_wvf.sphere_table(sums.cpu().numpy().reshape(F, K, -1), origin, "field", wf.reference_band)[:, :, 3], wf.radius)
    banded = int((key8 != _capi.CHROM_NO_BAND).sum().item())
    living = int((rays._dev["w"].view(nt, -1)[k, :n] > 0).sum().item())
    counted = int(wf.band_N.sum())
    paths_bytes = n + 4 * banded + (24 * (k + 2) + 8 * (k + 1)) * living + 28 * n
    fit_ops = counted * (2 * T + J)
    with ot.global_options.no_warnings():
        t = {name: timed(fn, repeat) for name, fn in (("focus", focus), ("paths", paths), ("moments", moments), ("zernike", zernike))}
        t_b = timed(lambda: RT.wavefront_field(n_zernike=J), repeat)
        t_b1 = timed(lambda: RT.wavefront_field(n_zernike=J, bands=1), repeat)
        t_c = timed(lambda: [RT.wavefront_analysis(source_index=f, n_zernike=J) for f in range(F)], repeat)
    return dict(rays=n, fields=F, bands=K, n_zernike=J, section=k, rays_banded=banded, rays_counted=counted,
                **{f"{name}_ms": ms for name, ms in t.items()}, wavefront_field_ms=t_b, wavefront_field_one_band_ms=t_b1,
                wavefront_analysis_loop_ms=t_c, loop_over_wavefront_field=t_c / t_b, loop_over_wavefront_field_one_band=t_c / t_b1,
                paths_bytes_requested=paths_bytes, paths_bytes_per_s=paths_bytes / (t["paths"] * 1e-3),
                paths_share_of_hbm_peak=paths_bytes / (t["paths"] * 1e-3) / HBM_PEAK, fit_f64_operations=fit_ops,
                fit_operations_per_s=fit_ops / (t["zernike"] * 1e-3), fit_share_of_f64_peak=fit_ops / (t["zernike"] * 1e-3) / F64_PEAK)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    require_device()
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=1)
        for source in [RT.ray_sources[i] for i in (1, 3)]:  # three field points: 0, 10 and 20 degrees
            RT.remove(source)
        RT.trace(args.rays)
    rows = []
    for J in (15, 36):
        rows.append(measure(RT, J, args.repeat))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
