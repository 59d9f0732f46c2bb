"""Timing of the beam footprints ("Footprints") on the benchmark's double-Gauss scene at --rays rays.  Device events
around whole calls, median of --repeat after one warm-up, everything in one process:

  (a) `ot_footprint_moments` alone
  (b) `ot_footprint_maps` at --n-px cells a side
  (c) the whole `RT.footprints()`
  (d) the same records formed without the kernel: torch operations on the device planes, per section masked sums, amin and amax;
      checked to agree with (a) within the bounds of the tests before it is timed

and the bytes per second of (a) over the bytes it must read: per pass and ray-section 8 B of weights, plus 24 B of position for
every living ray, counted from the storage.
Needs a HIP device.  python tools/bench_footprints.py [--out file.json]
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
from optrace_amd._device import ptr, stream_ptr, require_device, to_dev  # noqa: E402
import scenes  # noqa: E402

HBM_PEAK = 8e12  # bytes per second, the MI355X's specification
EPS = np.finfo(np.float64).eps
M = _capi.FP_M


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


def by_torch(P, W, axis, with_mag: bool = False):
    """The records by torch operations.  P (3, nt, n) f64 and W (nt, n) f32: views of the planes; axis (nt, 2) on the device.
    -> records (nt, 17) on the device, and with `with_mag` the sums of the absolute values of the terms of every sum beside them."""
    nt = W.shape[0]
    rec = torch.zeros(nt, M, dtype=torch.float64, device=W.device)
    mag = torch.zeros_like(rec)
    inf = float("inf")
    for i in range(nt):
        wi, wa = W[i].double(), W[i - 1 if i else 0].double()
        alive, arriving = wi > 0, wa > 0
        wz = torch.where(alive, wi, 0.0)
        rec[i, 0], rec[i, 1] = wz.sum(), alive.sum()
        rec[i, 2], rec[i, 3] = torch.where(arriving, wa, 0.0).sum(), arriving.sum()
        pos = [torch.where(alive, P[c, i], 0.0) for c in range(3)]  # (a dead ray's position may be NaN)
        for c in range(3):
            rec[i, 4 + c] = (wz * pos[c]).sum()
            rec[i, 7 + 2 * c] = torch.where(alive, P[c, i], inf).amin()
            rec[i, 8 + 2 * c] = torch.where(alive, P[c, i], -inf).amax()
            if with_mag:
                mag[i, 4 + c] = (wz * pos[c].abs()).sum()
        dx = torch.where(alive, pos[0] - rec[i, 4] / rec[i, 0], 0.0)
        dy = torch.where(alive, pos[1] - rec[i, 5] / rec[i, 0], 0.0)
        rec[i, 13], rec[i, 14], rec[i, 15] = (wz * (dx * dx)).sum(), (wz * (dy * dy)).sum(), (wz * (dx * dy)).sum()
        ux, uy = pos[0] - axis[i, 0], pos[1] - axis[i, 1]
        rec[i, 16] = torch.where(alive, ux * ux + uy * uy, 0.0).amax()
        if with_mag:
            mag[i, 0], mag[i, 2], mag[i, 13], mag[i, 14] = rec[i, 0], rec[i, 2], rec[i, 13], rec[i, 14]
            mag[i, 15] = (wz * (dx * dy).abs()).sum()
    return (rec, mag) if with_mag else rec


def agree(rec, ref, mag) -> float:
    """Both routes within the bounds of the tests of the true values, so within twice that of each other (the second-pass sums
    about centroids a rounding apart: the bound of the centroid's own sums on top).  -> the largest share of a bound in use."""
    rec, ref, mag = (t.cpu().numpy() for t in (rec, ref, mag))
    alive = rec[:, 1] > 0
    assert np.array_equal(rec[:, [1, 3]], ref[:, [1, 3]]), "counts"
    assert np.array_equal(rec[alive, 7:13], ref[alive, 7:13]) and np.all(np.isnan(rec[~alive, 7:13])), "extremes"
    assert np.all(np.abs(rec[:, 16] - ref[:, 16]) <= 8 * EPS * ref[:, 16]), "largest squared radius"
    worst = 0.0
    for s in (0, 2, 4, 5, 6, 13, 14, 15):
        n = rec[:, 3 if s == 2 else 1]
        bound = 2 * (n + 40) * EPS * mag[:, s]
        if s >= 13:  # d(sum w dx^2) = 2 sum w |dx| dc <= 2 sqrt(W sum w dx^2) dc, dc within the first-pass bound over W
            dc = 2 * (n + 40) * EPS * np.maximum(mag[:, 4], mag[:, 5]) / np.maximum(rec[:, 0], 1e-300)
            bound = bound + 4 * np.sqrt(rec[:, 0] * np.maximum(mag[:, 13], mag[:, 14])) * dc
        err = np.abs(rec[:, s] - ref[:, s])
        assert np.all(err <= bound), f"slot {s}: {err} above {bound}"
        worst = max(worst, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))))
    return worst


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=10_000_000)
    ap.add_argument("--n-px", type=int, default=64)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = require_device()
    lib = _capi.load_library()
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=1)
        RT.trace(args.rays)
    rays = RT.rays
    n, nt, Np = int(rays.N), int(rays.Nt), int(rays._Np)
    R = rays._rays_struct()
    surfaces = RT.tracing_surfaces
    axis = np.array([RT.ray_sources[0].pos[:2]] + [s.pos[:2] for s in surfaces] + [[0.0, 0.0]], dtype=np.float64)
    d_axis = to_dev(axis, np.float64)
    ws = torch.empty(lib.ot_footprint_workspace(n, nt), dtype=torch.float64, device=dev)
    rec = torch.zeros(nt * M, dtype=torch.float64, device=dev)
    n_px = args.n_px
    maps = torch.zeros(nt * n_px * n_px, dtype=torch.float64, device=dev)
    st = stream_ptr()

    def moments():
        _capi.check(lib.ot_footprint_moments(C.byref(R), 0, n, ptr(d_axis), ptr(ws), ptr(rec), st))

    def power_maps():
        _capi.check(lib.ot_footprint_maps(C.byref(R), 0, n, ptr(d_axis), ptr(rec), n_px, ptr(maps), st))

    P = rays._dev["p"].view(3, nt, Np)[:, :, :n]
    W = rays._dev["w"].view(nt, Np)[:, :n]
    d_axis2 = d_axis.view(nt, 2)
    moments()
    ref, mag = by_torch(P, W, d_axis2, with_mag=True)
    share = agree(rec.view(nt, M), ref, mag)
    living = int(rec.view(nt, M)[:, 1].sum().item())
    must_read = 2 * (8 * n * nt + 24 * living)

    with ot.global_options.no_warnings():
        t_a = timed(moments, args.repeat)
        t_b = timed(power_maps, args.repeat)
        t_c = timed(lambda: RT.footprints(), args.repeat)
        t_d = timed(lambda: by_torch(P, W, d_axis2), args.repeat)
    row = dict(rays=n, sections=nt, living_ray_sections=living, n_px=n_px, moments_ms=t_a, maps_ms=t_b, footprints_ms=t_c, torch_ms=t_d,
               torch_over_moments=t_d / t_a, bytes_must_read=must_read, bytes_per_s=must_read / (t_a * 1e-3),
               share_of_hbm_peak=must_read / (t_a * 1e-3) / HBM_PEAK, torch_agreement_share_of_bound=share)
    print(json.dumps(row), flush=True)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps([row], indent=1) + "\n")


if __name__ == "__main__":
    main()
