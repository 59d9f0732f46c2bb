"""Times `Raytracer.huygens_psf` on source 0 of the bench scene (double Gauss): `ot_psf_rays` and `ot_psf_sum` one by one at
several image sizes, with device events after a warm-up call, the whole call, and as a yardstick the same sum written with torch
complex operations in ray chunks on the same device.  Prints one JSON line.

    python tools/bench_psf.py [--rays 5000000] [--n-px 64 128 256] [--repeat 7] [--torch-repeat 3]

`--rays` is the whole trace; the scene's five sources share it evenly.  `f64_per_ray_point` is the count of f64 vector
instructions in the inner loop of `psf_sum_kernel` per ray and image point, read from the ISA ("Huygens PSF"); the
rate it gives is set against the 3.9e13 / s peak of the f64 vector pipe.
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
from optrace_amd._device import ptr, stream_ptr  # noqa: E402
import scenes  # noqa: E402

F64_PER_RAY_POINT = 53.5  # 214 f64 vector instructions per ray in the loop that serves four points per lane
F64_PEAK = 3.9e13         # f64 vector instructions x lanes per second: 256 CUs x 64 lanes x 2.4 GHz


def timed(fn, repeat):
    """Median milliseconds of fn() between two device events, after one warm-up call."""
    fn()
    out = []
    for _ in range(repeat):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return float(np.median(out))


def torch_sum(rec, radius, n_px, size, dz, budget=2 ** 25):
    """The definition with torch operations: chunks of rays against all image points, `budget` complex numbers at a time.
    -> field (n_px * n_px,) complex128"""
    n = rec.shape[0] // 6
    qx, qy, qz, tau0, kappa, a = (rec[i * n:(i + 1) * n] for i in range(6))
    ax, sg = abs(radius), 1.0 if radius > 0 else -1.0
    c = (torch.arange(n_px, dtype=torch.float64, device=rec.device) + 0.5 - n_px / 2) * (size / n_px)
    dx, dy = c.repeat(n_px)[:, None], c.repeat_interleave(n_px)[:, None]  # (P, 1): column from x, row from y
    dd = dx * dx + dy * dy + dz * dz
    U = torch.zeros(n_px * n_px, dtype=torch.complex128, device=rec.device)
    step = max(1, budget // (n_px * n_px))
    for s in range(0, n, step):
        e = slice(s, s + step)
        num = dd - 2 * ax * (dx * qx[e] + dy * qy[e] + dz * qz[e])
        dist = torch.sqrt((dx - ax * qx[e]) ** 2 + (dy - ax * qy[e]) ** 2 + (dz - ax * qz[e]) ** 2)
        tau = tau0[e] + sg * kappa[e] * (num / (dist + ax))
        tau = tau - torch.round(tau)
        U += (torch.polar(a[e].expand_as(tau), 2 * torch.pi * tau)).sum(dim=1)
    return U


def passes(RT, source, sizes, repeat, torch_repeat):
    lib, rays = _capi.load_library(), RT.rays
    first, end = int(rays.B_list[source]), int(rays.B_list[source + 1])
    count, k = end - first, rays.Nt - 2
    psf = RT.huygens_psf(source, n_px=8)
    dev, st, R = rays._dev["p"].device, stream_ptr(), rays._rays_struct()
    rays._dev["n"]
    d3 = C.c_double * 3
    ws = torch.empty(_capi.WF_WS, dtype=torch.float64, device=dev)
    u, v, opl = (torch.empty(count, dtype=torch.float64, device=dev) for _ in range(3))
    w = torch.empty(count, dtype=torch.float32, device=dev)
    missed = torch.zeros(1, dtype=torch.int64, device=dev)
    mom = torch.zeros(_capi.WF_M, dtype=torch.float64, device=dev)
    rec = torch.empty(6 * count, dtype=torch.float64, device=dev)
    wl = rays._dev["wl"][first:end]
    focus = d3(*psf.focus)
    lib.ot_wavefront_paths(C.byref(R), first, count, k, focus, psf.radius, ptr(u), ptr(v), ptr(opl), ptr(w), ptr(missed), st)
    lib.ot_wavefront_moments(count, ptr(u), ptr(v), ptr(opl), ptr(w), ptr(wl), ptr(ws), ptr(mom), st)
    t = {"rays": count, "used": psf.N, "section": k, "radius": psf.radius, "size": psf.size, "strehl": psf.strehl,
         "noise_floor": psf.noise_floor}
    t["rays_ms"] = timed(lambda: lib.ot_psf_rays(C.byref(R), first, count, k, focus, psf.radius, ptr(opl), ptr(mom), ptr(rec), st), repeat)
    for n_px in sizes:
        pws = torch.empty(_capi.psf_ws(count, n_px), dtype=torch.float64, device=dev)
        out = torch.zeros(2 * n_px * n_px + 4, dtype=torch.float64, device=dev)
        field, centre = out[:-4], out[-4:]
        ms = timed(lambda: lib.ot_psf_sum(count, ptr(rec), psf.radius, n_px, psf.size, 0.0, ptr(pws), ptr(field), ptr(centre), st), repeat)
        pairs = count * (n_px * n_px + 1)
        e = {"sum_ms": ms, "ray_points_per_s": pairs / ms * 1e3, "f64_per_ray_point": F64_PER_RAY_POINT,
             "f64_rate_of_peak": pairs * F64_PER_RAY_POINT / (ms * 1e-3) / F64_PEAK,
             "whole_call_ms": timed(lambda: RT.huygens_psf(source, n_px=n_px), repeat)}
        if torch_repeat:
            e["torch_ms"] = timed(lambda: torch_sum(rec, psf.radius, n_px, psf.size, 0.0), torch_repeat)
            U = torch_sum(rec, psf.radius, n_px, psf.size, 0.0)
            ref = torch.complex(field[:n_px * n_px], field[n_px * n_px:])
            e["torch_largest_difference"] = float((U - ref).abs().max() / centre[2])  # in units of A = sum a
            e["torch_over_kernel"] = e["torch_ms"] / ms
        t[f"n_px_{n_px}"] = e
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=5_000_000)
    ap.add_argument("--n-px", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--torch-repeat", type=int, default=3)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=1)
        RT.trace(args.rays)
        out["source_0"] = passes(RT, 0, args.n_px, args.repeat, args.torch_repeat)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
