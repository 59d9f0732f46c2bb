"""Times `Raytracer.wavefront_analysis` on the bench scene (double Gauss) and its passes one by one, with device events after a
warm-up call, and the host route (`rays.optical_lengths()` plus NumPy) for context.  Prints one JSON line.

    python tools/bench_wavefront.py [--rays 10000000] [--host-rays 1000000] [--repeat 7]
"""
import argparse
import ctypes as C
import json
import pathlib
import sys
import time

import numpy as np
import torch

ROOT = pathlib.Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]

import optrace_amd as ot  # noqa: E402
from optrace_amd import _capi  # noqa: E402
from optrace_amd._device import ptr, stream_ptr  # noqa: E402
import scenes  # noqa: E402


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


def passes(RT, source, repeat):
    """The entry points one by one, on the sphere the whole call finds."""
    lib, rays = _capi.load_library(), RT.rays
    first, end = (int(rays.B_list[source]), int(rays.B_list[source + 1])) if source is not None else (0, rays.N)
    count, k = end - first, rays.Nt - 2
    wa = RT.wavefront_analysis(source)
    dev, st, R = rays._dev["p"].device, stream_ptr(), rays._rays_struct()
    rays._dev["n"]
    d3 = C.c_double * 3
    ws = torch.empty(_capi.WF_WS, dtype=torch.float64, device=dev)
    sums = torch.zeros(_capi.WF_FOCUS_M, dtype=torch.float64, device=dev)
    u, v, opl = (torch.empty(count, dtype=torch.float64, device=dev) for _ in range(3))
    w = torch.empty(count, dtype=torch.float32, device=dev)
    missed = torch.zeros(1, dtype=torch.int64, device=dev)
    mom = torch.zeros(_capi.WF_M, dtype=torch.float64, device=dev)
    grid = torch.zeros(2 * 64 * 64, dtype=torch.float64, device=dev)
    big = torch.zeros(2 * 1024 * 1024, dtype=torch.float64, device=dev)
    zer = torch.zeros(36 * 37 // 2 + 36, dtype=torch.float64, device=dev)
    wl = rays._dev["wl"][first:end]
    origin, focus = d3(0, 0, float(wa.focus[2]) - abs(wa.radius)), d3(*wa.focus)
    nan = float("nan")
    t = {"rays": count, "used": wa.N, "section": k, "rms_waves": wa.rms_waves}
    t["focus"] = timed(lambda: lib.ot_wavefront_focus(C.byref(R), first, count, k, origin, ptr(ws), ptr(sums), st), repeat)
    t["paths"] = timed(lambda: lib.ot_wavefront_paths(C.byref(R), first, count, k, focus, wa.radius, ptr(u), ptr(v), ptr(opl), ptr(w),
                                                      ptr(missed), st), repeat)
    t["moments"] = timed(lambda: lib.ot_wavefront_moments(count, ptr(u), ptr(v), ptr(opl), ptr(w), ptr(wl), ptr(ws), ptr(mom), st), repeat)
    t["map_64"] = timed(lambda: lib.ot_wavefront_map(count, ptr(u), ptr(v), ptr(opl), ptr(w), ptr(mom), nan, 64, ptr(grid), st), repeat)
    t["map_1024"] = timed(lambda: lib.ot_wavefront_map(count, ptr(u), ptr(v), ptr(opl), ptr(w), ptr(mom), nan, 1024, ptr(big), st), repeat)
    for J in (15, 36):
        t[f"zernike_{J}"] = timed(lambda: lib.ot_wavefront_zernike(count, ptr(u), ptr(v), ptr(opl), ptr(w), ptr(mom), nan, J, ptr(ws),
                                                                   ptr(zer), st), repeat)
    t["whole_call"] = timed(lambda: RT.wavefront_analysis(source), repeat)
    t["whole_call_36"] = timed(lambda: RT.wavefront_analysis(source, n_zernike=36), repeat)
    # the hot pass against its algorithmic bytes
    read, written = (k + 2) * 24 + (k + 1) * 8 + 4, 28
    t["paths_GBps"] = count * (read + written) / t["paths"] * 1e-6  # every ray of the range counted in full
    # what the kernel asks for: a dead ray reads its weight and writes its four entries
    t["paths_GBps_requested"] = (wa.N * (read + written) + (count - wa.N) * (4 + written)) / t["paths"] * 1e-6
    return t


def host_route(RT, source):
    """The reference's way: whole planes to the host, then NumPy.  Seconds."""
    rays = RT.rays
    first, end = (int(rays.B_list[source]), int(rays.B_list[source + 1])) if source is not None else (0, rays.N)
    ch = np.zeros(rays.N, dtype=bool)
    ch[first:end] = True
    t0 = time.perf_counter()
    ol = rays.optical_lengths(ch)
    t1 = time.perf_counter()
    p, s, _, w, _, _, _ = rays.rays_by_mask(ch, ret=[1, 1, 0, 1, 0, 0, 0])
    t2 = time.perf_counter()
    k = rays.Nt - 2
    alive = w[:, k] > 0
    opl = ol[alive, :k].sum(axis=1)
    sk, pk, wk = s[alive, k], p[alive, k], w[alive, k].astype(np.float64)
    A = np.einsum("n,nij->ij", wk, np.eye(3) - sk[:, :, None] * sk[:, None, :])
    b = np.einsum("n,nij,nj->i", wk, np.eye(3) - sk[:, :, None] * sk[:, None, :], pk)
    c = np.linalg.solve(A, b)
    o = pk - c
    R = np.linalg.norm(c - (wk[:, None] * pk).sum(axis=0) / wk.sum())
    bb = (sk * o).sum(axis=1)
    tt = -bb - np.sqrt(bb * bb - ((o * o).sum(axis=1) - R * R))
    opl = opl + tt
    opd = opl - (wk * opl).sum() / wk.sum()
    rms = np.sqrt((wk * opd * opd).sum() / wk.sum())
    t3 = time.perf_counter()
    return {"rays": end - first, "optical_lengths_s": t1 - t0, "positions_directions_weights_s": t2 - t1, "numpy_s": t3 - t2, "rms": float(rms)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=10_000_000)
    ap.add_argument("--host-rays", type=int, default=1_000_000)
    ap.add_argument("--repeat", type=int, default=7)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0)}
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=1)
        RT.trace(args.rays)
        out["source_0"] = passes(RT, 0, args.repeat)
        out["all_rays"] = passes(RT, None, args.repeat)
        if args.host_rays:
            RT.trace(args.host_rays)
            out["host_route"] = host_route(RT, None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
