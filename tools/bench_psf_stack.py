"""Times `ot_psf_stack` on source 0 of the bench scene (double Gauss, spectral lines F, d, C): three bands ("lines") x 21 planes in
one launch, against the same 63 sums as a loop of `ot_psf_sum` calls on the band slices; device events, median after one warm-up
call, both in one process.  Then `Raytracer.huygens_stack` for the scene's five field points.  Prints one JSON line.

    python tools/bench_psf_stack.py [--rays 5000000] [--n-px 64 128] [--planes 21] [--span 0.05] [--repeat 7]

`--rays` is the whole trace; the scene's five sources share it evenly.  `--span`: the planes run from -span to +span mm about the
focus.  The f64 rate is that of tools/bench_psf.py: 53.5 f64 vector instructions per ray and image point against 3.9e13 / s.
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
from optrace_amd import psf as hp  # noqa: E402
from optrace_amd import wavefront  # noqa: E402
from optrace_amd._device import ptr, stream_ptr  # noqa: E402
from bench_psf import F64_PEAK, F64_PER_RAY_POINT, timed  # noqa: E402
import scenes  # noqa: E402


def grouped_records(RT, source, st):
    """The grouped records of the source's rays for the sphere of `st`, as `psf.analyse_stack` forms them.  -> (grouped, starts)"""
    lib, rays = _capi.load_library(), RT.rays
    first, end = int(rays.B_list[source]), int(rays.B_list[source + 1])
    count = end - first
    S = wavefront.sphere_stage(rays, first, count, st.section, np.zeros(3), st.focus, st.radius, 0)
    rec = torch.empty(6 * count, dtype=torch.float64, device=S.w.device)
    _capi.check(lib.ot_psf_rays(C.byref(S.R), first, count, st.section, (C.c_double * 3)(*st.focus), st.radius, ptr(S.opl), ptr(S.mom),
                                ptr(rec), stream_ptr()))
    key, K, table = hp.assign_bands(S.wl, rec[5 * count:] != 0, "lines")
    grouped, starts, table, _ = hp.group_records(rec, count, key, K, table)
    K, starts, _ = hp.settle_bands("lines", K, starts, table)
    return grouped, starts


def passes(RT, source, sizes, dz, repeat):
    lib, st_ = _capi.load_library(), stream_ptr()
    first = RT.huygens_stack(source, n_px=8, dz=dz)
    grouped, starts = grouped_records(RT, source, first)
    n, K, Z = int(starts[-1]), len(starts) - 1, len(dz)
    dev = grouped.device
    slices = [grouped.view(6, n)[:, starts[b]:starts[b + 1]].contiguous().view(-1) for b in range(K)]
    t = {"used": n, "bands": K, "band_N": np.diff(starts).tolist(), "planes": Z, "radius": first.radius, "size": first.size}
    c_starts, c_dz = (C.c_int64 * (K + 1))(*starts.tolist()), (C.c_double * Z)(*dz.tolist())
    for n_px in sizes:
        px = n_px * n_px
        ws = torch.empty(_capi.psf_stack_ws(n, K, n_px, Z), dtype=torch.float64, device=dev)
        field = torch.zeros(Z * K * 2 * px, dtype=torch.float64, device=dev)
        sums = torch.zeros(Z * K * 5, dtype=torch.float64, device=dev)

        def stack():
            _capi.check(lib.ot_psf_stack(n, ptr(grouped), K, c_starts, first.radius, n_px, first.size, Z, c_dz, ptr(ws), ptr(field),
                                         ptr(sums), st_))

        ws1 = [torch.empty(_capi.psf_ws(s.shape[0] // 6, n_px), dtype=torch.float64, device=dev) for s in slices]
        field1 = torch.zeros(Z * K * 2 * px, dtype=torch.float64, device=dev)
        centre1 = torch.zeros(Z * K * 4, dtype=torch.float64, device=dev)

        def loop():
            for z in range(Z):
                for b in range(K):
                    i = z * K + b
                    _capi.check(lib.ot_psf_sum(slices[b].shape[0] // 6, ptr(slices[b]), first.radius, n_px, first.size, float(dz[z]),
                                               ptr(ws1[b]), ptr(field1[i * 2 * px:]), ptr(centre1[i * 4:]), st_))

        ms_stack, ms_loop = timed(stack, repeat), timed(loop, repeat)
        pairs = n * (px + 1) * Z
        rate = lambda ms: {"ms": ms, "ray_points_per_s": pairs / ms * 1e3, "f64_rate_of_peak": pairs * F64_PER_RAY_POINT / (ms * 1e-3) / F64_PEAK}
        scale = float(sums.view(Z, K, 5)[0, :, 2].max())
        t[f"n_px_{n_px}"] = {"stack": rate(ms_stack), "loop_of_ot_psf_sum": rate(ms_loop), "stack_over_loop": ms_stack / ms_loop,
                             "largest_difference_in_A": float((field - field1).abs().max()) / scale}
    return t


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=5_000_000)
    ap.add_argument("--n-px", type=int, nargs="+", default=[64, 128])
    ap.add_argument("--planes", type=int, default=21)
    ap.add_argument("--span", type=float, default=0.05)
    ap.add_argument("--repeat", type=int, default=7)
    args = ap.parse_args()
    dz = np.linspace(-args.span, args.span, args.planes)
    out = {"device": torch.cuda.get_device_name(0), "dz": dz.tolist()}
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=1)
        RT.trace(args.rays)
        out["source_0"] = passes(RT, 0, args.n_px, dz, args.repeat)
        out["field_points"] = []
        for source in range(len(RT.ray_sources)):
            st = RT.huygens_stack(source, n_px=64, dz=dz)
            out["field_points"].append({"source": source, "N": st.N, "band_wavelength": st.band_wavelength.tolist(),
                                        "band_weight": st.band_weight.tolist(), "strehl_at_focus": float(st.strehl[args.planes // 2]),
                                        "strehl_best": float(st.strehl.max()), "best_focus": st.best_focus,
                                        "band_best_focus": [float(dz[int(np.argmax(st.band_strehl[:, b]))]) for b in range(st.band_N.shape[0])],
                                        "noise_floor": st.noise_floor, "mtf_x_at_50_100_200": st.mtf(int(np.argmax(st.strehl)), 5, 200.0).mtf_x[[1, 2, 4]].tolist()})
    print(json.dumps(out))


if __name__ == "__main__":
    main()
