"""Timing of the MTF analysis ("MTF analysis") on the benchmark's double-Gauss scene with three of its sources (0, 10 and
20 degrees) at --rays rays and its three spectral lines as bands, at (K, Z, Q) = (3, 1, 2), (3, 5, 8) and (3, 9, 64).  Device events
around whole calls, median of --repeat after one warm-up, everything in one process.  Per shape:

  (a) `ot_mtf_sums` alone, all fields, bands, planes and frequencies in the one call, on the records of one `ot_field_sums`
  (b) the whole `RT.mtf_analysis()`
  (c) the route there was before: a loop of `RT.spot_analysis(frequencies=)` over the sources and the planes with the detector
      moved to each plane -- which gives the x and y axes, not t and s, and no bands

and once (d) `ot_spot_otf` with 64 frequencies on as many points as (a) has rays in its sums (where they cross the plane z), the
yardstick for the rate of sine-cosine pairs: (a) forms 2 Z Q pairs per ray in the sums, (d) 2 * 64 per point.
(a) is checked before it is timed: the column of nu = 0 is the power of the records.
Needs a HIP device.  python tools/bench_mtf.py [--out file.json]
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
from optrace_amd._device import ptr, stream_ptr, require_device, to_dev  # noqa: E402
from optrace_amd.scene import SectionTable  # noqa: E402
import scenes  # noqa: E402

EPS = np.finfo(np.float64).eps
SHAPES = [(1, 2), (5, 8), (9, 64)]  # (Z, Q)


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


def spot_otf_yardstick(RT, front, z: float, repeat: int) -> dict:
    """(d): `ot_spot_otf` at 64 frequencies on the points where the rays in the sums of `front` cross the plane z."""
    dev = require_device()
    lib = _capi.load_library()
    rays = RT.rays
    n, nt, Np = int(rays.N), int(rays.Nt), int(rays._Np)
    k = nt - 2
    P = rays._dev["p"].view(3, nt, Np)[:, :, :n]
    w = rays._dev["w"].view(nt, Np)[k, :n]
    dz = P[2, k + 1] - P[2, k]
    inside = (front.key8[:n] != _capi.CHROM_NO_BAND) & (dz != 0)
    s = ((z - P[2, k]) / dz)[inside]
    x = (P[0, k][inside] + s * (P[0, k + 1] - P[0, k])[inside]).contiguous()
    y = (P[1, k][inside] + s * (P[1, k + 1] - P[1, k])[inside]).contiguous()
    wi = w[inside].contiguous()
    m = int(x.shape[0])
    K = 64
    ws = torch.empty(_capi.spot_ws(K), dtype=torch.float64, device=dev)
    mom = torch.zeros(_capi.SPOT_M, dtype=torch.float64, device=dev)
    otf = torch.zeros(4 * K, dtype=torch.float64, device=dev)
    st = stream_ptr()
    _capi.check(lib.ot_spot_moments(m, None, ptr(x), ptr(y), ptr(wi), ptr(ws), ptr(mom), st))
    freq = to_dev(np.linspace(0, 50, K), np.float64)
    t = timed(lambda: _capi.check(lib.ot_spot_otf(m, None, ptr(x), ptr(y), ptr(wi), ptr(mom), ptr(freq), K, ptr(ws), ptr(otf), st)), repeat)
    return dict(points=m, frequencies=K, spot_otf_ms=t, pairs_per_s=2.0 * K * m / (t * 1e-3))


def measure(RT, repeat: int) -> list:
    dev = require_device()
    lib = _capi.load_library()
    nt = int(RT.rays.Nt)
    k = nt - 2
    F = len(RT.ray_sources)
    st = stream_ptr()
    ranges = [(int(RT.rays.B_list[f]), int(RT.rays.B_list[f + 1] - RT.rays.B_list[f])) for f in range(F)]
    origin = np.array(SectionTable(RT).origin(k, None), dtype=np.float64)
    front = _field.band_records(RT.rays, ranges, k, origin, "lines", None)
    K = front.K
    with ot.global_options.no_warnings():
        fa = RT.field_analysis()
    z, in_sums = float(fa.z), int(fa.band_N.sum())
    t = _field.directions(fa.field)
    rows = [dict(case="spot_otf_yardstick", **spot_otf_yardstick(RT, front, z, repeat))]
    yard = rows[0]["pairs_per_s"]
    detector_z = float(RT.detectors[0].pos[2])
    for Z, Q in SHAPES:
        dz = np.linspace(-0.2, 0.2, Z) if Z > 1 else np.zeros(1)
        freq = np.linspace(0, 50, Q)
        zeta = z + dz - origin[2]
        ws = torch.empty(lib.ot_mtf_workspace(front.flat, F, K, Z, Q), dtype=torch.float64, device=dev)
        out = torch.zeros(F * K * Z * Q * 4, dtype=torch.float64, device=dev)
        d_freq = to_dev(freq, np.float64)

        def sums():
            _capi.check(lib.ot_mtf_sums(C.byref(front.R), front.flat, F, k, ptr(front.key8), front.lo, K, (C.c_double * 3)(*origin),
                                        ptr(front.d_rec), (C.c_double * (2 * F))(*t.reshape(-1)), (C.c_double * Z)(*zeta), Z,
                                        ptr(d_freq), Q, ptr(ws), ptr(out), st))

        sums()
        got = out.cpu().numpy().reshape(F, K, Z, Q, 4)
        W, N = fa.band_power[:, :, None], fa.band_N[:, :, None]
        assert np.all(np.abs(got[:, :, :, 0, 0] - W) <= (N + 40) * EPS * W), "the column of nu = 0 is the power of the records"
        analysis = lambda: RT.mtf_analysis(dz=dz, frequencies=freq, z=z)

        def loop():
            res = []
            for f in range(F):
                for off in dz:
                    RT.detectors[0].move_to([0, 0, z + off])
                    res.append(RT.spot_analysis(0, f, frequencies=freq))
            return res

        with ot.global_options.no_warnings():
            assert np.array_equal(analysis().sums, got), "the analysis' sums are the entry point's"
            t_a, t_b, t_c = timed(sums, repeat), timed(analysis, repeat), timed(loop, repeat)
            RT.detectors[0].move_to([0, 0, detector_z])
        pairs = 2.0 * Z * Q * in_sums
        rows.append(dict(case="mtf", rays=int(RT.rays.N), fields=F, bands=K, planes=Z, frequencies=Q, rays_in_sums=in_sums, z=z,
                         mtf_sums_ms=t_a, mtf_analysis_ms=t_b, spot_loop_ms=t_c, loop_over_mtf_analysis=t_c / t_b,
                         pairs_per_s=pairs / (t_a * 1e-3), share_of_spot_otf_rate=pairs / (t_a * 1e-3) / yard))
        print(json.dumps(rows[-1]), flush=True)
    return rows


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
    rows = measure(RT, args.repeat)
    print(json.dumps(rows[0]), flush=True)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
