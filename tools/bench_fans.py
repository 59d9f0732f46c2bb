"""Timing of the ray fans ("Ray fans") on the benchmark's double-Gauss scene at --rays rays, once with its three
spectral lines as bands (K = 3) and once traced with a flat spectrum over 450 .. 650 nm cut into K = 32 equal bands.  Device events
around whole calls, median of --repeat after one warm-up, everything in one process.  Per K, on the same traced bundle:

  (a) the whole `RT.ray_fans(source)`
  (b) the whole `RT.wavefront_analysis(source)`, a yardstick: the same sphere stage, a Zernike fit and a pupil map behind it
  (c) the whole `RT.chromatic_analysis(source)`, a yardstick: the same bands, two passes over the stored positions per plane
  (d) `ot_fans_transverse`, `ot_fans_bands` and `ot_fans_bins` alone, on the planes of the sphere stage of (a)

Needs a HIP device.  python tools/bench_fans.py [--out file.json]
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
from optrace_amd import psf as _psf  # noqa: E402
from optrace_amd import wavefront as _wavefront  # noqa: E402
from optrace_amd._device import ptr, stream_ptr, require_device  # noqa: E402
from optrace_amd.scene import SectionTable  # noqa: E402
import scenes  # noqa: E402


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


def measure(RT, source, bands, n_bins: int, slab: float, repeat: int) -> dict:
    dev = require_device()
    lib = _capi.load_library()
    rays = RT.rays
    first, end = (0, int(rays.N)) if source is None else (int(rays.B_list[source]), int(rays.B_list[source + 1]))
    count, k = end - first, int(rays.Nt) - 2
    st = stream_ptr()
    with ot.global_options.no_warnings():
        a = RT.ray_fans(source, bands=bands, n_bins=n_bins, slab=slab)
        # the planes of (a)'s sphere stage, for the entry points alone
        origin = SectionTable(RT).origin(k, source)
        S = _wavefront.sphere_stage(rays, first, count, k, origin, a.focus, a.radius, 0)
    K = a.n_bands
    planes = torch.empty(2 * count, dtype=torch.float64, device=dev)
    ex, ey = planes[:count], planes[count:]
    par = torch.zeros(1, dtype=torch.int64, device=dev)
    focus = (C.c_double * 3)(*a.focus)

    def transverse():
        _capi.check(lib.ot_fans_transverse(C.byref(S.R), first, count, k, focus, ptr(S.w), ptr(ex), ptr(ey), ptr(par), st))

    transverse()
    key, K_set, _ = _psf.assign_bands(S.wl, S.w > 0, bands)
    key8 = torch.where(key < K, key, _capi.CHROM_NO_BAND).to(torch.uint8)
    ws = torch.empty(lib.ot_fans_workspace(count, K), dtype=torch.float64, device=dev)
    rec = torch.zeros(K * _capi.FAN_M, dtype=torch.float64, device=dev)
    out = torch.zeros(K * 2 * n_bins * _capi.FAN_BIN_M, dtype=torch.float64, device=dev)

    def band_records():
        _capi.check(lib.ot_fans_bands(count, ptr(S.opl), ptr(ex), ptr(ey), ptr(S.w), ptr(S.wl), ptr(key8), K, ptr(ws), ptr(rec), st))

    def bins():
        _capi.check(lib.ot_fans_bins(count, ptr(S.u), ptr(S.v), ptr(S.opl), ptr(ex), ptr(ey), ptr(S.w), ptr(key8), ptr(S.mom), np.nan,
                                     ptr(rec), K, n_bins, slab, ptr(out), st))

    band_records()
    bins()
    got = out.cpu().numpy().reshape(K, 2, n_bins, _capi.FAN_BIN_M)
    assert np.array_equal(rec.cpu().numpy().reshape(K, -1), a.records) and np.array_equal(got[..., 1], a.count), "not the planes of (a)"
    with ot.global_options.no_warnings():
        t_fans = timed(lambda: RT.ray_fans(source, bands=bands, n_bins=n_bins, slab=slab), repeat)
        t_wave = timed(lambda: RT.wavefront_analysis(source), repeat)
        t_chrom = timed(lambda: RT.chromatic_analysis(source, bands=bands), repeat)
        t_tr, t_rec, t_bins = timed(transverse, repeat), timed(band_records, repeat), timed(bins, repeat)
    in_cuts = a.count.sum(axis=(0, 2))
    return dict(rays=count, rays_used=a.N, bands=K, n_bins=n_bins, slab=slab, rays_in_cuts=[int(c) for c in in_cuts],
                share_in_cuts=float(in_cuts.sum() / max(2 * a.N, 1)), lds_path=bool(K * 2 * n_bins * _capi.FAN_BIN_M * 8 <= 64 * 1024),
                ray_fans_ms=t_fans, wavefront_analysis_ms=t_wave, chromatic_analysis_ms=t_chrom, transverse_ms=t_tr, bands_ms=t_rec,
                bins_ms=t_bins)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--source", type=int, default=0)
    ap.add_argument("--bins", type=int, default=32)
    ap.add_argument("--slab", type=float, default=0.1)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    require_device()
    rows = []
    for bands, spectrum in (("lines", None), (32, ot.LightSpectrum("Rectangle", wl0=450., wl1=650.))):
        with ot.global_options.no_warnings():
            RT = scenes.double_gauss(ot, spectrum=spectrum, seed=1)
            RT.trace(args.rays)
        rows.append(measure(RT, args.source, bands, args.bins, args.slab, args.repeat))
        print(json.dumps(rows[-1]), flush=True)
        del RT
        torch.cuda.empty_cache()
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
