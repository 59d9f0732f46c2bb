"""Timing of the field analysis ("Field analysis") on the benchmark's double-Gauss scene with three of its sources (0, 10
and 20 degrees) at --rays rays, once with its three spectral lines as bands (K = 3) and once traced with a flat spectrum over
450 .. 650 nm cut into K = 32 equal bands.  Device events around whole calls, median of --repeat after one warm-up, everything in
one process.  Per K:

  (a) `ot_field_sums` alone (both passes, their last kernels and the finish), all three fields in the one call
  (b) the whole `RT.field_analysis()`
  (c) what there was before for the figures both have (power, centroid, spot size per field and band, a focus per band): a loop of
      `RT.chromatic_analysis(source_index=f)` over the three sources

and the bytes per second of (a) over the bytes it requests, which do not depend on the number of fields or bands: per pass 1 B of
key for every ray of a field; for a used ray of a band 4 B of weight and 48 B of positions, in the first pass 4 B of wavelength
besides.  (a) is checked against (c) before it is timed:
the rays and the power per field and band are those of the chromatic records.
Needs a HIP device.  python tools/bench_field.py [--out file.json]
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
from optrace_amd._device import ptr, stream_ptr, require_device  # noqa: E402
from optrace_amd.scene import SectionTable  # noqa: E402
import scenes  # noqa: E402

HBM_PEAK = 8e12  # bytes per second, the MI355X's specification
EPS = np.finfo(np.float64).eps
M = _capi.FIELD_M


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


def measure(RT, bands, repeat: int) -> dict:
    dev = require_device()
    lib = _capi.load_library()
    rays = RT.rays
    n, nt, Np = int(rays.N), int(rays.Nt), int(rays._Np)
    k = nt - 2
    F = len(RT.ray_sources)
    R = rays._rays_struct()
    st = stream_ptr()
    P = rays._dev["p"].view(3, nt, Np)[:, :, :n]
    w, wl = rays._dev["w"].view(nt, Np)[k, :n], rays._dev["wl"][:n]
    d2 = sum((P[c, k + 1] - P[c, k]) ** 2 for c in range(3))
    live = (w > 0) & (d2 > 0)
    key, K, table = _psf.assign_bands(wl, live, bands)
    if isinstance(bands, str):
        K = int(table[0].item())
    key8 = torch.where(key < K, key, _capi.CHROM_NO_BAND).to(torch.uint8)
    ranges = [(int(RT.rays.B_list[f]), int(RT.rays.B_list[f + 1] - RT.rays.B_list[f])) for f in range(F)]
    flat = (C.c_int64 * (2 * F))(*[v for pair in ranges for v in pair])
    origin = np.array(SectionTable(RT).origin(k, None), dtype=np.float64)
    ws = torch.empty(lib.ot_field_workspace(flat, F, K), dtype=torch.float64, device=dev)
    rec = torch.zeros(F * K * M, dtype=torch.float64, device=dev)

    def sums():
        _capi.check(lib.ot_field_sums(C.byref(R), flat, F, k, ptr(key8), 0, K, (C.c_double * 3)(*origin), ptr(ws), ptr(rec), st))

    sums()
    got = rec.cpu().numpy().reshape(F, K, M)
    with ot.global_options.no_warnings():
        fa = RT.field_analysis(bands=bands)
        loop = lambda: [RT.chromatic_analysis(source_index=f, bands=bands, z=fa.z) for f in range(F)]
        before = loop()
    assert fa.n_bands == K and np.array_equal(fa.records, got), "the analysis' records are the entry point's"
    if isinstance(bands, str):  # (a number of bands is cut over each source's own range of wavelengths by the loop: other bands)
        for f, ca in enumerate(before):
            assert np.array_equal(ca.band_N, got[f, :, 1]) and np.array_equal(ca.n_parallel, got[f, :, 7].sum())
            assert np.all(np.abs(ca.band_power - got[f, :, 0]) <= 2 * (got[f, :, 1] + 40) * EPS * got[f, :, 0])
            assert np.allclose(ca.centroid, fa.centroid[f], rtol=0, atol=1e-9) and np.allclose(ca.rms_radius, fa.rms_radius[f], rtol=1e-6, atol=1e-9)
    alive = int((key8 != _capi.CHROM_NO_BAND).sum().item())  # the used rays of a band: what the kernels read planes for
    requested = 2 * n + (56 + 52) * alive
    with ot.global_options.no_warnings():
        t_a = timed(sums, repeat)
        t_b = timed(lambda: RT.field_analysis(bands=bands), repeat)
        t_c = timed(loop, repeat)
    return dict(rays=n, fields=F, bands=K, rays_used=alive, rays_in_sums=int(got[:, :, 1].sum()), z=float(fa.z), field_sums_ms=t_a,
                field_analysis_ms=t_b, chromatic_loop_ms=t_c, loop_over_field_analysis=t_c / t_b, bytes_requested=requested,
                bytes_requested_per_used_ray=(requested - 2 * n) / alive, bytes_per_s=requested / (t_a * 1e-3),
                share_of_hbm_peak=requested / (t_a * 1e-3) / HBM_PEAK)


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=10_000_000)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    require_device()
    rows = []
    for bands, spectrum in (("lines", None), (32, ot.LightSpectrum("Rectangle", wl0=450., wl1=650.))):
        with ot.global_options.no_warnings():
            RT = scenes.double_gauss(ot, spectrum=spectrum, seed=1)
            for source in [RT.ray_sources[i] for i in (1, 3)]:  # three field points: 0, 10 and 20 degrees
                RT.remove(source)
            RT.trace(args.rays)
        rows.append(measure(RT, bands, args.repeat))
        print(json.dumps(rows[-1]), flush=True)
        del RT
        torch.cuda.empty_cache()
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
