"""Timing of the chromatic analysis ("Chromatic analysis") on the benchmark's double-Gauss scene at --rays rays, once
with its three spectral lines as bands (K = 3) and once traced with a flat spectrum over 450 .. 650 nm cut into K = 32 equal bands.
Device events around whole calls, median of --repeat after one warm-up, everything in one process.  Per K:

  (a) `ot_chromatic_focus` alone
  (b) `ot_chromatic_plane` alone (both passes, their last kernels and the finish)
  (c) the whole `RT.chromatic_analysis(None)` with the plane defaulted: two reads of the device
  (d) the same sums and records formed without the kernels: torch masked sums per band on the device planes; checked to agree
      with (a) and (b) within the bounds of the tests before it is timed

and the bytes per second of (a) and (b) over the bytes they request: per band and pass 1 B of key for every ray; for a ray of
the band 4 B of weight and 48 B of positions, in the first plane pass 4 B of wavelength besides.  What the memory system moves
is more: a band's rays lie among the others', so most 128-byte lines of the planes are pulled once per band.
Needs a HIP device.  python tools/bench_chromatic.py [--out file.json]
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
import scenes  # noqa: E402

HBM_PEAK = 8e12  # bytes per second, the MI355X's specification
EPS = np.finfo(np.float64).eps
M, FM = _capi.CHROM_M, _capi.WF_FOCUS_M


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


def by_torch(p0, p1, w, wl, key, K, origin, z0, with_mag: bool = False):
    """Focus sums (K, 17) and records (K, 10) by torch operations.  p0, p1: the three planes each of the section's start and end
    (f64 views), w f32, wl f32, key int64 (K: no band), origin (3,) and z0 host numbers.  With `with_mag` the sums of the absolute
    values of the elementary terms of every sum beside them."""
    dev = w.device
    d = [p1[c] - p0[c] for c in range(3)]
    L = torch.sqrt(d[0] * d[0] + d[1] * d[1] + d[2] * d[2])
    used = (w > 0) & (L > 0)
    zero = torch.zeros((), dtype=torch.float64, device=dev)
    wd = torch.where(used, w.double(), zero)
    s = [torch.where(used, d[c] / L, zero) for c in range(3)]
    q = [torch.where(used, p0[c] - origin[c], zero) for c in range(3)]
    sp = s[0] * q[0] + s[1] * q[1] + s[2] * q[2]
    asp = (s[0] * q[0]).abs() + (s[1] * q[1]).abs() + (s[2] * q[2]).abs()
    cross = used & (d[2] != 0)
    t = torch.where(cross, (z0 - p0[2]) / d[2], zero)
    x = torch.where(cross, p0[0] + t * d[0], zero)
    y = torch.where(cross, p0[1] + t * d[1], zero)
    wc = torch.where(cross, wd, zero)
    lam = wl.double()
    sums, rec = torch.zeros(K, FM, dtype=torch.float64, device=dev), torch.zeros(K, M, dtype=torch.float64, device=dev)
    smag, rmag = torch.zeros_like(sums), torch.zeros_like(rec)
    pairs = [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    for b in range(K):
        mine = key == b
        wb, wcb = torch.where(mine, wd, zero), torch.where(mine, wc, zero)
        sums[b, 0], sums[b, 1] = wb.sum(), (mine & used).sum()
        for c in range(3):
            sums[b, 2 + c], sums[b, 5 + c] = (wb * q[c]).sum(), (wb * s[c]).sum()
            sums[b, 14 + c] = (wb * (q[c] - s[c] * sp)).sum()
        for j, (a, c) in enumerate(pairs):
            sums[b, 8 + j] = (wb * ((1.0 if a == c else 0.0) - s[a] * s[c])).sum()
        rec[b, 0], rec[b, 1], rec[b, 9] = wcb.sum(), (mine & cross).sum(), (mine & used & ~cross).sum()
        rec[b, 2], rec[b, 3], rec[b, 4] = (wcb * x).sum(), (wcb * y).sum(), (wcb * lam).sum()
        dx = torch.where(mine & cross, x - rec[b, 2] / rec[b, 0], zero)
        dy = torch.where(mine & cross, y - rec[b, 3] / rec[b, 0], zero)
        rec[b, 5], rec[b, 6], rec[b, 7] = (wcb * (dx * dx)).sum(), (wcb * (dy * dy)).sum(), (wcb * (dx * dy)).sum()
        rec[b, 8] = (dx * dx + dy * dy).amax()
        if with_mag:
            smag[b, 0], smag[b, 1] = sums[b, 0], sums[b, 1]
            for c in range(3):
                smag[b, 2 + c], smag[b, 5 + c] = (wb * q[c].abs()).sum(), (wb * s[c].abs()).sum()
                smag[b, 14 + c] = (wb * (q[c].abs() + s[c].abs() * asp)).sum()
            for j, (a, c) in enumerate(pairs):
                smag[b, 8 + j] = (wb * ((1.0 if a == c else 0.0) + (s[a] * s[c]).abs())).sum()
            rmag[b, 0], rmag[b, 4], rmag[b, 5], rmag[b, 6] = rec[b, 0], rec[b, 4], rec[b, 5], rec[b, 6]
            rmag[b, 2], rmag[b, 3], rmag[b, 7] = (wcb * x.abs()).sum(), (wcb * y.abs()).sum(), (wcb * (dx * dy).abs()).sum()
    return (sums, rec, smag, rmag) if with_mag else (sums, rec)


def agree(sums, rec, tsums, trec, smag, rmag) -> float:
    """Both routes within the bounds of the tests of the true values, so within twice that of each other (the second-pass sums
    about centroids a rounding apart: the bound of the centroid's own sums on top).  -> the largest share of a bound in use."""
    sums, rec, tsums, trec, smag, rmag = (t.cpu().numpy() for t in (sums, rec, tsums, trec, smag, rmag))
    assert np.array_equal(sums[:, 1], tsums[:, 1]) and np.array_equal(rec[:, [1, 9]], trec[:, [1, 9]]), "counts"
    worst = 0.0
    n = sums[:, 1:2]
    bound = 2 * (n + 40) * EPS * smag
    err = np.abs(sums - tsums)
    assert np.all(err <= bound), f"focus sums: {(err - bound).max()} above the bound"
    worst = max(worst, float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1), 0))))
    n = rec[:, 1]
    some = n > 0
    # the two centroids lie within the first-pass bound over W of the truth each: dc apart at the most, per coordinate
    dc = 2 * (n + 40) * EPS * np.maximum(rmag[:, 2], rmag[:, 3]) / np.maximum(rec[:, 0], 1e-300)
    # d(dx^2 + dy^2) <= 2 (|dx| + |dy|) dc <= 2 sqrt(2 r^2) dc, beside the 4 eps of each route
    r2_bound = 8 * EPS * trec[:, 8] + 2 * np.sqrt(2 * trec[:, 8]) * dc + 2 * dc * dc
    assert np.all(np.abs(rec[some, 8] - trec[some, 8]) <= r2_bound[some]), "largest squared radius"
    for s in (0, 2, 3, 4, 5, 6, 7):
        bound = 2 * (n + 40) * EPS * rmag[:, s]
        if s >= 5:  # d(sum w dx^2) = 2 sum w |dx| dc <= 2 sqrt(W sum w dx^2) dc
            bound = bound + 4 * np.sqrt(rec[:, 0] * np.maximum(rmag[:, 5], rmag[:, 6])) * dc
        err = np.abs(rec[some, s] - trec[some, s])
        assert np.all(err <= bound[some]), f"slot {s}: {err} above {bound[some]}"
        worst = max(worst, float(np.max(np.where(bound[some] > 0, err / np.where(bound[some] > 0, bound[some], 1), 0), initial=0.0)))
    return worst


def measure(RT, bands, repeat: int) -> dict:
    dev = require_device()
    lib = _capi.load_library()
    rays = RT.rays
    n, nt, Np = int(rays.N), int(rays.Nt), int(rays._Np)
    k = nt - 2
    R = rays._rays_struct()
    st = stream_ptr()
    P = rays._dev["p"].view(3, nt, Np)[:, :, :n]
    w, wl = rays._dev["w"].view(nt, Np)[k, :n], rays._dev["wl"][:n]
    p0, p1 = [P[c, k] for c in range(3)], [P[c, k + 1] for c in range(3)]
    d2 = (p1[0] - p0[0]) ** 2 + (p1[1] - p0[1]) ** 2 + (p1[2] - p0[2]) ** 2
    live = (w > 0) & (d2 > 0)
    key, K, table = _psf.assign_bands(wl, live, bands)
    if isinstance(bands, str):
        K = int(table[0].item())
    key = torch.where(key < K, key, K)
    key8 = torch.where(key < K, key, _capi.CHROM_NO_BAND).to(torch.uint8)
    origin = np.array(RT.tracing_surfaces[k - 1].pos, dtype=np.float64)
    ws = torch.empty(lib.ot_chromatic_workspace(n, K), dtype=torch.float64, device=dev)
    sums = torch.zeros(K * FM, dtype=torch.float64, device=dev)
    rec = torch.zeros(K * M, dtype=torch.float64, device=dev)

    def focus():
        _capi.check(lib.ot_chromatic_focus(C.byref(R), 0, n, k, ptr(key8), K, (C.c_double * 3)(*origin), ptr(ws), ptr(sums), st))

    with ot.global_options.no_warnings():
        z0 = float(RT.chromatic_analysis(None, bands=bands).z)

    def plane():
        _capi.check(lib.ot_chromatic_plane(C.byref(R), 0, n, k, ptr(key8), K, z0, ptr(ws), ptr(rec), st))

    focus()
    plane()
    tsums, trec, smag, rmag = by_torch(p0, p1, w, wl, key, K, origin, z0, with_mag=True)
    share = agree(sums.view(K, FM), rec.view(K, M), tsums, trec, smag, rmag)
    in_bands = int(sums.view(K, FM)[:, 1].sum().item())
    focus_bytes = K * n + 52 * in_bands
    plane_bytes = 2 * (K * n + 52 * in_bands) + 4 * in_bands
    with ot.global_options.no_warnings():
        t_a = timed(focus, repeat)
        t_b = timed(plane, repeat)
        t_c = timed(lambda: RT.chromatic_analysis(None, bands=bands), repeat)
        t_d = timed(lambda: by_torch(p0, p1, w, wl, key, K, origin, z0), repeat)
    return dict(rays=n, bands=K, rays_in_bands=in_bands, z=z0, focus_ms=t_a, plane_ms=t_b, chromatic_analysis_ms=t_c, torch_ms=t_d,
                torch_over_kernels=t_d / (t_a + t_b), focus_bytes_requested=focus_bytes, plane_bytes_requested=plane_bytes,
                focus_bytes_per_s=focus_bytes / (t_a * 1e-3), plane_bytes_per_s=plane_bytes / (t_b * 1e-3),
                focus_share_of_hbm_peak=focus_bytes / (t_a * 1e-3) / HBM_PEAK, plane_share_of_hbm_peak=plane_bytes / (t_b * 1e-3) / HBM_PEAK,
                torch_agreement_share_of_bound=share)


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
