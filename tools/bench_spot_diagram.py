"""Timing of the spot diagram ("Spot diagrams") on the benchmark's double-Gauss scene with three of its sources (0, 10 and
20 degrees) at --rays rays each, its three spectral lines as bands, five planes over -0.2 .. 0.2 mm and 64 x 64 cells.  Device
events around whole calls, median of --repeat after one warm-up, everything in one process:

  (a) `ot_spotdiag_extent` alone, on the band centroids of the records of one `ot_field_sums`
  (b) `ot_spotdiag_maps` alone, at the default size (a) gives (one kernel launch; the outputs are accumulated into)
  (c) the whole `RT.spot_diagram()`
  (d) `ot_mtf_sums` for the same fields, bands and planes with eight frequencies, and (e) the whole `RT.mtf_analysis()`

with the bytes (a), (b) and (d) request, counted from the keys: every ray's key byte once per pass over the rays, and w (4 B) and
the two position planes (48 B) of the rays of the bands a workgroup takes.  (b) is checked before it is timed: no ray outside, and
the power of every tile is slot 0 of its record.
Needs a HIP device.  python tools/bench_spot_diagram.py [--out file.json]
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
from optrace_amd import spot_diagram as _sd  # noqa: E402
from optrace_amd._device import ptr, stream_ptr, require_device, to_dev  # noqa: E402
from optrace_amd.scene import SectionTable  # noqa: E402
import scenes  # noqa: E402

EPS = np.finfo(np.float64).eps
RAY_BYTES = 4 + 6 * 8  # w and the start of sections k and k + 1


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


def measure(RT, repeat: int, Z: int, Q: int, n_px: int) -> dict:
    dev = require_device()
    lib = _capi.load_library()
    k = int(RT.rays.Nt) - 2
    F = len(RT.ray_sources)
    st = stream_ptr()
    ranges = [(int(RT.rays.B_list[f]), int(RT.rays.B_list[f + 1] - RT.rays.B_list[f])) for f in range(F)]
    origin = np.array(SectionTable(RT).origin(k, None), dtype=np.float64)
    front = _field.band_records(RT.rays, ranges, k, origin, "lines", None)
    K = front.K
    with ot.global_options.no_warnings():
        fa = RT.field_analysis()
    z, in_sums = float(fa.z), int(fa.band_N.sum())
    dz = np.linspace(-0.2, 0.2, Z)
    zeta = z + dz - origin[2]
    org, c_zeta = (C.c_double * 3)(*origin), (C.c_double * Z)(*zeta)
    rel = np.full((F, K, Z, 2), np.nan)
    rel[:, front.keep] = _sd.centres(front.rec, zeta, "centroid", front.reference_band, origin[:2])
    d_centre = to_dev(rel.reshape(-1), np.float64)
    head = (C.byref(front.R), front.flat, F, k, ptr(front.key8), front.lo, K, org)

    ws = torch.empty(lib.ot_spotdiag_workspace(front.flat, F, K, Z), dtype=torch.float64, device=dev)
    d_ext = torch.zeros(F * K * Z * 2, dtype=torch.float64, device=dev)
    extent = lambda: _capi.check(lib.ot_spotdiag_extent(*head, ptr(d_centre), c_zeta, Z, ptr(ws), ptr(d_ext), st))
    extent()
    size = _sd.SIZE_FACTOR * float(np.sqrt(d_ext.cpu().numpy().reshape(F, K, Z, 2)[..., 0].max()))
    cells = F * K * Z * n_px * n_px
    d_maps = torch.zeros(cells, dtype=torch.float64, device=dev)
    d_counts = torch.zeros(F * K * Z * 2, dtype=torch.int64, device=dev)
    d_out = torch.zeros(F * K * Z, dtype=torch.float64, device=dev)
    maps = lambda: _capi.check(lib.ot_spotdiag_maps(*head, ptr(d_centre), c_zeta, Z, n_px, size, ptr(d_maps), ptr(d_counts), ptr(d_out), st))
    maps()
    counts, power = d_counts.cpu().numpy().reshape(F, K, Z, 2), d_maps.cpu().numpy().reshape(F, K, Z, -1).sum(axis=-1)
    W, N = fa.band_power[:, :, None], fa.band_N[:, :, None]
    assert np.all(counts[..., 1] == 0) and np.all(counts[..., 0] == N), "no ray outside at the default size"
    assert np.all(np.abs(power - W) <= (N + 40) * EPS * W), "the power of a tile is slot 0 of its record"

    freq = np.linspace(0, 50, Q)
    t = _field.directions(fa.field)
    ws_m = torch.empty(lib.ot_mtf_workspace(front.flat, F, K, Z, Q), dtype=torch.float64, device=dev)
    d_sums = torch.zeros(F * K * Z * Q * 4, dtype=torch.float64, device=dev)
    d_freq = to_dev(freq, np.float64)
    mtf = lambda: _capi.check(lib.ot_mtf_sums(*head, ptr(front.d_rec), (C.c_double * (2 * F))(*t.reshape(-1)), c_zeta, Z, ptr(d_freq), Q,
                                              ptr(ws_m), ptr(d_sums), st))
    with ot.global_options.no_warnings():
        t_a, t_b, t_d = timed(extent, repeat), timed(maps, repeat), timed(mtf, repeat)
        t_c = timed(lambda: RT.spot_diagram(dz=dz, z=z, n_px=n_px), repeat)
        t_e = timed(lambda: RT.mtf_analysis(dz=dz, z=z, frequencies=freq), repeat)

    # bytes requested, from the keys: passes over the rays, and the passes that take a band's rays
    n_all = sum(n for _, n in ranges)
    per_band = torch.bincount(front.key8.to(torch.int64), minlength=256)[:K].cpu().numpy()
    KB = min(K, 4)
    tile = 3 if KB == 3 else 8 // KB
    passes_extent = -(-K // KB) * -(-Z // tile)
    takes_extent = np.full(K, -(-Z // tile))
    chunks = lib.ot_spotdiag_chunks(K, Z, n_px)
    T = min(_capi.SD_LDS_BYTES // (8 * n_px * n_px + 40), K * Z) or K * Z
    takes_maps = np.array([len({t_ // T for t_ in range(b * Z, (b + 1) * Z)}) for b in range(K)])
    tile_m = 3 if KB == 3 else 8 // KB
    passes_mtf = -(-K // KB) * -(-Z * Q // tile_m)
    bytes_of = lambda passes, takes: int(passes * n_all + RAY_BYTES * int((per_band * takes).sum()))
    once = bytes_of(1, np.ones(K))
    row = dict(case="spot_diagram", rays=n_all, fields=F, bands=K, planes=Z, n_px=n_px, size=size, rays_in_sums=in_sums, z=z,
               chunks=int(chunks), tiles_per_chunk=int(T),
               extent_ms=t_a, maps_ms=t_b, spot_diagram_ms=t_c, frequencies=Q, mtf_sums_ms=t_d, mtf_analysis_ms=t_e,
               maps_over_mtf_sums=t_b / t_d, extent_over_mtf_sums=t_a / t_d,
               bytes_once=once, extent_bytes=bytes_of(passes_extent, takes_extent), maps_bytes=bytes_of(chunks, takes_maps),
               mtf_bytes=bytes_of(passes_mtf, np.full(K, -(-Z * Q // tile_m))))
    for name in ("extent", "maps", "mtf"):
        ms = {"extent": t_a, "maps": t_b, "mtf": t_d}[name]
        row[f"{name}_GB_per_s"] = row[f"{name}_bytes"] / (ms * 1e-3) / 1e9
    row["mtf_ms_per_ray_read"] = t_d / passes_mtf
    row["maps_ms_per_chunk"] = t_b / chunks
    return row


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=10_000_000, help="per field")
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--planes", type=int, default=5)
    ap.add_argument("--frequencies", type=int, default=8)
    ap.add_argument("--n-px", type=int, default=64)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    require_device()
    with ot.global_options.no_warnings():
        RT = scenes.double_gauss(ot, seed=1)
        for source in [RT.ray_sources[i] for i in (1, 3)]:  # three field points: 0, 10 and 20 degrees
            RT.remove(source)
        RT.trace(3 * args.rays)
    row = measure(RT, args.repeat, args.planes, args.frequencies, args.n_px)
    print(json.dumps(row), flush=True)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(row, indent=1) + "\n")


if __name__ == "__main__":
    main()
