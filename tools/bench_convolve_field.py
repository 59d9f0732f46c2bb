"""Timing of the field-dependent convolution ("Field-dependent convolution"): an RGB image of --size pixels a side on a
--grid x --grid grid of PSFs of --psf pixels a side at the image's pitch.  Device events around whole calls, median of --repeat
after one warm-up, everything in one process:

  (a) `ot_convolve_field` alone
  (b) the whole `ot.convolve_field` call
  (c) the same sum by FFTs, as it could be formed without the kernel: per node the masked image planes W[b][a] I and the node's
      PSF through real FFTs of convolve's padded length, their products added up in the spectrum, one inverse transform per
      channel; checked to agree with (a) to 1e-9 before it is timed
  (d) one `ot.convolve` of the same image with one PSF, for scale

and the multiply-adds of the definition per second of (a): per channel, source pixel and node with W > 0, py x px of them.
Needs a HIP device.  python tools/bench_convolve_field.py [--out file.json]
"""
import argparse
import json
import pathlib
import sys

import numpy as np
import torch

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import optrace_amd as ot  # noqa: E402
from optrace_amd import _capi  # noqa: E402
from optrace_amd._device import ptr, stream_ptr, require_device  # noqa: E402
from optrace_amd.convolve import _fast_len  # noqa: E402

F64_PEAK_FMA = 78.6e12 / 2  # vector f64 peak of the MI355X in fused multiply-adds per second


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


def hat_weights(n: int, G: int, dev) -> torch.Tensor:
    t = torch.arange(n, dtype=torch.float64, device=dev) / (n - 1) * (G - 1)
    return (1 - (t[None, :] - torch.arange(G, dtype=torch.float64, device=dev)[:, None]).abs()).clamp_(min=0)


def blob(pn: int, b: int, a: int, G: int) -> np.ndarray:
    yy, xx = np.mgrid[0:pn, 0:pn]
    c = (pn - 1) / 2
    r2 = (xx - c - 0.04 * pn * (a - G // 2)) ** 2 + (yy - c - 0.04 * pn * (b - G // 2)) ** 2
    v = np.exp(-r2 / (0.01 * pn * pn * (1 + 0.3 * (a + b))))
    return v / v.max()


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1000)
    ap.add_argument("--grid", type=int, default=5)
    ap.add_argument("--psf", type=int, nargs="+", default=[64, 256])
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    dev = require_device()
    lib = _capi.load_library()
    N, G = args.size, args.grid
    rng = np.random.default_rng(3)
    data = rng.uniform(0.0, 1.0, (N, N, 3))
    img_s = [1.0, 1.0]
    img = ot.RGBImage(data, img_s)
    from optrace_amd.image import srgb_to_srgb_linear
    d_img = torch.from_numpy(np.ascontiguousarray(np.moveaxis(srgb_to_srgb_linear(data), 2, 0))).to(dev)
    wy, wx = hat_weights(N, G, dev), hat_weights(N, G, dev)
    pairs = int(sum(int((wy[b] > 0).sum()) * int((wx[a] > 0).sum()) for b in range(G) for a in range(G)))
    rows = []
    for pn in args.psf:
        psf_s = [(pn - 1) / (N - 1)] * 2  # the image's pitch
        psfs = [[ot.GrayscaleImage(blob(pn, b, a, G), psf_s) for a in range(G)] for b in range(G)]
        lin = np.stack([np.stack([srgb_to_srgb_linear(p.data) for p in row]) for row in psfs])
        d_psf = torch.from_numpy(lin / lin.sum(axis=(2, 3), keepdims=True)).to(dev)
        out = torch.empty(3, N + pn - 1, N + pn - 1, dtype=torch.float64, device=dev)

        def kernel():
            _capi.check(lib.ot_convolve_field(ptr(d_img), 3, N, N, 0, 0, N, N, ptr(d_psf), G, G, pn, pn, ptr(out), stream_ptr()))

        L = _fast_len(N + pn - 1)

        def by_fft():
            spec = torch.zeros(3, L, L // 2 + 1, dtype=torch.complex128, device=dev)
            for b in range(G):
                for a in range(G):
                    w = wy[b][:, None] * wx[a][None, :]
                    spec += torch.fft.rfft2(d_img * w[None], s=(L, L)) * torch.fft.rfft2(d_psf[b, a], s=(L, L))[None]
            return torch.fft.irfft2(spec, s=(L, L))[:, :N + pn - 1, :N + pn - 1]

        kernel()
        dev_ab = float((by_fft() - out).abs().max())
        assert dev_ab <= 1e-9, dev_ab
        with ot.global_options.no_warnings():
            t_a = timed(kernel, args.repeat)
            t_b = timed(lambda: ot.convolve_field(img, psfs), args.repeat)
            t_c = timed(by_fft, args.repeat)
            t_d = timed(lambda: ot.convolve(img, psfs[G // 2][G // 2]), args.repeat)
        fma = 3 * pairs * pn * pn
        rows.append(dict(size=N, grid=G, psf=pn, kernel_ms=t_a, convolve_field_ms=t_b, fft_ms=t_c, convolve_ms=t_d, kernel_minus_fft=dev_ab,
                         multiply_adds=fma, multiply_adds_per_s=fma / (t_a * 1e-3), share_of_f64_peak=fma / (t_a * 1e-3) / F64_PEAK_FMA))
        print(json.dumps(rows[-1]), flush=True)
    if args.out:
        pathlib.Path(args.out).parent.mkdir(parents=True, exist_ok=True)
        pathlib.Path(args.out).write_text(json.dumps(rows, indent=1) + "\n")


if __name__ == "__main__":
    main()
