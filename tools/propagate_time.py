#!/usr/bin/env python
"""Time a focus series (libtike.hipfft.propagate, ptycho_propagate) against the same series written in torch.

4 fields x 64 distances at S = 128 and S = 256, figures only and with planes; at 128 both the one-launch path and the
same call with the handle's "tile" option off (the two-pass path every larger side takes).  Each native call is one
ptycho_propagate on a ready spectrum, timed between two events over --reps calls after a warm-up; the torch series is
the transfer-function route a user would write (one ifft2 over all planes, |.|^2, the seven reductions), with H built
once outside the timed region, which favours torch: the native call evaluates H in float64 inside the timed region.
Appends to --out (profiles/r15/propagate.txt).

    python tools/propagate_time.py [--sizes 128 256] [--fields 4] [--planes 64] [--out profiles/r15/propagate.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "libtike-cufft_amd"))

from libtike.hipfft import _native as nat  # noqa: E402
from libtike.hipfft.operators import PtychoHIP, _ptr, _stream  # noqa: E402

LAM, PIX = 0.05, 1.0


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def torch_series(spec, H, want_planes):
    """planes [F, D, S, S] = ifft2(spec H) and the eight figures per plane, as torch reductions."""
    S = spec.shape[-1]
    planes = torch.fft.ifft2(spec[:, None] * H[None], norm="forward")
    v = (planes.real * planes.real + planes.imag * planes.imag).double()
    y = torch.arange(S, dtype=torch.float64, device=v.device)
    flat = v.reshape(v.shape[0], v.shape[1], -1)
    top, idx = flat.max(dim=-1)
    rows, cols = v.sum(dim=-1), v.sum(dim=-2)
    met = torch.stack((flat.sum(-1), (flat * flat).sum(-1), (rows * y).sum(-1), (cols * y).sum(-1),
                       (rows * y * y).sum(-1), (cols * y * y).sum(-1), top, idx.double()), dim=-1)
    return (planes if want_planes else None), met


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[128, 256])
    ap.add_argument("--fields", type=int, default=4)
    ap.add_argument("--planes", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r15", "propagate.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    nf, nd = args.fields, args.planes
    gen = torch.Generator(device="cuda").manual_seed(1)
    with open(args.out, "a") as out:
        out.write("# tools/propagate_time.py on %s: %d fields x %d distances, per call, %d calls after a warm-up\n"
                  % (torch.cuda.get_device_name(0), nf, nd, args.reps))
        for S in args.sizes:
            u = torch.randn((nf, S, S, 2), generator=gen, device="cuda")
            u = torch.view_as_complex(u.contiguous())
            z = np.linspace(-0.6, 0.6, nd) * S * PIX ** 2 / LAM
            q0 = (LAM / (S * PIX)) ** 2
            k = np.fft.fftfreq(S) * S
            t = -0.5 * (z / LAM)[:, None, None] * q0 * (k[:, None] ** 2 + k[None, :] ** 2)[None]
            H = torch.as_tensor(np.exp(2j * np.pi * (t - np.rint(t))) / (S * S), device="cuda").to(torch.complex64)
            zl = torch.as_tensor(z / LAM, dtype=torch.float64, device="cuda")
            planes = torch.empty((nf, nd, S, S), dtype=torch.complex64, device="cuda")
            met = torch.empty((nf, nd, nat.PROPAGATE_WORDS), dtype=torch.float64, device="cuda")
            results = {}
            with PtychoHIP(nf, S, S, 1, S + 2, S + 2) as op:
                spec = op.fft2(u)
                for tile in ((True, False) if S <= 128 else (True,)):
                    op.set_tile(tile)
                    for want in (False, True):
                        words = int(nat.propagate_work_words(op._h, nf, nd, int(want)))
                        work = torch.empty(max(words, 2), dtype=torch.float64, device="cuda")

                        def call():
                            nat.check(nat.propagate(op._h, _ptr(planes) if want else None, _ptr(met), _ptr(spec), nf, _ptr(zl),
                                                    nd, q0, 0, _ptr(work), _stream()))
                        for _ in range(3):
                            call()
                        path = "one launch" if S <= 128 and tile else "two-pass"
                        results[(path, want)] = (timed(call, args.reps), met.clone(), planes.clone() if want else None)
                op.set_tile(True)
            for want in (False, True):
                for _ in range(3):
                    torch_series(spec, H, want)
                results[("torch", want)] = (timed(lambda: torch_series(spec, H, want), args.reps),) + \
                    tuple(reversed(torch_series(spec, H, want)))
            for (path, want), (dt, m, p) in results.items():
                ref_m = results[("torch", want)][1]
                line = "S %d %-10s %-12s %8.1f us" % (S, path, "with planes" if want else "figures only", dt * 1e6)
                if path != "torch":
                    line += "   (torch %.1f x; power agrees with torch to %.1e)" % (
                        results[("torch", want)][0] / dt, float(((m[..., 0] - ref_m[..., 0]).abs() / ref_m[..., 0]).max()))
                out.write(line + "\n")
                print(line, flush=True)
            out.flush()


if __name__ == "__main__":
    main()
