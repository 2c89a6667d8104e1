"""Cost of libtike.hipfft.frc: whole-call time from device events (warmed, median of --reps calls) for S in {512, 1024,
2048} x ptheta in {1, 8} x align on / off, and the host time of the NumPy restatement (tests/frc_ref.py) at one angle for
contrast.  Per-kernel times: run under ``rocprofv3 --kernel-trace --stats`` with ``--reps 3 --no-numpy``.

    python tools/frc_time.py [--reps R] [--no-numpy]"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "libtike-cufft_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import libtike.hipfft as pt  # noqa: E402


def call_ms(a, b, align, reps):
    pt.frc(a, b, align=align)
    pt.frc(a, b, align=align)
    times = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        pt.frc(a, b, align=align)
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1))
    return float(np.median(times)), float(min(times)), float(max(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-numpy", action="store_true")
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    for s in (512, 1024, 2048):
        for ptheta in (1, 8):
            shape = (ptheta, s, s)
            a = torch.randn(shape, dtype=torch.complex64, device=dev)
            b = a + 0.5 * torch.randn(shape, dtype=torch.complex64, device=dev)
            for align in (False, True):
                med, lo, hi = call_ms(a, b, align, args.reps)
                print("frc S %4d ptheta %d align %-5s: %8.3f ms (min %.3f, max %.3f; %d calls)"
                      % (s, ptheta, align, med, lo, hi, args.reps), flush=True)
            del a, b
            torch.cuda.empty_cache()
        if not args.no_numpy:
            import frc_ref as ref
            a = (rng.standard_normal((s, s)) + 1j * rng.standard_normal((s, s))).astype(np.complex64)
            b = a + 0.5 * (rng.standard_normal((s, s)) + 1j * rng.standard_normal((s, s))).astype(np.complex64)
            for align in (False, True):
                t = time.perf_counter()
                ref.frc(a, b, align=align)
                print("numpy restatement S %4d ptheta 1 align %-5s: %8.1f ms (host, float64, one call)"
                      % (s, align, 1e3 * (time.perf_counter() - t)), flush=True)


if __name__ == "__main__":
    main()
