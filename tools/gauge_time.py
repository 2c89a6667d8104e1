"""Time of the illumination map and of the gauge fit / apply against one object adjoint, at the geometry of
BASELINE.json configs[1]: 4096 positions, nprb = ndet = 256, that config's object, 1 and 4 probe modes.

Device events around a block of back-to-back calls, after WARM calls of the same shape; the calls per block are sized
per operation from a short trial so that a block lasts about WINDOW_MS (at least MIN_REPS calls): a window of a few
milliseconds would measure the scheduler.  BLOCKS such blocks per operation, interleaved so that a drift of the clocks
or of the neighbours' load hits every operation alike.  Reported: the median
block (ms per call) with the fastest and the slowest block, and the ratio of the medians to ``PtychoHIP.adj``.

    python tools/gauge_time.py [--out FILE]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "libtike-cufft_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import libtike.hipfft as pt  # noqa: E402
from libtike.hipfft import synthetic as syn  # noqa: E402

WARM, MIN_REPS, BLOCKS, WINDOW_MS = 3, 20, 7, 250.0


def block_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the report to this file as well")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("gauge_time.py needs a GPU: a time taken anywhere else says nothing")
    p = syn.make_problem(64, 64, 8, 256, 256, seed=1234)
    nz, n, nscan = p["nz"], p["n"], p["nscan"]
    dev = lambda x: torch.as_tensor(x, device="cuda")  # noqa: E731
    psi, scan, prb1 = dev(p["psi"]), dev(p["scan"]), dev(p["probe"])
    rng = np.random.default_rng(1)
    extra = (rng.standard_normal((1, 3, 256, 256)) + 1j * rng.standard_normal((1, 3, 256, 256))).astype(np.complex64)
    prb4 = torch.cat((prb1[:, None], dev(extra) * prb1.abs().max() * 0.1), 1).contiguous()
    ill = torch.empty((1, nz, n), dtype=torch.float32, device="cuda")
    weight = pt.illumination(scan, prb1, nz, n)
    work = psi.clone()
    ops = {}
    with pt.PtychoHIP(nscan, 256, 256, 1, nz, n) as op:
        g = op.fwd(psi, scan, prb1)
        back = torch.empty_like(psi)
        ops["adj (PtychoHIP.adj, 1 mode)"] = lambda: op.adj(g, scan, prb1, out=back)
        ops["illumination, 1 mode"] = lambda: pt.illumination(scan, prb1, nz, n, out=ill)
        ops["illumination, 4 modes"] = lambda: pt.illumination(scan, prb4, nz, n, out=ill)
        ops["fit_gauge (weight, no ref)"] = lambda: pt.fit_gauge(psi, weight)
        ops["fit_gauge (weight, ref)"] = lambda: pt.fit_gauge(psi, weight, work)
        gauge = pt.fit_gauge(psi, weight)
        gauge[:, 3] = 1.0   # applied over and over to one buffer: keep its amplitude where it is
        ops["apply_gauge (object)"] = lambda: pt.apply_gauge(work, gauge, "object")
        ops["fit_gauge + apply_gauge"] = lambda: pt.apply_gauge(work, pt.fit_gauge(work, weight), "object")   # fixes its own output: stays put
        for fn in ops.values():
            for _ in range(WARM):
                fn()
        torch.cuda.synchronize()
        reps = {k: max(MIN_REPS, min(20000, int(WINDOW_MS / max(block_ms(fn, MIN_REPS), 1e-4)))) for k, fn in ops.items()}
        times = {k: [] for k in ops}
        for _ in range(BLOCKS):
            for k, fn in ops.items():
                times[k].append(block_ms(fn, reps[k]))
    med = {k: float(np.median(v)) for k, v in times.items()}
    base = med["adj (PtychoHIP.adj, 1 mode)"]
    lines = ["tools/gauge_time.py on %s: %d positions x 256^2, object %d x %d; %d blocks of about %g ms per operation after %d warm-up calls"
             % (torch.cuda.get_device_name(0), nscan, nz, n, BLOCKS, WINDOW_MS, WARM),
             "%-34s %8s %10s %10s %10s %10s" % ("operation", "calls", "median ms", "fastest", "slowest", "/ adj")]
    for k, v in times.items():
        lines.append("%-34s %8d %10.4f %10.4f %10.4f %10.3f" % (k, reps[k], med[k], min(v), max(v), med[k] / base))
    for m in ("1 mode", "4 modes"):
        r = med["illumination, " + m] / base
        lines.append("illumination, %s, costs %.3f of one adj: %s" % (m, r, "below 1" if r < 1 else "NOT below 1"))
    text = "\n".join(lines)
    print(text)
    if args.out:
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
