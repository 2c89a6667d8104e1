"""CG iterations per second with and without a measured-pixel mask, alternating in one process, on bench.py's CG problem
(4096 positions x 256^2, Gaussian probe, one mode, object = 1) and on configs[2] (4096 x 512^2, 4 Hermite modes).
The mask is the "detector" mask of tests/cg_reference.py (beamstop, module gaps, 2 % dead pixels).

    python tools/cg_mask_time.py [--only 256|cfg3] [--mask on|off] [--iters K] [--rounds R]

--only / --mask restrict the run to one problem / one variant (for a kernel-trace run of each under rocprofv3)."""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "libtike-cufft_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import libtike.hipfft as pt  # noqa: E402
from libtike.hipfft import synthetic as syn  # noqa: E402
from cg_reference import detector_mask  # noqa: E402


def bench_problem(dev):
    R, step, ndet = 64, 8, 256
    nz, n = syn.object_size_for(R, R, step, ndet)
    psi = torch.as_tensor(syn.random_object(nz, n, np.random.default_rng(1234)), device=dev)
    prb = torch.as_tensor(syn.gaussian_probe(ndet), device=dev)
    scan = torch.as_tensor(syn.raster_scan(R, R, step, np.random.default_rng(1234)), device=dev)
    slv = pt.CGPtychoSolver(R * R, ndet, ndet, 1, nz, n)
    data = (torch.abs(slv.fwd(psi, scan, prb)) ** 2).contiguous()
    return slv, data, scan, prb[:, None].contiguous(), torch.ones_like(psi)


def cfg3_problem(dev):
    R, step, ndet, M = 64, 8, 512, 4
    nz = n = 1024
    rng = np.random.default_rng(4321)
    psi = torch.as_tensor(syn.random_object(nz, n, rng), device=dev)
    scan = torch.as_tensor(syn.raster_scan(R, R, step, rng), device=dev)
    modes = torch.as_tensor(syn.hermite_modes(ndet, M), device=dev)
    slv = pt.CGPtychoSolver(R * R, ndet, ndet, 1, nz, n)
    data = torch.zeros((1, R * R, ndet, ndet), dtype=torch.float32, device=dev)
    for k in range(M):
        data += torch.abs(slv.fwd(psi, scan, modes[:, k].contiguous())) ** 2
    slv.release_scratch()
    torch.cuda.empty_cache()
    return slv, data, scan, modes, torch.ones_like(psi)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["256", "cfg3"], default=None)
    ap.add_argument("--mask", choices=["on", "off"], default=None)
    ap.add_argument("--iters", type=int, default=None, help="iterations per timed run (default 50 at 256^2, 10 at configs[2])")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    problems = [("256", bench_problem, 50), ("cfg3", cfg3_problem, 10)]
    variants = [v for v in ("off", "on") if args.mask in (None, v)]
    for name, make, iters in problems:
        if args.only not in (None, name):
            continue
        iters = args.iters or iters
        slv, data, scan, prb, psi0 = make(dev)
        slv.verbose = False
        mask = torch.as_tensor(detector_mask(data.shape[-1]), device=dev)
        for v in variants:      # warm-up: every kernel of both variants loaded, work slots allocated
            slv.run(data, psi0, scan.clone(), prb.clone(), piter=2, mask=mask if v == "on" else None)
        torch.cuda.synchronize()
        rates = {v: [] for v in variants}
        for _ in range(args.rounds):
            for v in variants:
                t0 = time.perf_counter()
                slv.run(data, psi0, scan.clone(), prb.clone(), piter=iters, mask=mask if v == "on" else None)
                torch.cuda.synchronize()
                rates[v].append(iters / (time.perf_counter() - t0))
        slv.free()
        del data
        torch.cuda.empty_cache()
        line = "%s: %d iterations per run, %d rounds, mask measured fraction %.3f" % (
            name, iters, args.rounds, float(mask.float().mean()))
        for v in variants:
            line += " | mask %s: %s it/s (median %.2f)" % (v, " ".join("%.2f" % r for r in rates[v]), np.median(rates[v]))
        if len(variants) == 2:
            line += " | masked / unmasked %.4f" % (np.median(rates["on"]) / np.median(rates["off"]))
        print(line, flush=True)


if __name__ == "__main__":
    main()
