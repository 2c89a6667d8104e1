"""Cost of ortho_prb: CG iterations per second with ortho_prb=False and True, alternating in one process, with probe
recovery on two 4-mode problems -- bench.py's CG geometry with 4 Hermite modes (4096 positions x 256^2) and configs[2]
(4096 x 512^2, 4 Hermite modes) -- plus the device time of one orthogonalize_modes call (probe + two companions, CUDA
events, median of 50) at those sizes and at 8 and 16 modes.

    python tools/cg_ortho_time.py [--only 256|cfg3] [--iters K] [--rounds R]"""
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


def problem(dev, ndet, nz, seed):
    R, step, M = 64, 8, 4
    rng = np.random.default_rng(seed)
    if nz is None:
        nz, n = syn.object_size_for(R, R, step, ndet)
    else:
        n = nz
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


def helper_ms(dev, nmodes, nprb, reps=50):
    x = [torch.randn((1, nmodes, nprb, nprb), dtype=torch.complex64, device=dev) for _ in range(3)]
    pt.orthogonalize_modes(*x)
    times = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        pt.orthogonalize_modes(*x)
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    return float(np.median(times))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", choices=["256", "cfg3"], default=None)
    ap.add_argument("--iters", type=int, default=None, help="iterations per timed run (default 20 at 256^2, 6 at configs[2])")
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    dev = torch.device("cuda", 0)
    for nmodes, nprb in ((4, 256), (4, 512), (8, 256), (16, 256)):
        print("orthogonalize_modes, %2d modes x %d^2, probe + 2 companions: %.3f ms" % (nmodes, nprb, helper_ms(dev, nmodes, nprb)),
              flush=True)
    problems = [("256", 256, None, 1234, 20), ("cfg3", 512, 1024, 4321, 6)]
    for name, ndet, nz, seed, iters in problems:
        if args.only not in (None, name):
            continue
        iters = args.iters or iters
        slv, data, scan, prb, psi0 = problem(dev, ndet, nz, seed)
        slv.verbose = False
        for ortho in (False, True):     # warm-up
            slv.run(data, psi0, scan.clone(), prb.clone(), piter=2, recover_prb=True, ortho_prb=ortho)
        torch.cuda.synchronize()
        rates = {False: [], True: []}
        for _ in range(args.rounds):
            for ortho in (False, True):
                t0 = time.perf_counter()
                slv.run(data, psi0, scan.clone(), prb.clone(), piter=iters, recover_prb=True, ortho_prb=ortho)
                torch.cuda.synchronize()
                rates[ortho].append(iters / (time.perf_counter() - t0))
        slv.free()
        del data
        torch.cuda.empty_cache()
        print("%s (4 modes, probe recovery): %d iterations per run, %d rounds | off: %s it/s (median %.3f) | on: %s it/s "
              "(median %.3f) | on / off %.4f" % (name, iters, args.rounds, " ".join("%.3f" % r for r in rates[False]),
                                                 np.median(rates[False]), " ".join("%.3f" % r for r in rates[True]),
                                                 np.median(rates[True]), np.median(rates[True]) / np.median(rates[False])),
              flush=True)


if __name__ == "__main__":
    main()
