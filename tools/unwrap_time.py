#!/usr/bin/env python
"""Time the phase unwrapper (libtike.hipfft.unwrap) against the same iteration written in torch slicing operations.

For N x N phases (default 768 and 2304) with 1 and 8 angles: the time of one PCG iteration of the HIP kernels (four
launches, measured over a block of enqueued iterations between two events) and the bytes per second this amounts to
(12 float32 per pixel and iteration without weights: apply reads r, 1 / D, p and writes p', q; update reads x, r, p', q,
1 / D and writes x, r), the same iteration as a user would write it in torch, the iterations and the wall time of a whole
solve to tol = 1e-4, and the observed error of the device against the float64 restatement of tests/unwrap_ref.py beside
the float32 restatement's own (the cases of tests/test_hip_unwrap.py).  Appends to --out (profiles/r10/unwrap.txt).

    python tools/unwrap_time.py [--sizes 768 2304] [--angles 1 8] [--out profiles/r10/unwrap.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "libtike-cufft_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from libtike.hipfft import _native as nat  # noqa: E402
from libtike.hipfft.operators import _ptr, _stream  # noqa: E402
from libtike.hipfft.unwrap import unwrap_phase  # noqa: E402

TWO_PI = 2.0 * np.pi


def make_phase(ptheta, n):
    """The bump on a ramp of tests/unwrap_ref.py scaled to the size, wrapped, float32, on the device."""
    y, x = torch.meshgrid(torch.arange(n, dtype=torch.float64, device="cuda"),
                          torch.arange(n, dtype=torch.float64, device="cuda"), indexing="ij")
    s = 0.18 * n
    planes = []
    for t in range(ptheta):
        amp = (0.3 - 0.02 * t) * n
        truth = amp * torch.exp(-((y - 0.45 * n) ** 2 + (x - 0.55 * n) ** 2) / (2 * s * s)) + 0.21 * x - 0.13 * y
        planes.append((truth - TWO_PI * torch.round(truth / TWO_PI)).to(torch.float32))
    return torch.stack(planes)


def torch_state(phase):
    """x, r, p, 1 / D, edge weights and rz of the unweighted problem, as torch tensors."""
    def W(a):
        return a - TWO_PI * torch.round(a / TWO_PI)
    dx, dy = W(phase[..., 1:] - phase[..., :-1]), W(phase[..., 1:, :] - phase[..., :-1, :])
    wx, wy = torch.ones_like(dx), torch.ones_like(dy)
    b, D = torch.zeros_like(phase), torch.zeros_like(phase)
    b[..., 1:] += dx; b[..., :-1] -= dx; b[..., 1:, :] += dy; b[..., :-1, :] -= dy          # noqa: E702
    D[..., 1:] += wx; D[..., :-1] += wx; D[..., 1:, :] += wy; D[..., :-1, :] += wy          # noqa: E702
    minv = 1.0 / D
    z = minv * b
    rz = (b.double() * z.double()).sum((-2, -1))
    return [torch.zeros_like(phase), b, z.clone(), minv, wx, wy, rz]


def torch_iteration(s):
    x, r, p, minv, wx, wy, rz = s
    tx, ty = wx * (p[..., 1:] - p[..., :-1]), wy * (p[..., 1:, :] - p[..., :-1, :])
    q = torch.zeros_like(p)
    q[..., 1:] += tx; q[..., :-1] -= tx; q[..., 1:, :] += ty; q[..., :-1, :] -= ty          # noqa: E702
    alpha = rz / (p.double() * q.double()).sum((-2, -1))
    a32 = alpha.float()[:, None, None]
    x += a32 * p
    r -= a32 * q
    z = minv * r
    rz2 = (r.double() * z.double()).sum((-2, -1))
    s[2] = z + (rz2 / rz).float()[:, None, None] * p
    s[6] = rz2


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn(reps)
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def hip_iteration_time(phase, reps):
    ptheta, nz, n = phase.shape
    buf = torch.empty((int(nat.unwrap_buffer_floats(ptheta, nz, n)),), dtype=torch.float32, device="cuda")
    work = torch.empty((int(nat.unwrap_work_words(ptheta, nz, n)),), dtype=torch.float64, device="cuda")
    state = torch.empty((ptheta, nat.UNWRAP_STATE_WORDS), dtype=torch.float64, device="cuda")
    nat.check(nat.unwrap_begin(_ptr(buf), _ptr(state), _ptr(phase), None, ptheta, nz, n, _ptr(work), _stream()))

    def run(k):
        nat.check(nat.unwrap_iterate(_ptr(buf), _ptr(state), None, ptheta, nz, n, k, 10 ** 9, 0.0, _ptr(work), _stream()))
    run(5)
    dt = timed(run, reps)
    assert (state[:, nat.UNWRAP_ITER] == 5 + reps).all(), state[:, :8]     # every enqueued iteration ran
    return dt


def errors(out):
    import unwrap_ref as ref
    truth = ref.make_truth(67, 129, 25)
    phi = ref.wrap(truth + np.random.default_rng(11).normal(0, 0.6, truth.shape)).astype(np.float32)
    w = np.ones(phi.shape, np.float32)
    w[:, 60:63] = 0

    def centred(a):
        a = a.astype(np.float64)
        return a - a.mean()
    for name, weight in (("case 3, noise 0.6 rad, unweighted", None), ("case 4, two regions", w)):
        got = unwrap_phase(phi, weight=weight, tol=1e-6, congruent=False)
        r64 = ref.unwrap(phi, weight, tol=1e-6, congruent=False)
        r32 = ref.unwrap(phi, weight, tol=1e-6, congruent=False, dtype=np.float32)
        m = slice(0, 60) if weight is not None else slice(None)
        dev = got["phase"].cpu().numpy()
        e_dev = np.abs(centred(dev[:, m]) - centred(r64["phase"][:, m])).max()
        d32 = np.abs(centred(r32["phase"][:, m]) - centred(r64["phase"][:, m])).max()
        out.write("error 67x129 %s: device %.2e rad, float32 restatement %.2e rad; iterations %d / %d / %d (device, "
                  "float64, float32); residues %d\n" % (name, e_dev, d32, got["iterations"], r64["iterations"],
                                                         r32["iterations"], got["residues"]))


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--sizes", type=int, nargs="+", default=[768, 2304])
    ap.add_argument("--angles", type=int, nargs="+", default=[1, 8])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "unwrap.txt"))
    args = ap.parse_args()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "a") as out:
        out.write("# tools/unwrap_time.py on %s\n" % torch.cuda.get_device_name(0))
        errors(out)
        out.flush()
        for n in args.sizes:
            for ptheta in args.angles:
                phase = make_phase(ptheta, n)
                t_hip = hip_iteration_time(phase, args.reps)
                s = torch_state(phase)
                for _ in range(3):
                    torch_iteration(s)
                t_torch = timed(lambda k: [torch_iteration(s) for _ in range(k)], max(5, args.reps // 5))
                del s
                gbs = 12 * 4 * ptheta * n * n / t_hip * 1e-9
                t0 = time.perf_counter()
                got = unwrap_phase(phase)
                torch.cuda.synchronize()
                wall = time.perf_counter() - t0
                line = ("%d x %d, %d angle(s): HIP iteration %.1f us (%.0f GB/s), torch iteration %.1f us (%.1f x); solve to "
                        "tol 1e-4: %s iterations, %.3f s, converged %s\n"
                        % (n, n, ptheta, t_hip * 1e6, gbs, t_torch * 1e6, t_torch / t_hip,
                           np.asarray(got["iterations"]).tolist(), wall, np.asarray(got["converged"]).tolist()))
                out.write(line)
                out.flush()
                print(line, end="", flush=True)
                del phase, got


if __name__ == "__main__":
    main()
