#!/usr/bin/env python
"""Time the first-look kernels (libtike.hipfft.dpc): the moment pass, the scan map and one iteration of the integration.

The moment pass reads ``data`` once (default 4096 x 256^2 float32, 1 GiB) and writes eight float64 per frame: its time is
given as the bytes of ``data`` over the time, beside a device-to-device copy of the same bytes (which reads and writes
them, i.e. moves twice as many) and beside the same six sums and the dark-field sum formed with torch (float64
``tensordot`` of the frames with the seven weight images: what a user would write without the kernel), timed alternately
in the same call; the two must agree to 1e-9 of each figure's scale before anything is timed.  ``scan_map`` (four
channels, with the illumination launch that forms its weight) and one iteration of the solver (four launches) are timed
at two object sizes (default 768^2 and 2304^2) for a raster of positions 8 pixels apart and a 256-pixel probe.
Everything goes through the C ABI with every buffer allocated beforehand.  Appends to --out (profiles/r17/dpc.txt).

    python tools/dpc_time.py [--frames 4096] [--ndet 256] [--sizes 768 2304] [--reps 10] [--rounds 5] [--out ...]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "libtike-cufft_amd"))

from libtike.hipfft import _native as nat  # noqa: E402
from libtike.hipfft.operators import _ptr, _stream  # noqa: E402


def timed(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e-3 / reps


def median_alternating(fns, reps, rounds):
    """Median over ``rounds`` of the time of each function, the functions taking turns within a round."""
    for fn in fns:
        fn()
    times = [[] for _ in fns]
    for _ in range(rounds):
        for i, fn in enumerate(fns):
            times[i].append(timed(fn, reps))
    return [float(np.median(t)) for t in times], [float(np.ptp(t)) for t in times]


def weight_images(ndet, radius):
    """The seven weight images of the moments, float64 ``[7, ndet * ndet]``."""
    r = torch.arange(ndet, dtype=torch.float64, device="cuda")
    k = torch.where(r < ndet - ndet // 2, r, r - ndet)
    ky, kx = k[:, None].expand(ndet, ndet), k[None, :].expand(ndet, ndet)
    one = torch.ones_like(ky)
    dark = (ky * ky + kx * kx > radius * radius).to(torch.float64)
    return torch.stack([one, ky, kx, ky * ky, kx * kx, ky * kx, dark]).reshape(7, -1)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--frames", type=int, default=4096)
    ap.add_argument("--ndet", type=int, default=256)
    ap.add_argument("--sizes", type=int, nargs="+", default=[768, 2304])
    ap.add_argument("--nprb", type=int, default=256)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r17", "dpc.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("tools/dpc_time.py needs a GPU: a time taken elsewhere says nothing")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    nscan, ndet = args.frames, args.ndet
    gen = torch.Generator(device="cuda").manual_seed(1)
    with open(args.out, "a") as out:
        def say(line):
            out.write(line + "\n")
            out.flush()
            print(line, flush=True)

        # ---- the moment pass -------------------------------------------------------------------------------------------
        data = torch.rand((1, nscan, ndet, ndet), generator=gen, device="cuda", dtype=torch.float32) ** 4 * 1000
        radius = 0.25 * ndet
        moved = data.numel() * 4
        mom = torch.empty((1, nscan, 8), dtype=torch.float64, device="cuda")
        work = torch.empty((max(int(nat.frame_moments_work_words(1, nscan, ndet)), 1),), dtype=torch.float64, device="cuda")

        def moments():
            nat.check(nat.frame_moments(_ptr(mom), _ptr(data), None, radius, 1, nscan, ndet, _ptr(work), _stream()))

        wimg = weight_images(ndet, radius)
        frames = data.reshape(nscan, -1)
        chunk = max(1, (1 << 28) // (ndet * ndet * 8))                    # float64 copies of at most 256 MiB at a time

        def with_torch():
            return torch.cat([frames[j:j + chunk].to(torch.float64) @ wimg.T for j in range(0, nscan, chunk)])
        moments()
        want = with_torch()
        scale = (frames.to(torch.float32).abs().sum(1, dtype=torch.float64)[:, None] * wimg.abs().amax(1)[None, :])
        diff = ((mom[0, :, :7] - want).abs() / scale).max().item()
        say("# tools/dpc_time.py on %s: moments of %d x %d^2 float32, %d bytes read per call" % (
            torch.cuda.get_device_name(0), nscan, ndet, moved))
        say("moments against the torch sums: %.2e of each figure's scale" % diff)
        if not diff <= 1e-9:
            raise SystemExit("the moment pass and the torch sums disagree: %.3e" % diff)
        copy = torch.empty_like(data)
        (t_copy,), (s_copy,) = median_alternating([lambda: copy.copy_(data)], args.reps, args.rounds)
        say("copy of the same bytes (reads and writes them): %.1f us (spread %.1f), %.2f TB/s moved"
            % (t_copy * 1e6, s_copy * 1e6, 2 * moved / t_copy * 1e-12))
        del copy
        (t_m, t_t), (s_m, s_t) = median_alternating([moments, with_torch], max(2, args.reps // 2), args.rounds)
        say("frame_moments: %.1f us (spread %.1f), %.2f TB/s read, %.2f of the copy's time; torch sums: %.1f us (spread %.1f); "
            "ratio %.1f" % (t_m * 1e6, s_m * 1e6, moved / t_m * 1e-12, t_m / t_copy, t_t * 1e6, s_t * 1e6, t_t / t_m))
        del data, frames, want

        # ---- the scan map and one iteration of the integration --------------------------------------------------------
        for size in args.sizes:
            nprb = min(args.nprb, size // 2)
            py, px = np.meshgrid(np.arange(0.25, size - nprb - 1, 8.0), np.arange(0.5, size - nprb - 1, 8.0), indexing="ij")
            scan = torch.from_numpy(np.stack([py.ravel(), px.ravel()], -1).astype(np.float32)[None]).cuda()
            npos = scan.shape[1]
            r = torch.arange(nprb, dtype=torch.float32, device="cuda") - (nprb - 1) / 2
            g = torch.exp(-(r / (nprb / 6.0)) ** 2)
            probe = (g[:, None] * g[None, :]).to(torch.complex64)[None, None].contiguous()
            values = torch.rand((1, npos, 4), generator=gen, device="cuda", dtype=torch.float32)
            weight = torch.empty((1, size, size), dtype=torch.float32, device="cuda")
            res = torch.empty((1, 4, size, size), dtype=torch.float32, device="cuda")

            def scan_map():
                nat.check(nat.scan_map(_ptr(weight), _ptr(res), _ptr(values), None, _ptr(scan), _ptr(probe), 1, npos, 4, 1, nprb,
                                       size, size, 0, None, _stream()))

            def illum():
                nat.check(nat.illumination(_ptr(weight), _ptr(scan), _ptr(probe), 1, npos, 1, nprb, size, size, _stream()))
            (t_s, t_i), (s_s, s_i) = median_alternating([scan_map, illum], max(1, args.reps // 5), args.rounds)
            say("scan_map %d^2, %d positions, nprb %d, 4 channels: %.2f ms (spread %.2f), of which the illumination launch "
                "%.2f ms (spread %.2f)" % (size, npos, nprb, t_s * 1e3, s_s * 1e3, t_i * 1e3, s_i * 1e3))
            buf = torch.empty((int(nat.unwrap_buffer_floats(1, size, size)),), dtype=torch.float32, device="cuda")
            uwork = torch.empty((int(nat.unwrap_work_words(1, size, size)),), dtype=torch.float64, device="cuda")
            state = torch.empty((1, nat.UNWRAP_STATE_WORDS), dtype=torch.float64, device="cuda")
            gy, gx = res[:, 2].contiguous(), res[:, 3].contiguous()
            wn = (weight / weight.amax()).contiguous()
            block = 50

            def begin():
                nat.check(nat.integrate_begin(_ptr(buf), _ptr(state), _ptr(gy), _ptr(gx), _ptr(wn), 1, size, size, _ptr(uwork),
                                              _stream()))

            def iterate():                                                # from a fresh start, so that no angle has stopped
                begin()
                nat.check(nat.unwrap_iterate(_ptr(buf), _ptr(state), _ptr(wn), 1, size, size, block, 1 << 30, 0.0, _ptr(uwork),
                                             _stream()))
            (t_b, t_it), (s_b, s_it) = median_alternating([begin, iterate], max(1, args.reps // 5), args.rounds)
            per = (t_it - t_b) / block
            say("integrate %d^2: begin %.1f us (spread %.1f), one iteration %.1f us (%d iterations in %.2f ms, spread %.2f), "
                "%.2f TB/s of the 13 float32 planes an iteration moves" % (size, t_b * 1e6, s_b * 1e6, per * 1e6, block,
                                                                           (t_it - t_b) * 1e3, s_it * 1e3,
                                                                           13 * size * size * 4 / per * 1e-12))
            if not float(state[0, nat.UNWRAP_ITER].item()) == block:
                raise SystemExit("the timed iterations did not all run: %r" % state[0].tolist())


if __name__ == "__main__":
    main()
