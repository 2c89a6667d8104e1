#!/usr/bin/env python
"""Time the B-spline resampler (libtike.hipfft.resample) against torch's bilinear grid_sample.

For a batch of complex64 images (default 8 x 2048 x 2048): per order the prefilter (two launches) and the warp under a
17 degree rotation about the centre (one launch, coefficients given), each as the bytes that must move -- the input once
and the output once -- over the time, beside the rate a device-to-device copy of the same bytes reaches in the same call.
The baseline, measured alternately with order 1 in the same call, is ``torch.nn.functional.grid_sample(mode="bilinear",
align_corners=True)`` on the real and imaginary channels with a precomputed grid: the same arithmetic as ``order=1``;
the two must agree to 1e-5 of the largest value where the four neighbours lie inside the image before anything is timed.
The kernels are timed through the C ABI with every buffer allocated beforehand; ``warp (api)`` is the public function,
which also copies the six numbers of the map to the device.  Appends to --out (profiles/r16/resample.txt).

    python tools/resample_time.py [--images 8] [--size 2048] [--reps 20] [--rounds 5] [--out profiles/r16/resample.txt]
"""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "libtike-cufft_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))

from libtike.hipfft import _native as nat  # noqa: E402
from libtike.hipfft import resample as rs  # noqa: E402
from libtike.hipfft.operators import _ptr, _stream  # noqa: E402


def smooth_images(nimg, n):
    """Complex64 images of a few long waves (period >= n / 5): a float32 coordinate cannot move their value by 1e-5."""
    y, x = torch.meshgrid(torch.arange(n, dtype=torch.float64, device="cuda"),
                          torch.arange(n, dtype=torch.float64, device="cuda"), indexing="ij")
    out = []
    for i in range(nimg):
        k = 2 * np.pi / n
        re = torch.cos(k * (2 + i % 3) * y + 0.3 * i) * torch.sin(k * 3 * x) + 0.2 * torch.cos(k * 5 * (x + y))
        im = torch.sin(k * 2 * y - k * (1 + i % 4) * x) + 0.1 * i
        out.append(torch.complex(re, im).to(torch.complex64))
    return torch.stack(out)


def rotation(n, degrees):
    a = np.deg2rad(degrees)
    m = np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])
    c = np.array([(n - 1) / 2.0, (n - 1) / 2.0])
    return m, c - m @ c


def grid_for(m, off, n, nimg):
    """grid_sample's normalised (x, y) grid of the map, float32, and the mask of pixels whose neighbours are all inside."""
    oy, ox = torch.meshgrid(torch.arange(n, dtype=torch.float64, device="cuda"),
                            torch.arange(n, dtype=torch.float64, device="cuda"), indexing="ij")
    sy, sx = m[0, 0] * oy + m[0, 1] * ox + off[0], m[1, 0] * oy + m[1, 1] * ox + off[1]
    grid = torch.stack([2 * sx / (n - 1) - 1, 2 * sy / (n - 1) - 1], -1).to(torch.float32)
    inside = (sy >= 1) & (sy <= n - 2) & (sx >= 1) & (sx <= n - 2)
    return grid[None].expand(nimg, n, n, 2).contiguous(), inside


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


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=8)
    ap.add_argument("--size", type=int, default=2048)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r16", "resample.txt"))
    args = ap.parse_args()
    nimg, n = args.images, args.size
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    x = smooth_images(nimg, n)
    m, off = rotation(n, 17.0)
    xf = torch.from_numpy(np.tile(np.concatenate([m.ravel(), off]), (nimg, 1))).cuda()
    res, coef = torch.empty_like(x), torch.empty_like(x)
    work = torch.empty((int(nat.spline_work_words(nimg, n, n, 1)),), dtype=torch.float64, device="cuda")
    moved = 2 * x.numel() * 8

    def prefilter(order):
        nat.check(nat.spline_prefilter(_ptr(coef), _ptr(x), nimg, n, n, 1, order, _ptr(work), _stream()))

    def warp(order, src):
        nat.check(nat.warp(_ptr(res), _ptr(src), _ptr(xf), nimg, n, n, n, n, 1, order, 0, 0.0, 0.0, None, _stream()))

    # the baseline computes what order 1 computes
    grid, inside = grid_for(m, off, n, nimg)
    planes = torch.view_as_real(x).permute(0, 3, 1, 2).contiguous()                   # [nimg, 2, n, n]

    def baseline():
        return torch.nn.functional.grid_sample(planes, grid, mode="bilinear", padding_mode="zeros", align_corners=True)
    warp(1, x)
    ours = torch.view_as_real(res).permute(0, 3, 1, 2)
    diff = ((ours - baseline()).abs() * inside).max().item() / x.abs().max().item()
    with open(args.out, "a") as out:
        def say(line):
            out.write(line + "\n")
            out.flush()
            print(line, flush=True)
        say("# tools/resample_time.py on %s: %d x %d x %d complex64, 17 degree rotation, %d bytes must move per call"
            % (torch.cuda.get_device_name(0), nimg, n, n, moved))
        say("order 1 against grid_sample (bilinear, align_corners) where the neighbours are inside: %.2e of the largest value"
            % diff)
        if not diff <= 1e-5:
            raise SystemExit("order 1 and grid_sample disagree: %.3e" % diff)
        (t_copy,), _ = median_alternating([lambda: res.copy_(x)], args.reps, args.rounds)
        say("copy of the same bytes: %.1f us, %.2f TB/s" % (t_copy * 1e6, moved / t_copy * 1e-12))
        (t1, tb), (s1, sb) = median_alternating([lambda: warp(1, x), baseline], args.reps, args.rounds)
        say("warp order 1: %.1f us (spread %.1f), %.2f TB/s; grid_sample: %.1f us (spread %.1f); ratio %.2f"
            % (t1 * 1e6, s1 * 1e6, moved / t1 * 1e-12, tb * 1e6, sb * 1e6, tb / t1))
        for order in range(6):
            if order >= 2:
                (tp,), (sp,) = median_alternating([lambda: prefilter(order)], args.reps, args.rounds)
                say("prefilter order %d: %.1f us (spread %.1f), %.2f TB/s, %.2f of the copy rate"
                    % (order, tp * 1e6, sp * 1e6, moved / tp * 1e-12, t_copy / tp))
            src = coef if order >= 2 else x
            (tw, ta), (sw, sa) = median_alternating(
                [lambda: warp(order, src), lambda: rs.warp(src, m, off, None, order, prefilter=False, out=res)],
                args.reps, args.rounds)
            say("warp order %d: %.1f us (spread %.1f), %.2f TB/s, %.2f of the copy rate; warp (api) %.1f us"
                % (order, tw * 1e6, sw * 1e6, moved / tw * 1e-12, t_copy / tw, ta * 1e6))


if __name__ == "__main__":
    main()
