"""Time of ``fit_frames`` (csrc/k_fit.hpp) at 4096 positions x 256^2, for one probe mode (farplane + data, 12 bytes per
pixel read) and for three (summed intensity of two modes + last farplane + data, 16 bytes per pixel), with and without
the per-pixel maps, of ``accumulate_intensity``, and of the same sums written in plain torch on the same device.

Device events around a block of back-to-back calls, after WARM calls of the same shape; the calls per block are sized
per operation from a short trial so that a block lasts about WINDOW_MS (at least MIN_REPS calls).  BLOCKS such blocks per
operation, interleaved so that a drift of the clocks or of the neighbours' load hits every operation alike.  Reported:
the median block (ms per call) with the fastest and the slowest block, the bytes the operation has to read (inputs) and
the bytes it moves in all (inputs, outputs, and the partial sums written to and read back from the scratch), and the
rate of the inputs and of all bytes over the median time.  The inputs (3 to 4 GiB) do not fit the 256 MiB cache.

    python tools/fit_time.py [--out FILE] [--nscan 4096] [--ndet 256]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "libtike-cufft_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import libtike.hipfft as pt  # noqa: E402
from libtike.hipfft import _native as nat  # noqa: E402
from libtike.hipfft.operators import _ptr, _stream  # noqa: E402

WARM, MIN_REPS, BLOCKS, WINDOW_MS = 3, 10, 7, 250.0


def block_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def torch_fit(data, g, inten, pixels):
    """The sums of ``fit_frames`` in plain torch: float32 terms, float64 sums (whose order torch chooses)."""
    I = g.real * g.real + g.imag * g.imag
    if inten is not None:
        I = inten + I
    sI, sd = torch.sqrt(I), torch.sqrt(data)
    diff = sI - sd
    sq = diff * diff
    terms = (I, data, torch.sqrt(I * data), sq, I - data * torch.log(I + 1e-32), data - data * torch.log(data + 1e-32),
             diff.abs(), sd)
    frames = torch.stack([t.sum((-2, -1), dtype=torch.float64) for t in terms], -1)
    maps = torch.stack([t.sum(1, dtype=torch.float64) for t in (I, data, diff, sq)], 1) if pixels else None
    return frames, maps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the report to this file as well")
    ap.add_argument("--nscan", type=int, default=4096)
    ap.add_argument("--ndet", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("fit_time.py needs a GPU: a time taken anywhere else says nothing")
    nscan, ndet = args.nscan, args.ndet
    npix, shape = ndet * ndet, (1, nscan, ndet, ndet)
    gen = torch.Generator(device="cuda").manual_seed(1)
    fall = torch.logspace(1.5, -0.5, npix, device="cuda").reshape(ndet, ndet)     # amplitudes over two decades
    g = torch.view_as_complex(torch.randn(shape + (2,), generator=gen, device="cuda") * fall[..., None])
    other = torch.randn(shape, generator=gen, device="cuda").square_() * fall * fall
    data = torch.poisson(1.3 * (g.real * g.real + g.imag * g.imag), generator=gen)
    data3 = torch.poisson(1.3 * (other + g.real * g.real + g.imag * g.imag), generator=gen)
    scratch = torch.empty(shape, dtype=torch.float32, device="cuda")

    # bytes: inputs, and everything (outputs and both directions of the partial sums in the scratch)
    words = int(nat.fit_work_words(1, nscan, npix))
    nwt = -(-npix // 512)
    fwords = nscan * nwt * 8 if nwt > 1 else 0
    pwords = words - fwords
    total = nscan * npix
    out_f, out_p = nscan * 8 * 8, 4 * npix * 8
    extra = {False: 2 * 8 * fwords + out_f, True: 2 * 8 * fwords + out_f + 2 * 8 * pwords + out_p}
    ops, nbytes = {}, {}

    def add(name, fn, inputs, moved):
        ops[name], nbytes[name] = fn, (inputs, moved)

    for pix in (True, False):
        tag = "maps" if pix else "no maps"
        add("fit_frames M=1, %s" % tag, lambda pix=pix: pt.fit_frames(data, g, None, pixels=pix), 12 * total, 12 * total + extra[pix])
        add("fit_frames M=3, %s" % tag, lambda pix=pix: pt.fit_frames(data3, g, other, pixels=pix), 16 * total, 16 * total + extra[pix])
    add("accumulate_intensity (=)", lambda: nat.check(nat.fit_accumulate(_ptr(scratch), _ptr(g), total, 0, _stream())),
        8 * total, 12 * total)
    add("accumulate_intensity (+=)", lambda: pt.accumulate_intensity(g, out=scratch), 12 * total, 16 * total)
    add("torch, M=1, maps", lambda: torch_fit(data, g, None, True), 12 * total, 12 * total)
    add("torch, M=1, no maps", lambda: torch_fit(data, g, None, False), 12 * total, 12 * total)

    # the two formulations agree before either is timed
    mine, theirs = pt.fit_frames(data, g), torch_fit(data, g, None, True)
    for a, b, dims in ((mine["frames"], theirs[0], (0, 1)), (mine["pixels"], theirs[1], (0, 2, 3))):
        scale = b.abs().amax(dim=dims, keepdim=True)                   # per column / per map
        assert float(((a - b).abs() / scale).max()) < 1e-5
    del mine, theirs

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
    lines = ["tools/fit_time.py on %s: %d positions x %d^2; %d blocks of about %g ms per operation after %d warm-up calls; "
             "scratch %d float64 words" % (torch.cuda.get_device_name(0), nscan, ndet, BLOCKS, WINDOW_MS, WARM, words),
             "%-28s %6s %10s %9s %9s %11s %11s %10s %10s" % ("operation", "calls", "median ms", "fastest", "slowest",
                                                              "inputs GB", "moved GB", "inputs TB/s", "moved TB/s")]
    for k, v in times.items():
        inputs, moved = nbytes[k]
        lines.append("%-28s %6d %10.4f %9.4f %9.4f %11.3f %11.3f %10.2f %10.2f"
                     % (k, reps[k], med[k], min(v), max(v), inputs / 1e9, moved / 1e9, inputs / med[k] / 1e9, moved / med[k] / 1e9))
    for tag in ("maps", "no maps"):
        lines.append("torch / fit_frames, M=1, %s: %.1f x" % (tag, med["torch, M=1, %s" % tag] / med["fit_frames M=1, %s" % tag]))
    lines.append("(the torch rows count their inputs only: what torch moves through its temporaries was not measured)")
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
