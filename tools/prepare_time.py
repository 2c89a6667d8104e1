"""Time of ``prepare_frames`` (csrc/k_prepare.hpp) at 4096 positions x 256^2 output pixels: 16-bit counts at bin 1, 16-bit
counts at bin 2 from 512^2 raw frames, float32 at bin 1; each with and without the per-pixel maps.  Then the same
preparation end to end from host memory, beside the host chain it replaces (``PtychoDataset.from_record`` +
``solver_inputs`` + the copy of float32 ``data`` to the device).

Kernel rows: device events around a block of back-to-back calls on device-resident frames, after WARM calls; the calls
per block are sized from a short trial so that a block lasts about WINDOW_MS (at least MIN_REPS calls); BLOCKS blocks per
setting, interleaved.  Reported: the median block (ms per call) with the fastest and the slowest, the bytes of the
definition (raw frames read once: nscan (bin ndet)^2 sizeof(raw); data written once: nscan ndet^2 4), the bytes moved in
all (adding the statistics and both directions of the partial results in the scratch) and both over the median time.
End-to-end rows: a host clock from NumPy arrays in pageable memory to a synchronise, REPEAT times, the median.

    python tools/prepare_time.py [--out FILE] [--nscan 4096] [--ndet 256]
"""
import argparse
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "libtike-cufft_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import libtike.hipfft as pt  # noqa: E402
from libtike.hipfft import _native as nat  # noqa: E402
from libtike.hipfft.io import PtychoDataset, solver_inputs  # noqa: E402

WARM, MIN_REPS, BLOCKS, WINDOW_MS, REPEAT = 3, 10, 7, 250.0, 3


def block_ms(fn, reps):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def host_ms(fn):
    times = []
    for _ in range(REPEAT):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


def counts(nscan, side):
    """Device frames of 16-bit counts, falling off from the centre over three decades."""
    gen = torch.Generator(device="cuda").manual_seed(1)
    y = torch.linspace(-1, 1, side, device="cuda")
    fall = 20000.0 * torch.exp(-7.0 * (y[:, None] ** 2 + y[None, :] ** 2)) + 2.0
    return torch.poisson(fall.expand(nscan, side, side), generator=gen).to(torch.int16).view(torch.uint16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="append the report to this file as well")
    ap.add_argument("--nscan", type=int, default=4096)
    ap.add_argument("--ndet", type=int, default=256)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("prepare_time.py needs a GPU: a time taken anywhere else says nothing")
    nscan, ndet = args.nscan, args.ndet
    npix = ndet * ndet
    u16 = counts(nscan, ndet)
    u16x2 = counts(nscan, 2 * ndet)
    f32 = u16.to(torch.int32).to(torch.float32)
    out = torch.empty((1, nscan, ndet, ndet), dtype=torch.float32, device="cuda")
    settings = {"uint16, bin 1": (u16, 1), "uint16, bin 2 from %d^2" % (2 * ndet): (u16x2, 2), "float32, bin 1": (f32, 1)}

    words = int(nat.prepare_work_words(1, nscan, npix))
    nwt = -(-npix // 256)
    fwords = nscan * nwt * 4 if nwt > 1 else 0
    pwords = words - fwords
    ops, nbytes = {}, {}
    for name, (raw, b) in settings.items():
        defined = raw.numel() * raw.element_size() + nscan * npix * 4
        for pix in (True, False):
            moved = defined + 2 * 8 * fwords + nscan * 4 * 8 + ((2 * 8 * pwords + 4 * npix * 8) if pix else 0) + npix
            key = "%s, %s" % (name, "maps" if pix else "no maps")
            ops[key] = lambda raw=raw, b=b, pix=pix: pt.prepare_frames(raw, ndet, bin=b, pixels=pix, out=out)
            nbytes[key] = (defined, moved)

    # the device agrees with the host chain it replaces before either is timed (bit for bit: scale 1, even ndet)
    got = pt.prepare_frames(u16[:8], ndet)["data"].cpu().numpy()
    assert np.array_equal(got[0], np.fft.fftshift(u16[:8].cpu().numpy().astype(np.float32), axes=(1, 2)))

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
    lines = ["tools/prepare_time.py on %s: %d positions x %d^2 output pixels; %d blocks of about %g ms per setting after %d "
             "warm-up calls; scratch %d float64 words" % (torch.cuda.get_device_name(0), nscan, ndet, BLOCKS, WINDOW_MS, WARM,
                                                         words),
             "%-36s %6s %10s %9s %9s %11s %9s %12s %10s" % ("setting", "calls", "median ms", "fastest", "slowest",
                                                          "defined GB", "moved GB", "defined TB/s", "moved TB/s")]
    for k, v in times.items():
        defined, moved = nbytes[k]
        lines.append("%-36s %6d %10.4f %9.4f %9.4f %11.3f %9.3f %12.2f %10.2f"
                     % (k, reps[k], med[k], min(v), max(v), defined / 1e9, moved / 1e9, defined / med[k] / 1e9,
                        moved / med[k] / 1e9))

    # end to end from pageable host memory, a host clock to a synchronise
    raw_h = u16.cpu().numpy()
    probe = np.zeros((1, 16, 16), np.complex64)
    probe[0, 8, 8] = 2.0                                                # max |probe| = 2: the host chain divides by 4
    side = int(np.ceil(np.sqrt(nscan)))
    pos = np.stack(np.divmod(np.arange(nscan), side), 1).astype(np.float32)
    rec = {"data": raw_h, "positions_0": pos, "positions_1": pos, "initprobe": probe, "recprobe": probe,
           "detector_pixel_size": 1.0, "detector_distance": 1.0, "incident_wavelength": 16e10, "rotation_angle": 0.0}

    def host_chain():
        ds = PtychoDataset.from_record(rec, view_dims=(side + 1, side + 1))
        return torch.as_tensor(solver_inputs(ds, (side + 1, side + 1))["data"], device="cuda")

    def device_chain():
        return pt.prepare_frames(raw_h, ndet, scale=0.25, out=out)["data"]

    a, b = host_chain(), device_chain()
    same = a.shape == b.shape and bool(torch.equal(a, b))
    del a, b
    t_host, t_dev = host_ms(host_chain), host_ms(device_chain)
    f32_h = f32.cpu().numpy()
    t_dev32 = host_ms(lambda: pt.prepare_frames(f32_h, ndet, scale=0.25, out=out))
    lines += ["end to end from pageable host memory to a synchronise, uint16 frames, median of %d (host clock):" % REPEAT,
              "  host chain (from_record + solver_inputs + copy of float32 data to the device)  %10.1f ms" % t_host,
              "  prepare_frames (copy of the uint16 frames to the device + the pass)             %10.1f ms   (%.1f x)"
              % (t_dev, t_host / t_dev),
              "  prepare_frames on float32 frames from the host (twice the bytes to copy)        %10.1f ms" % t_dev32,
              "  the two chains give the same bits: %s" % same]
    text = "\n".join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
