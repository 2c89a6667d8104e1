"""Time of the scan-position gradient (adj_scan) at 4096 x 256^2, nprb 64 and 256, against three baselines on the same
inputs: adj_probe, the inverse fft2 of the farplane alone, and a device copy of the farplane.

    python tools/scan_grad_time.py [repeats] > profiles/r18/scan_grad.txt

Device events around `repeats` calls after three warm-up calls; the median of five such windows.  Bytes: what each call
must move at least (the farplane is 2 GiB: it is read once; adj_scan writes its tiles once more and reads their centre
nprb x nprb crop)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "libtike-cufft_amd")]
import torch  # noqa: E402
import libtike.hipfft as pt  # noqa: E402
from libtike.hipfft import synthetic as syn  # noqa: E402


def window_ms(call, repeats):
    for _ in range(3):
        call()
    times = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(repeats):
            call()
        b.record()
        torch.cuda.synchronize()
        times.append(a.elapsed_time(b) / repeats)
    return sorted(times)


def main():
    repeats = int(sys.argv[1]) if len(sys.argv) > 1 else 10
    ndet = 256
    print("adj_scan at 4096 positions x %d^2, %s, %d calls per window, 5 windows (ms: min / median / max)"
          % (ndet, torch.cuda.get_device_name(0), repeats))
    for nprb in (64, 256):
        p = syn.make_problem(64, 64, 8, nprb, ndet, seed=1234)
        D = lambda x: torch.as_tensor(x, device="cuda")
        with pt.PtychoCuFFT(p["nscan"], nprb, ndet, 1, p["nz"], p["n"]) as slv:
            psi, scan, prb = D(p["psi"]), D(p["scan"]), D(p["probe"])
            g = slv.fwd(psi, scan, prb)
            gib = g.numel() * 8 / 2.0 ** 30
            other = torch.empty_like(g)
            out = torch.empty((1, p["nscan"], 2), dtype=torch.float32, device="cuda")
            chunk = max(1, (256 << 20) // (ndet * ndet * 8))
            work = torch.empty((chunk, ndet, ndet), dtype=torch.complex64, device="cuda")
            own = (2 + (nprb / ndet) ** 2) * gib
            rows = [("adj_scan (chunk=None: %d tiles)" % chunk, lambda: slv.adj_scan(g, scan, psi, prb, out=out), own),
                    ("adj_scan (chunk=4096)", lambda: slv.adj_scan(g, scan, psi, prb, out=out, chunk=4096), own),
                    ("adj_probe", lambda: slv.adj_probe(g, scan, psi), gib),
                    ("fft2 inverse, whole farplane", lambda: slv.fft2(g, inverse=True, out=other), 2 * gib),
                    ("fft2 inverse, %d-tile pieces" % chunk,
                     lambda: [slv.fft2(g[0, k:k + chunk], inverse=True, out=work[:min(chunk, p["nscan"] - k)])
                              for k in range(0, p["nscan"], chunk)], 2 * gib),
                    ("device copy of the farplane", lambda: other.copy_(g), 2 * gib)]
            print("nprb %d (object %d x %d, farplane %.2f GiB)" % (nprb, p["nz"], p["n"], gib))
            for name, call, moved in rows:
                t = window_ms(call, repeats)
                print("  %-40s %8.3f / %8.3f / %8.3f ms   %6.2f TB/s of %.2f GiB at the median"
                      % (name, t[0], t[2], t[-1], moved * 2.0 ** 30 / (t[2] * 1e-3) / 1e12, moved))
            del g, other, work
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
