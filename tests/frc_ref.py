"""Float64 NumPy restatement of ``libtike.hipfft.frc`` (steps 1-11 of DESIGN.md, "Fourier ring correlation"), written
from the definition and independent of the library's host code: the window from the textbook Tukey formula, the rings
from ``rint(sqrt(r2))``, the sums by ``bincount``, the crossing vectorised.  Step 5 is the CPU oracle's
``register_translation_batch`` (every pair registered in a batch of at least two, as ``frc`` does).

``precision="single"`` evaluates the crops, the window and the spectra in float32 / complex64 (the sums stay float64): its
distance from the float64 evaluation sizes the tolerances of ``tests/test_hip_frc.py``.
"""
import numpy as np

from oracle.cg_oracle import register_translation_batch

UPSAMPLE = 100


def tukey(s, taper):
    """Symmetric Tukey window: 1 in the middle, raised-cosine flanks of total fraction ``taper``."""
    x = np.arange(s) / (s - 1.0)
    w = np.ones(s)
    if taper <= 0:
        return w
    lo, hi = x < taper / 2, x > 1 - taper / 2
    w[lo] = 0.5 * (1 + np.cos(2 * np.pi / taper * (x[lo] - taper / 2)))
    w[hi] = 0.5 * (1 + np.cos(2 * np.pi / taper * (x[hi] - 1 + taper / 2)))
    return w


def freqs(s):
    return np.rint(np.fft.fftfreq(s) * s).astype(np.int64)


def rings(s):
    """Ring index of every pixel of an ``s x s`` spectrum, ``rint(sqrt(fy^2 + fx^2))``."""
    f = freqs(s)
    return np.rint(np.sqrt(f[:, None] ** 2 + f[None, :] ** 2)).astype(np.int64)


def threshold(count, kind):
    n = np.sqrt(np.asarray(count, dtype=np.float64))
    if kind == "half-bit":
        return (0.2071 + 1.9102 / n) / (1.2071 + 0.9102 / n)
    if kind == "one-bit":
        return (0.5 + 2.4142 / n) / (1.5 + 1.4142 / n)
    return np.full(n.shape, float(kind))


def crossing(curve, thr):
    g = curve - thr
    below = np.nonzero(g[1:] < 0)[0]
    if below.size == 0:
        return float(len(curve) - 1), False
    k = int(below[0]) + 1
    return (1.0 if k == 1 else (k - 1) + g[k - 1] / (g[k - 1] - g[k])), True


def spectra(a, b, y0, x0, s, taper, precision="double"):
    ctype = np.complex128 if precision == "double" else np.complex64
    win = np.outer(tukey(s, taper), tukey(s, taper)).astype(ctype().real.dtype)
    ca = a[:, y0:y0 + s, x0:x0 + s].astype(ctype) * win
    cb = b[:, y0:y0 + s, x0:x0 + s].astype(ctype) * win
    return np.fft.fft2(ca).astype(ctype), np.fft.fft2(cb).astype(ctype)


def register(A, B):
    p = A.shape[0]
    if p == 1:
        A, B = np.concatenate([A, A]), np.concatenate([B, B])
    return register_translation_batch(A, B, UPSAMPLE, space="fourier")[:p]


def ring_sums(A, B, shift):
    """``[ptheta, K, 5]``: Re C, Im C, PA, PB, n per ring, ``B`` shifted by ``exp(-2 pi i (fy dy + fx dx) / S)``."""
    ptheta, s = A.shape[0], A.shape[-1]
    K = s // 2 + 1
    k = rings(s).ravel()
    keep = k <= s // 2
    f = freqs(s).astype(np.float64)
    out = np.zeros((ptheta, K, 5))
    for t in range(ptheta):
        ramp = np.exp(-2j * np.pi * (f[:, None] * shift[t, 0] + f[None, :] * shift[t, 1]) / s)
        a = A[t].astype(np.complex128).ravel()[keep]
        bb = (B[t].astype(np.complex128) * ramp).ravel()[keep]
        c = a * bb.conj()
        kk = k[keep]
        out[t, :, 0] = np.bincount(kk, c.real, K)
        out[t, :, 1] = np.bincount(kk, c.imag, K)
        out[t, :, 2] = np.bincount(kk, np.abs(a) ** 2, K)
        out[t, :, 3] = np.bincount(kk, np.abs(bb) ** 2, K)
        out[t, :, 4] = np.bincount(kk, None, K)
    return out


def curve(sums, real, kind, s):
    c = sums[..., 0] + 1j * sums[..., 1]
    pp = sums[..., 2] * sums[..., 3]
    phase = np.zeros(sums.shape[0]) if real else np.angle(c.sum(axis=1))
    frc = np.zeros(pp.shape)
    ok = pp > 0
    frc[ok] = (np.exp(-1j * phase)[:, None] * c).real[ok] / np.sqrt(pp[ok])
    thr = np.tile(threshold(sums[0, :, 4], kind), (sums.shape[0], 1))
    kc, crossed = map(np.array, zip(*(crossing(frc[t], thr[t]) for t in range(frc.shape[0]))))
    return {"frequency": np.arange(s // 2 + 1) / s, "count": sums[0, :, 4].astype(np.int64), "frc": frc,
            "threshold": thr, "crossing": kc, "half_period_px": s / (2 * kc), "crossed": crossed, "phase": phase}


def frc(a, b, region=None, taper=0.25, align=True, threshold="half-bit", precision="double", shift=None):
    """The restatement; 3-D result shapes always (a 2-D input is one angle), plus ``sums``.  ``shift``: use this
    ``[ptheta, 2]`` alignment instead of registering (to compare sums at the device's shift)."""
    a, b = np.asarray(a), np.asarray(b)
    real = not np.iscomplexobj(a) and not np.iscomplexobj(b)
    if a.ndim == 2:
        a, b = a[None], b[None]
    nz, n = a.shape[-2:]
    if region is None:
        m = min(nz, n)
        s = 2048 if m >= 2048 else min(m, 1024)
        y0, x0 = (nz - s) // 2, (n - s) // 2
    else:
        y0, x0, s = region
    A, B = spectra(a, b, y0, x0, s, taper, precision)
    if shift is None:
        shift = register(A, B) if align else np.zeros((a.shape[0], 2))
    sums = ring_sums(A, B, np.asarray(shift, dtype=np.float64))
    res = curve(sums, real, threshold, s)
    res["shift"] = np.asarray(shift, dtype=np.float64)
    res["sums"] = sums
    return res
