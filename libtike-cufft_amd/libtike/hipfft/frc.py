"""Fourier ring correlation (FRC) of two reconstructions: a resolution estimate that needs no ground truth.

The two images are cropped to a square, windowed, transformed with the project's own FFT, optionally aligned by the
sub-pixel registration of the CG position correction, and correlated ring by ring in frequency (kernels in
``csrc/k_frc.hpp``, C ABI ``ptycho_frc_prepare`` / ``ptycho_frc_rings``).  The curve, the threshold and the crossing are
``O(S)`` per angle and are formed here in float64 from one small copy of the ring sums.  DESIGN.md, "Fourier ring
correlation", states the semantics in full.
"""
import numbers

import numpy as np
import torch

from . import _native as nat
from ._args import _device_of, _opt
from .operators import PtychoHIP, _ptr, _stream
from .registration import register_translation_batch

__all__ = ["frc"]

#: upsampling of the alignment: the CG position correction's
UPSAMPLE = 100
THRESHOLDS = ("half-bit", "one-bit")


def supported_side(s):
    """Crop sides ``ptycho_fft2`` transforms, from 16 up: ``16 <= s <= 1024`` or ``s == 2048``."""
    return 16 <= s <= 1024 or s == 2048


def default_side(m):
    """The largest supported side ``<= m``, or ``None`` below 16."""
    if m >= 2048:
        return 2048
    if m >= 16:
        return min(m, 1024)
    return None


def tukey_window(s, taper):
    """Symmetric Tukey window of length ``s`` and taper fraction ``taper`` in float64
    (``scipy.signal.windows.tukey(s, taper)``: 0 is no window, 1 the Hann window)."""
    if taper <= 0:
        return np.ones(s)
    x = np.arange(s, dtype=np.float64)
    if taper >= 1:
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * x / (s - 1))
    width = int(np.floor(taper * (s - 1) / 2.0))
    w = np.ones(s)
    n1, n3 = x[:width + 1], x[s - width - 1:]
    w[:width + 1] = 0.5 * (1 + np.cos(np.pi * (-1 + 2.0 * n1 / taper / (s - 1))))
    w[s - width - 1:] = 0.5 * (1 + np.cos(np.pi * (-2.0 / taper + 1 + 2.0 * n3 / taper / (s - 1))))
    return w


def threshold_curve(count, threshold):
    """``T_k`` for ring pixel counts ``count``: the half-bit or one-bit curve (van Heel & Schatz 2005), or a constant."""
    r = np.sqrt(np.asarray(count, dtype=np.float64))
    if isinstance(threshold, str):
        if threshold == "half-bit":
            return (0.2071 + 1.9102 / r) / (1.2071 + 0.9102 / r)
        return (0.5 + 2.4142 / r) / (1.5 + 1.4142 / r)
    return np.full(r.shape, float(threshold))


def crossing(curve, thr):
    """First ring ``k >= 1`` where ``curve`` falls below ``thr``, interpolated linearly between ``k - 1`` and ``k``
    (``k_c = 1`` if that is ring 1).  Returns ``(k_c, crossed)``; without a crossing ``(len(curve) - 1, False)``."""
    g = np.asarray(curve, dtype=np.float64) - np.asarray(thr, dtype=np.float64)
    for k in range(1, g.shape[0]):
        if g[k] < 0:
            if k == 1:
                return 1.0, True
            return (k - 1) + g[k - 1] / (g[k - 1] - g[k]), True
    return float(g.shape[0] - 1), False


def curve_from_sums(sums, real, threshold, s):
    """The result dict of ``frc`` (3-D shapes) from the float64 ring sums ``[ptheta, K, 5]`` (Re C, Im C, PA, PB, n)."""
    c = sums[..., 0] + 1j * sums[..., 1]
    pa, pb = sums[..., 2], sums[..., 3]
    count = np.rint(sums[0, :, 4]).astype(np.int64)
    phase = np.zeros(sums.shape[0]) if real else np.angle(c.sum(axis=1))
    num = (np.exp(-1j * phase)[:, None] * c).real
    den = np.sqrt(pa * pb)
    curve = np.where(den > 0, num / np.where(den > 0, den, 1.0), 0.0)
    thr = np.broadcast_to(threshold_curve(count, threshold), curve.shape).copy()
    kc, crossed = zip(*(crossing(curve[t], thr[t]) for t in range(curve.shape[0])))
    kc = np.array(kc)
    return {"frequency": np.arange(s // 2 + 1) / s, "count": count, "frc": curve, "threshold": thr,
            "crossing": kc, "half_period_px": s / (2.0 * kc), "crossed": np.array(crossed), "phase": phase}


def check_arguments(shape, other_shape, region, taper, threshold):
    """Validate ``frc``'s arguments (no device use); returns ``(y0, x0, s)``."""
    shape, other_shape = tuple(shape), tuple(other_shape)
    if shape != other_shape:
        raise ValueError("frc: a and b differ in shape: %s and %s" % (shape, other_shape))
    if len(shape) not in (2, 3) or 0 in shape:
        raise ValueError("frc: images must be [nz, n] or [ptheta, nz, n], got %s" % (shape,))
    nz, n = shape[-2:]
    if region is None:
        s = default_side(min(nz, n))
        if s is None:
            raise ValueError("frc: images of %d x %d are smaller than the smallest crop, 16 x 16" % (nz, n))
        y0, x0 = (nz - s) // 2, (n - s) // 2
    else:
        try:
            y0, x0, s = (int(v) for v in region)
        except (TypeError, ValueError):
            raise ValueError("frc: region must be (y0, x0, S)") from None
        if not supported_side(s):
            raise ValueError("frc: crop side %d not supported (16 <= S <= 1024, or S = 2048)" % s)
        if y0 < 0 or x0 < 0 or y0 + s > nz or x0 + s > n:
            raise ValueError("frc: region %s lies outside the %d x %d image" % ((y0, x0, s), nz, n))
    if isinstance(taper, bool) or not isinstance(taper, numbers.Real) or not 0.0 <= float(taper) <= 1.0:
        raise ValueError("frc: taper must be in [0, 1], got %r" % (taper,))
    if isinstance(threshold, str):
        if threshold not in THRESHOLDS:
            raise ValueError("frc: unknown threshold %r (%s, or a number)" % (threshold, ", ".join(THRESHOLDS)))
    elif isinstance(threshold, bool) or not isinstance(threshold, numbers.Real) or not np.isfinite(threshold):
        raise ValueError("frc: unknown threshold %r (%s, or a number)" % (threshold, ", ".join(THRESHOLDS)))
    return y0, x0, s


def _is_complex(x):
    return x.is_complex() if isinstance(x, torch.Tensor) else np.iscomplexobj(x)


def _upload(x, dev, shape3):
    if not isinstance(x, torch.Tensor):
        x = torch.as_tensor(np.ascontiguousarray(x))
    return x.to(device=dev).to(torch.complex64).reshape(shape3).contiguous()


def frc(a, b, region=None, taper=0.25, align=True, threshold="half-bit"):
    """Fourier ring correlation of ``a`` and ``b`` (two independent reconstructions of the same object).

    ``a``, ``b``: ``[nz, n]`` or ``[ptheta, nz, n]``, torch tensors on the GPU or NumPy arrays; complex inputs are taken
    as complex64, real ones (e.g. ``torch.angle(psi)``) as complex64 with zero imaginary part.
    ``region``: ``(y0, x0, S)``, the crop ``[..., y0:y0+S, x0:x0+S]``, ``16 <= S <= 1024`` or ``S = 2048``; default the
    centred square of the largest supported side ``<= min(nz, n)``.
    ``taper``: Tukey window fraction (0: none, 1: Hann), the window ``w(y) w(x)`` applied to each crop.
    ``align``: register ``b`` onto ``a`` per angle (``register_translation_batch``, upsampling 100, as the CG position
    correction) and shift ``B`` by ``exp(-2 pi i (fy dy + fx dx) / S)``.
    ``threshold``: ``"half-bit"``, ``"one-bit"`` or a constant.

    Per angle and ring ``k = round(|f|) <= S // 2``: ``FRC_k = Re(exp(-i phi) C_k) / sqrt(PA_k PB_k)`` with
    ``C_k = sum A conj(B)``, ``PA_k = sum |A|^2``, ``PB_k = sum |B|^2`` (float64), ``phi = arg sum_k C_k`` for complex
    inputs (the global phase a ptychographic solution leaves free) and 0 for real ones.  The crossing ``k_c`` is the
    first ring ``k >= 1`` where ``FRC_k < T_k``, interpolated from ring ``k - 1``; ``S // 2`` if none crosses.

    Returns a dict of host NumPy values: ``frequency`` (``k / S``), ``count`` (pixels per ring), ``frc`` and
    ``threshold`` (``[ptheta, K]``), ``crossing`` (``k_c``), ``half_period_px`` (``S / (2 k_c)``), ``crossed``,
    ``shift`` (``[ptheta, 2]``, the alignment applied, ``(dy, dx)``) and ``phase`` (``phi``), one per angle.  For 2-D
    inputs the angle axis is dropped from every entry.  The call synchronises once, at the end.
    """
    y0, x0, s = check_arguments(a.shape, b.shape, region, taper, threshold)
    sums, shift = ring_sums(a, b, (y0, x0, s), taper, align)
    res = curve_from_sums(sums, not _is_complex(a) and not _is_complex(b), threshold, s)
    res["shift"] = shift
    if len(a.shape) == 2:
        for key in ("frc", "threshold", "shift"):
            res[key] = res[key][0]
        res["crossing"] = float(res["crossing"][0])
        res["half_period_px"] = float(res["half_period_px"][0])
        res["crossed"] = bool(res["crossed"][0])
        res["phase"] = float(res["phase"][0])
    return res


def ring_sums(a, b, region, taper, align):
    """The device half of ``frc`` for checked arguments: the host float64 ring sums ``[ptheta, K, 5]`` (Re C, Im C, PA,
    PB, n) and the alignment ``[ptheta, 2]``, from one device-to-host copy."""
    y0, x0, s = region
    shape = tuple(a.shape)
    nz, n = shape[-2:]
    ptheta = shape[0] if len(shape) == 3 else 1
    dev = _device_of(a, "frc")
    K = s // 2 + 1
    with torch.cuda.device(dev):
        at, bt = _upload(a, dev, (ptheta, nz, n)), _upload(b, dev, (ptheta, nz, n))
        crops = torch.empty((2, ptheta, s, s), dtype=torch.complex64, device=dev)
        win = None
        if taper > 0:
            win = torch.as_tensor(tukey_window(s, float(taper)).astype(np.float32), device=dev)
        nat.check(nat.frc_prepare(_ptr(crops), _ptr(at), _ptr(bt), ptheta, nz, n, y0, x0, s, _opt(win),
                                  _stream()))
        # a batch of one would meet the registration's "axis of length 1" rule (its shift is set to 0): register
        # every pair in a batch of at least two
        nb = max(ptheta, 2)
        with PtychoHIP(nb, s, s, 1, s + 2, s + 2) as op:
            spec = op.fft2(crops)
            del crops
            shift = torch.zeros((ptheta, 2), dtype=torch.float64, device=dev)
            if align:
                sa, sb = spec[0], spec[1]
                if nb > ptheta:
                    sa, sb = sa.expand(nb, s, s), sb.expand(nb, s, s)
                shift = register_translation_batch(sa, sb, UPSAMPLE, space="fourier", op=op)[:ptheta]
                shift = shift.to(torch.float64).contiguous()
            sums = torch.empty((ptheta, K, 5), dtype=torch.float64, device=dev)
            nat.check(nat.frc_rings(_ptr(sums), _ptr(spec), ptheta, s, _ptr(shift) if align else None, _stream()))
            host = torch.cat((sums.reshape(-1), shift.reshape(-1))).cpu().numpy()
    return host[:ptheta * K * 5].reshape(ptheta, K, 5), host[ptheta * K * 5:].reshape(ptheta, 2)
