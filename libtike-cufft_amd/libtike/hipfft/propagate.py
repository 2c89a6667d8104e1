"""Free-space propagation of probes (or any square complex field) on the device, and the focus series of a probe.

``initial_probe`` returns a probe at focus, and a reconstructed probe sits wherever the sample was: ``propagate`` moves a
field along the beam, ``focus_series`` propagates it through a range of distances and reports, per plane, the figures
that say where it is sharpest and how wide it is there.  Kernels: ``csrc/k_propagate.hpp``, C ABI ``ptycho_propagate``;
include/ptycho_hip.h and DESIGN.md section 16 state the transfer functions and the figures in full, and
tests/propagate_ref.py restates them in NumPy.  Bitwise reproducible.

Typical use::

    probe = propagate(initial_probe(data, nprb), z_sample, wavelength, object_pixel_size(wavelength, L, pix, ndet))
    fs = focus_series(res["probe"][:, 0], np.linspace(-2e-3, 2e-3, 81), wavelength, pixel)   # fs["focus"], fs["width"]

The convolution is circular: a field that spreads beyond its frame wraps around.  ``size=`` pads it (zeros, centred)
to a larger transform side for the call and crops the result.
"""
import numbers

import numpy as np
import torch

from . import _native as nat
from ._args import _device_of, _need_array
from .frc import supported_side
from .operators import PtychoHIP, _ptr, _stream

__all__ = ["propagate", "focus_series", "object_pixel_size", "check_arguments"]

METHODS = tuple(nat.PROPAGATE_METHODS)
#: bytes of planes (or of scratch, for a series without planes) one native call may hold: the distances of a call are
#: chunked to stay below it (one distance per call at the least)
CHUNK_BYTES = 1 << 28


def _positive(v, name):
    if isinstance(v, bool) or not isinstance(v, numbers.Real) or not np.isfinite(v) or not v > 0:
        raise ValueError("%s must be a positive finite number, got %r" % (name, v))
    return float(v)


def object_pixel_size(wavelength, detector_distance, detector_pixel, ndet):
    """Pixel size of the object (and probe) plane of a far-field measurement: ``lambda L / (ndet * pixel)``."""
    lam, dist = _positive(wavelength, "wavelength"), _positive(detector_distance, "detector_distance")
    pix = _positive(detector_pixel, "detector_pixel")
    if isinstance(ndet, bool) or not isinstance(ndet, numbers.Integral) or ndet < 1:
        raise ValueError("ndet must be a positive integer, got %r" % (ndet,))
    return lam * dist / (int(ndet) * pix)


def check_arguments(field, distance, wavelength, pixel_size, method="fresnel", size=None):
    """Validate the arguments of ``propagate`` / ``focus_series`` (no device use).

    Returns ``(s, S, z, scalar)``: the field's side, the transform side, the distances as a float64 vector and whether
    ``distance`` was a scalar."""
    _need_array(field, "field")
    if "complex" not in str(field.dtype):
        raise TypeError("field must be complex, got %s" % (field.dtype,))
    shape = tuple(int(v) for v in field.shape)
    if len(shape) < 2 or shape[-1] != shape[-2] or 0 in shape:
        raise ValueError("field must be [..., s, s] with non-empty axes, got shape %s" % (shape,))
    s = shape[-1]
    if method not in METHODS:
        raise ValueError("unknown method %r (%s)" % (method, ", ".join(METHODS)))
    _positive(wavelength, "wavelength")
    _positive(pixel_size, "pixel_size")
    scalar = isinstance(distance, numbers.Real) and not isinstance(distance, bool)
    try:
        z = np.atleast_1d(np.asarray(distance, dtype=np.float64))
    except (TypeError, ValueError):
        raise TypeError("distance must be a number or a sequence of numbers, got %r" % (distance,)) from None
    if z.ndim != 1 or z.size == 0:
        raise ValueError("distance must be a number or a non-empty sequence of numbers, got shape %s" % (z.shape,))
    if not np.all(np.isfinite(z)):
        raise ValueError("every distance must be finite")
    if size is None:
        if not supported_side(s):
            raise ValueError("field side %d is not a transform side (16 <= S <= 1024, or S = 2048): pad it with size=" % s)
        big = s
    else:
        if isinstance(size, bool) or not isinstance(size, numbers.Integral):
            raise TypeError("size must be an integer, got %r" % (size,))
        big = int(size)
        if big < s:
            raise ValueError("size=%d is smaller than the field's side %d" % (big, s))
        if not supported_side(big):
            raise ValueError("size=%d is not a transform side (16 <= S <= 1024, or S = 2048)" % big)
    return s, big, z, scalar


def parabola_vertex(x, y):
    """Abscissa of the vertex of the parabola through three points, or ``None`` if they have no maximum."""
    (y0, y1, y2), mid = y, x[1]
    x0, x2 = x[0] - mid, x[2] - mid   # about the middle point: y = y1 + b x + a x^2
    den = x0 * x2 * (x0 - x2)
    if den == 0:
        return None
    a = (x2 * (y0 - y1) - x0 * (y2 - y1)) / den
    b = (x0 * x0 * (y2 - y1) - x2 * x2 * (y0 - y1)) / den
    if not a < 0 or not np.isfinite(b):
        return None
    return mid - b / (2.0 * a)


def _series(field, z, wavelength, pixel_size, method, s, big, want_planes, want_metrics):
    """The device half for checked arguments: ``(planes, metrics)`` on the device, ``[nf, D, S, S]`` complex64 and
    ``[nf, D, 8]`` float64 (``None`` where not wanted), ``nf`` the product of the field's batch axes."""
    dev = _device_of(field, "propagate")
    nf = int(np.prod(field.shape[:-2], dtype=np.int64))
    nd = z.shape[0]
    lo = (big - s) // 2
    q0 = (float(wavelength) / (big * float(pixel_size))) ** 2
    with torch.cuda.device(dev):
        if not isinstance(field, torch.Tensor):
            field = torch.as_tensor(np.ascontiguousarray(field))
        u = field.to(device=dev).to(torch.complex64).reshape(nf, s, s)
        if big != s:
            padded = torch.zeros((nf, big, big), dtype=torch.complex64, device=dev)
            padded[:, lo:lo + s, lo:lo + s] = u
            u = padded
        zl = torch.as_tensor(z / float(wavelength), dtype=torch.float64, device=dev)
        per = max(1, min(nd, CHUNK_BYTES // (nf * big * big * 8)))
        planes = torch.empty((nf, nd, big, big), dtype=torch.complex64, device=dev) if want_planes else None
        parts = []
        with PtychoHIP(nf, big, big, 1, big + 2, big + 2) as op:
            spec = op.fft2(u.contiguous())
            for d0 in range(0, nd, per):
                n = min(per, nd - d0)
                whole = want_planes and n == nd
                chunk = planes if whole else (torch.empty((nf, n, big, big), dtype=torch.complex64, device=dev)
                                              if want_planes else None)
                words = 0 if want_planes else int(nat.propagate_work_words(op._h, nf, n, 0))
                work = torch.empty(max(words, 2), dtype=torch.float64, device=dev)
                met = torch.empty((nf, n, nat.PROPAGATE_WORDS), dtype=torch.float64, device=dev) if want_metrics else None
                nat.check(nat.propagate(op._h, None if chunk is None else _ptr(chunk), None if met is None else _ptr(met),
                                        _ptr(spec), nf, _ptr(zl[d0:d0 + n]), n, q0, nat.PROPAGATE_METHODS[method], _ptr(work),
                                        _stream()))
                if want_planes and not whole:
                    planes[:, d0:d0 + n] = chunk
                if want_metrics:
                    parts.append(met)
        metrics = None
        if want_metrics:
            metrics = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
    return planes, metrics


def propagate(field, distance, wavelength, pixel_size, method="fresnel", size=None):
    """``field`` propagated by ``distance`` along the beam: a complex64 device tensor.

    ``field``: ``[..., s, s]`` complex, a device tensor or a NumPy array; every leading axis is batch, so probes
    ``[ptheta, M, nprb, nprb]`` go in as they are.  ``distance``: a number (the result has ``field``'s shape) or a
    sequence (an axis of that length is added before the last two).  ``wavelength``, ``pixel_size`` (of the field's
    plane) and the distances share one length unit.  ``method``: ``"fresnel"`` (paraxial transfer function) or
    ``"angular"`` (angular spectrum with the carrier ``exp(2 pi i z / lambda)`` removed; evanescent frequencies are
    set to zero for either sign of ``z``).  ``size``: transform side ``S >= s``: the field is zero-padded, centred at
    ``(S - s) // 2``, and the result is the cropped view; default ``S = s``.

    ``plane = IDFT(DFT(field) H)``, ``H = exp(2 pi i t)`` with ``t = -(z / lambda) q / 2`` (fresnel) or
    ``-(z / lambda) q / (1 + sqrt(1 - q))`` (angular), ``q = (lambda / (S p))^2 (ky^2 + kx^2)``; the phase is reduced
    in float64, the transforms are the project's own in complex64.  ``distance = 0`` returns the field."""
    s, big, z, scalar = check_arguments(field, distance, wavelength, pixel_size, method, size)
    planes, _ = _series(field, z, wavelength, pixel_size, method, s, big, True, False)
    lo = (big - s) // 2
    batch = tuple(field.shape[:-2])
    out = planes[:, :, lo:lo + s, lo:lo + s].reshape(batch + (z.shape[0], s, s))
    return out[..., 0, :, :] if scalar else out


def focus_series(field, distances, wavelength, pixel_size, method="fresnel", size=None, planes=False):
    """Figures of ``field`` propagated to every one of ``distances``: where it is sharpest and how wide it is there.

    Arguments as for ``propagate``.  With ``v = |plane|^2`` (float32) summed in float64 over the transform's ``S x S``
    frame, returns a dict of host float64 arrays, ``[..., D]`` over the field's batch axes and the distances:

    ``power`` (``sum v``), ``sharpness`` (``sum v^2 / (sum v)^2``), ``peak`` (``max v``), ``peak_index`` (``[..., D, 2]``,
    ``(y, x)`` of the first maximum), ``centroid`` (``[..., D, 2]``, ``(y, x)``), ``width`` (the rms radius
    ``sqrt(var_y + var_x)`` in pixels); indices and centroids are in the field's own coordinates whatever ``size`` is.
    Per field (``[...]``): ``best`` (arg-max of sharpness), ``focus`` (the vertex of the parabola through the sharpness
    at ``best - 1, best, best + 1`` over the distances; ``distances[best]`` where ``best`` is an end of the range or the
    three points have no maximum) and ``bracketed`` (whether the parabola was used).  Per distance (``[D]``):
    ``distance`` and ``sampled`` (``|z| <= S p^2 / lambda``, the Nyquist limit of the Fresnel kernel's phase).
    ``planes=True`` adds ``planes``, the complex64 device tensor ``[..., D, s, s]``.

    Without ``planes`` no plane reaches memory on the sides whose tile fits a compute unit (16 ... 128 with a plan); the
    distances are processed ``CHUNK_BYTES`` of planes or scratch at a time, and the figures come back in one copy."""
    s, big, z, _ = check_arguments(field, distances, wavelength, pixel_size, method, size)
    if not isinstance(planes, (bool, np.bool_)):
        raise TypeError("planes must be a bool, got %r" % (planes,))
    out_planes, metrics = _series(field, z, wavelength, pixel_size, method, s, big, bool(planes), True)
    lo = (big - s) // 2
    batch = tuple(field.shape[:-2])
    nd = z.shape[0]
    m = metrics.cpu().numpy().reshape(batch + (nd, nat.PROPAGATE_WORDS))
    res = figures(m, z, big, lo)
    res["sampled"] = np.abs(z) <= big * float(pixel_size) ** 2 / float(wavelength)
    if planes:
        res["planes"] = out_planes[:, :, lo:lo + s, lo:lo + s].reshape(batch + (nd, s, s))
    return res


def figures(m, z, big, lo):
    """The result dict of ``focus_series`` from the host metrics ``[..., D, 8]`` (no device use)."""
    with np.errstate(divide="ignore", invalid="ignore"):
        power = m[..., 0]
        sharp = m[..., 1] / (power * power)
        cy, cx = m[..., 2] / power, m[..., 3] / power
        var = (m[..., 4] / power - cy * cy) + (m[..., 5] / power - cx * cx)
        width = np.sqrt(np.maximum(var, 0.0))
    idx = m[..., 7]
    found = idx >= 0
    iy = np.where(found, np.floor_divide(idx, big) - lo, -1.0)
    ix = np.where(found, np.mod(idx, big) - lo, -1.0)
    batch = m.shape[:-2]
    nd = z.shape[0]
    flat = np.where(np.isnan(sharp), -np.inf, sharp).reshape(-1, nd)
    best = flat.argmax(axis=1)
    focus, bracketed = np.empty(best.shape), np.zeros(best.shape, dtype=bool)
    for k, b in enumerate(best):
        focus[k] = z[b]
        if 0 < b < nd - 1:
            v = parabola_vertex(z[b - 1:b + 2], flat[k, b - 1:b + 2])
            if v is not None:
                focus[k], bracketed[k] = v, True
    return {"distance": z.copy(), "power": power, "sharpness": sharp, "peak": m[..., 6],
            "peak_index": np.stack((iy, ix), axis=-1), "centroid": np.stack((cy - lo, cx - lo), axis=-1),
            "width": width, "best": best.reshape(batch), "focus": focus.reshape(batch),
            "bracketed": bracketed.reshape(batch)}
