"""Raw detector frames to the inputs of ``CGPtychoSolver.run``, on the device.

``prepare_frames`` takes the frames as the detector wrote them (16- or 32-bit counts or float32, stored centred) and in
one bandwidth-bound pass crops a window around the beam centre, bins it, subtracts the dark frame, multiplies by the
gain, drops bad pixels, clips, scales and moves the centre to ``[0, 0]`` -- the layout of the operators -- while it forms
per-frame and per-pixel statistics (sum, sum of squares, maximum, saturated pixels) in float64 in a fixed order: the same
inputs give the same bits.  It also returns the measured-pixel mask that ``run(mask=)`` takes.  ``initial_probe`` makes a
starting probe from the mean diffraction pattern with the project's own FFT.  Kernels: ``csrc/k_prepare.hpp``, C ABI
``ptycho_prepare_work_words`` / ``ptycho_prepare_frames``; include/ptycho_hip.h and DESIGN.md, "Preparing data", state the
definition in full, and tests/prepare_ref.py restates it in NumPy bit for bit.
"""
import numbers

import numpy as np
import torch

from . import _native as nat
from ._args import _check_out, _device_of, _dtype, _need_array, _opt
from .operators import PtychoHIP, _ptr, _stream

__all__ = ["prepare_frames", "initial_probe", "check_prepare"]

BINS = (1, 2, 4)
MAX_NDET = 32768


def _plane(x, name, dtype, shape):
    if x is None:
        return
    _need_array(x, name)
    if dtype is not None and _dtype(x) != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, _dtype(x)))
    if tuple(int(v) for v in x.shape) != shape:
        raise ValueError("%s must be %s, got shape %s" % (name, shape, tuple(x.shape)))


def _contiguous(x):
    return x.is_contiguous() if isinstance(x, torch.Tensor) else bool(x.flags["C_CONTIGUOUS"])


def check_prepare(raw, ndet, center=None, bin=1, dark=None, gain=None, bad=None, index=None, saturation=None, scale=1.0,
                  out=None):
    """Validate ``prepare_frames``'s arguments (no device use); returns ``(ptheta, nraw, nscan, H, W, y0, x0)``."""
    _need_array(raw, "raw")
    if _dtype(raw) not in nat.PREPARE_DTYPES:
        raise TypeError("raw must be uint16, uint32, int32 or float32, got %s" % _dtype(raw))
    shape = tuple(int(v) for v in raw.shape)
    if len(shape) not in (3, 4) or 0 in shape:
        raise ValueError("raw must be [nraw, H, W] or [ptheta, nraw, H, W] with non-empty axes, got shape %s" % (shape,))
    if not _contiguous(raw):
        raise ValueError("raw must be contiguous")
    ptheta = shape[0] if len(shape) == 4 else 1
    nraw, H, W = shape[-3:]
    if isinstance(ndet, bool) or not isinstance(ndet, numbers.Integral) or not 1 <= ndet <= MAX_NDET:
        raise ValueError("ndet must be an integer in [1, %d], got %r" % (MAX_NDET, ndet))
    if isinstance(bin, bool) or bin not in BINS:
        raise ValueError("bin must be 1, 2 or 4, got %r" % (bin,))
    if center is None:
        center = (H // 2, W // 2)
    try:
        cy, cx = center
        ok = all(isinstance(v, numbers.Integral) and not isinstance(v, bool) and abs(v) <= 2 ** 29 for v in (cy, cx))
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError("center must be two integers (cy, cx) in raw pixels, got %r" % (center,))
    for x, name, dtype in ((dark, "dark", "float32"), (gain, "gain", "float32"), (bad, "bad", None)):
        _plane(x, name, dtype, (H, W))
    nscan = nraw
    if index is not None:
        _need_array(index, "index")
        if _dtype(index) != "int64":
            raise TypeError("index must be int64, got %s" % _dtype(index))
        ishape = tuple(int(v) for v in index.shape)
        if len(ishape) != len(shape) - 2 or 0 in ishape or (len(ishape) == 2 and ishape[0] != ptheta):
            raise ValueError("index must be %s, got shape %s"
                             % ("[nscan]" if len(shape) == 3 else "[%d, nscan]" % ptheta, ishape))
        nscan = ishape[-1]
    if saturation is not None and (isinstance(saturation, bool) or not isinstance(saturation, numbers.Real)
                                   or saturation != saturation):
        raise ValueError("saturation must be a number or None, got %r" % (saturation,))
    if isinstance(scale, bool) or not isinstance(scale, numbers.Real):
        raise ValueError("scale must be a number, got %r" % (scale,))
    if out is not None:
        _plane(out, "out", "float32", (ptheta, nscan, int(ndet), int(ndet)))
    half = int(ndet) // 2
    return ptheta, nraw, nscan, H, W, int(cy) - half * bin, int(cx) - half * bin


def _to_device(x, dev, dtype=None):
    """``x`` (``None``, NumPy or tensor) as a contiguous tensor on ``dev``, in its own dtype unless ``dtype`` is given."""
    if x is None:
        return None
    if not isinstance(x, torch.Tensor):
        x = torch.from_numpy(np.ascontiguousarray(x))
    x = x.to(dev)
    if dtype is not None and x.dtype != dtype:
        x = (x != 0).to(dtype) if dtype == torch.uint8 else x.to(dtype)
    return x.contiguous()


def prepare_frames(raw, ndet, center=None, bin=1, dark=None, gain=None, bad=None, index=None, saturation=None, scale=1.0,
                   clip=True, pixels=True, out=None):
    """Crop, bin, correct and shift raw detector frames into the solver's ``data``, with statistics.

    ``raw``: ``[nraw, H, W]`` or ``[ptheta, nraw, H, W]``, uint16 / uint32 / int32 / float32, contiguous, frames stored
    centred; a device tensor, or a NumPy array that is copied to the current device in its own dtype (no float32 copy
    is made on the host).  ``center = (cy, cx)``: the raw pixel that becomes the centre of the window (default
    ``(H // 2, W // 2)``); the window starts at ``y0 = cy - (ndet // 2) * bin`` and may overhang the frame.  ``bin``: 1,
    2 or 4 raw pixels per output pixel and axis.  ``dark``, ``gain``: float32 ``[H, W]``; ``bad``: ``[H, W]``, nonzero =
    bad.  ``index``: int64 ``[nscan]`` / ``[ptheta, nscan]``: output frame ``j`` is raw frame ``index[j]``; an entry
    outside ``[0, nraw)`` gives a zero frame with zero statistics.  ``saturation``: raw level from which a pixel counts
    as saturated (``None``: no count).

    Centred pixel ``(oy, ox)`` covers the raw pixels ``(y0 + oy * bin + by, x0 + ox * bin + bx)``; it is measured when
    all of them are inside the frame and none is bad.  In float32, each operation rounded: ``t = (raw - dark) * gain``,
    ``v = sum t`` (``by`` outer, ``bx`` inner), ``clip``: ``v = 0 where v < 0`` (a NaN stays), ``v = v * scale``; an
    unmeasured pixel is 0 whatever ``raw``, ``dark`` and ``gain`` hold there.

    Returns device tensors: ``"data"`` float32 ``[ptheta, nscan, ndet, ndet]`` (``out`` if given, written in full), the
    ``ifftshift`` of the centred window; ``"mask"`` uint8 ``[ndet, ndet]`` in the same layout, 1 = measured, the
    argument of ``run(mask=)``; ``"frames"`` float64 ``[ptheta, nscan, 4]``: over the measured pixels of a frame the sum
    of ``v``, the sum of ``v * v``, the maximum (NaN skipped) and the number of saturated raw pixels; ``"pixels"``
    float64 ``[ptheta, 4, ndet, ndet]`` (``pixels=False``: ``None``): the same over the frames of an angle, map 3
    counting the frames in which any raw pixel of the bin was saturated.  Bitwise reproducible; two launches on the
    current stream, no synchronisation.
    """
    ptheta, nraw, nscan, H, W, y0, x0 = check_prepare(raw, ndet, center, bin, dark, gain, bad, index, saturation, scale, out)
    ndet = int(ndet)
    if isinstance(raw, torch.Tensor):
        if not raw.is_cuda:
            raise ValueError("raw must be a device tensor or a NumPy array")
        dev = raw.device
    else:
        dev = _device_of(None, "prepare")
    _check_out(out, dev, "out must be a contiguous tensor on raw's device")
    code = nat.PREPARE_DTYPES[_dtype(raw)]
    npix = ndet * ndet
    words = int(nat.prepare_work_words(ptheta, nscan, npix))
    with torch.cuda.device(dev):
        raw_d = _to_device(raw, dev)
        dark_d, gain_d = _to_device(dark, dev), _to_device(gain, dev)
        bad_d, index_d = _to_device(bad, dev, torch.uint8), _to_device(index, dev)
        data = torch.empty((ptheta, nscan, ndet, ndet), dtype=torch.float32, device=dev) if out is None else out
        mask = torch.empty((ndet, ndet), dtype=torch.uint8, device=dev)
        frames = torch.empty((ptheta, nscan, 4), dtype=torch.float64, device=dev)
        maps = torch.empty((ptheta, 4, ndet, ndet), dtype=torch.float64, device=dev) if pixels else None
        work = torch.empty((max(words, 1),), dtype=torch.float64, device=dev)
        nat.check(nat.prepare_frames(_ptr(data), _ptr(mask), _ptr(frames), _opt(maps), _ptr(raw_d), code, _opt(index_d),
                                     _opt(dark_d), _opt(gain_d), _opt(bad_d), ptheta, nraw, nscan, H, W, y0, x0, int(bin), ndet,
                                     float("nan") if saturation is None else float(saturation), float(scale),
                                     1 if clip else 0, _ptr(work), _stream()))
    return {"data": data, "mask": mask, "frames": frames, "pixels": maps}


def initial_probe(pattern, nprb, power=None):
    """A starting probe from a diffraction pattern: the field whose far field has the pattern's amplitude and zero phase.

    ``pattern``: ``[ptheta, ndet, ndet]`` real, in the layout of ``data`` (a device tensor or a NumPy array), for example
    the mean frame ``prepare_frames(...)["pixels"][:, 0] / nscan``.  The probe is the inverse DFT (``ptycho_fft2``,
    direction +1) of ``sqrt(max(pattern, 0))`` divided by ``ndet``, ``fftshift``-ed and cropped to the central
    ``nprb x nprb`` pixels: with ``nprb == ndet`` the operators give ``|fwd(ones, scan, probe)|^2 == pattern`` in every
    frame.  ``power``: rescale so that ``sum |probe|^2 == power`` per angle.  Returns complex64 ``[ptheta, 1, nprb,
    nprb]`` on the device.  Torch glue around the project's FFT on a temporary handle.
    """
    _need_array(pattern, "pattern")
    shape = tuple(int(v) for v in pattern.shape)
    if len(shape) != 3 or 0 in shape or shape[-1] != shape[-2]:
        raise ValueError("pattern must be [ptheta, ndet, ndet], got shape %s" % (shape,))
    if "complex" in _dtype(pattern):
        raise TypeError("pattern must be real, got %s" % _dtype(pattern))
    ptheta, ndet = shape[0], shape[-1]
    if isinstance(nprb, bool) or not isinstance(nprb, numbers.Integral) or not 1 <= nprb <= ndet:
        raise ValueError("nprb must be an integer in [1, ndet = %d], got %r" % (ndet, nprb))
    if power is not None and (isinstance(power, bool) or not isinstance(power, numbers.Real) or not power > 0):
        raise ValueError("power must be a positive number or None, got %r" % (power,))
    dev = _device_of(pattern, "prepare")
    with torch.cuda.device(dev):
        pat = pattern if isinstance(pattern, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(pattern))
        amp = torch.sqrt(torch.clamp(pat.to(dev).to(torch.float32), min=0.0)).to(torch.complex64).contiguous()
        with PtychoHIP(ptheta, ndet, ndet, 1, ndet + 2, ndet + 2) as op:
            field = op.fft2(amp, inverse=True)
        field = torch.fft.fftshift(field / float(ndet), dim=(-2, -1))
        lo = ndet // 2 - int(nprb) // 2
        probe = field[:, None, lo:lo + int(nprb), lo:lo + int(nprb)].contiguous()
        if power is not None:
            have = (probe.real * probe.real + probe.imag * probe.imag).sum(dim=(1, 2, 3), keepdim=True, dtype=torch.float64)
            probe = probe * torch.sqrt(float(power) / have).to(torch.float32)
    return probe
