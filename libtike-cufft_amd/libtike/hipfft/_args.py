"""Argument checks, operand placement and pointer idioms that the analysis modules (gauge, fit, prepare, unwrap, frc,
propagate, resample, dpc) share."""
import numbers

import numpy as np
import torch

from .operators import _ptr


def _dtype(x):
    return str(getattr(x, "dtype", None)).replace("torch.", "")


def _need_array(x, name):
    if not hasattr(x, "shape") or not hasattr(x, "dtype"):
        raise TypeError("%s must be an array, got %s" % (name, type(x).__name__))


def _array(x, name, dtype, ranks):
    """Shape of ``x`` after the dtype and rank checks (no device use)."""
    _need_array(x, name)
    if _dtype(x) != dtype:
        raise TypeError("%s must be %s, got %s" % (name, dtype, _dtype(x)))
    shape = tuple(int(v) for v in x.shape)
    if len(shape) not in ranks or 0 in shape:
        raise ValueError("%s must have %s non-empty axes, got shape %s"
                         % (name, " or ".join(str(r) for r in ranks), shape))
    return shape


def _size(v, name):
    if isinstance(v, bool) or not isinstance(v, numbers.Integral) or v < 1:
        raise ValueError("%s must be a positive integer, got %r" % (name, v))
    return int(v)


def _device(*tensors):
    """Contiguous device tensors on one device (``None`` passes through); that device."""
    dev = None
    for t in tensors:
        if t is None:
            continue
        if not isinstance(t, torch.Tensor) or not t.is_cuda:
            raise ValueError("libtike.hipfft works on device tensors; there is no CPU path")
        if dev is not None and t.device != dev:
            raise ValueError("operands live on different devices: %s and %s" % (dev, t.device))
        dev = t.device
    return [None if t is None else t.contiguous() for t in tensors], dev


def _opt(t):
    return None if t is None else _ptr(t)


def _check_out(out, dev, message):
    """``out`` is ``None`` or a contiguous tensor on ``dev``, or ``ValueError(message)``."""
    if out is not None and not (isinstance(out, torch.Tensor) and out.is_cuda and out.is_contiguous() and out.device == dev):
        raise ValueError(message)


def _device_of(x, module):
    """``x``'s device if it is a device tensor, else the current one; ``module`` names the caller in the error."""
    if isinstance(x, torch.Tensor) and x.is_cuda:
        return x.device
    if not torch.cuda.is_available():
        raise RuntimeError("libtike.hipfft.%s needs a ROCm GPU; there is no CPU path" % module)
    return torch.device("cuda", torch.cuda.current_device())


def _to_device(arrays, module, message):
    """The operands (device tensors or NumPy arrays, which are copied; ``None`` passes through) as contiguous tensors on
    one device, and that device: the tensors' own, or the current one if there is none.  A host tensor raises
    ``ValueError(message)``; ``module`` names the caller where there is no GPU."""
    dev = None
    for t in arrays:
        if isinstance(t, torch.Tensor):
            if not t.is_cuda:
                raise ValueError(message)
            if dev is not None and t.device != dev:
                raise ValueError("operands live on different devices: %s and %s" % (dev, t.device))
            dev = t.device
    if dev is None:
        dev = _device_of(None, module)
    with torch.cuda.device(dev):
        moved = [None if t is None else
                 (t if isinstance(t, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(t)).to(dev)).contiguous()
                 for t in arrays]
    return moved, dev
