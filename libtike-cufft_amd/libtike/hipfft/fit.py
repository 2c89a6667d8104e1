"""How well a reconstruction explains the data, frame by frame and detector pixel by detector pixel.

After ``CGPtychoSolver.run`` the questions are which scan positions fit badly (a beam dump, a position far off, a
saturated frame), which detector pixels fit badly (a hot pixel missing from the mask, an incoherent background) and what
the R-factor and the Poisson deviance are.  ``fit_frames`` answers them in one bandwidth-bound pass over the farplane
and the data: eight sums per frame and four maps per angle, all accumulated in float64 in a fixed order (the same inputs
give the same bits), with no farplane-sized temporary.  ``accumulate_intensity`` sums ``|farplane|^2`` over the probe
modes that come before the last one, ``flag_frames`` picks the outliers of a per-frame figure, and
``PtychoHIP.residuals`` drives them from a solver.  Everything runs on the device on the current stream and nothing
synchronises.  Kernels: ``csrc/k_fit.hpp``, C ABI ``ptycho_fit_accumulate`` / ``ptycho_fit_work_words`` /
``ptycho_fit_frames``; DESIGN.md, "Fit residuals", states the definitions in full.

With ``I`` the modelled intensity of a pixel (``I' = I (a / b)^2`` when the probe rescale ``ab`` is given) and ``d`` the
data, the columns of ``frames`` are the sums over the measured pixels of a frame of::

    0  I'                       4  I' - d ln(I' + 1e-32)     (the poisson_ml cost, as logged)
    1  d                        5  d - d ln(d + 1e-32)       (2 * (col 4 - col 5) is the Poisson deviance)
    2  sqrt(I' d)               6  |sqrt I' - sqrt d|
    3  (sqrt I' - sqrt d)^2     7  sqrt d                    (col 6 / col 7 is the amplitude R-factor)

(columns 2 and 0 summed over all frames are ``a`` and ``b`` of the probe rescale, column 3 is the gaussian cost), and the
maps of ``pixels`` are the sums over the frames of an angle of ``I'``, ``d``, ``sqrt I' - sqrt d`` (signed: a background
or a hot pixel shows as a bias) and ``(sqrt I' - sqrt d)^2``.
"""
import numbers

import torch

from . import _native as nat
from ._args import _array, _check_out, _device, _need_array, _opt
from .operators import _ptr, _stream

__all__ = ["fit_frames", "accumulate_intensity", "flag_frames", "check_fit_frames"]


def check_fit_frames(data, farplane=None, intensity=None, mask=None, ab=None):
    """Validate ``fit_frames``'s arguments (no device use); returns ``(ptheta, nscan, ndet)``."""
    shape = _array(data, "data", "float32", (4,))
    if shape[-1] != shape[-2]:
        raise ValueError("data must be [ptheta, nscan, ndet, ndet], got %s" % (shape,))
    if farplane is None and intensity is None:
        raise ValueError("at least one of farplane and intensity must be given")
    if farplane is not None and _array(farplane, "farplane", "complex64", (4,)) != shape:
        raise ValueError("farplane must have data's shape %s, got %s" % (shape, tuple(farplane.shape)))
    if intensity is not None and _array(intensity, "intensity", "float32", (4,)) != shape:
        raise ValueError("intensity must have data's shape %s, got %s" % (shape, tuple(intensity.shape)))
    if mask is not None:
        _need_array(mask, "mask")
        if tuple(int(v) for v in mask.shape) != shape[-2:]:
            raise ValueError("mask must be %s, got shape %s" % (shape[-2:], tuple(mask.shape)))
    if ab is not None and _array(ab, "ab", "float64", (1,)) != (2,):
        raise ValueError("ab must hold the two numbers (a, b), got shape %s" % (tuple(ab.shape),))
    return shape[0], shape[1], shape[2]


def accumulate_intensity(farplane, out=None):
    """``out = |farplane|^2`` (``out=None``: a new float32 tensor of ``farplane``'s shape) or ``out += |farplane|^2``.

    ``|g|^2 = re * re + im * im`` in float32 with every operation rounded, so modes added one after the other equal the
    same statement in NumPy bit for bit.  Returns ``out``; one launch, no synchronisation.
    """
    shape = _array(farplane, "farplane", "complex64", (1, 2, 3, 4))
    if out is not None and _array(out, "out", "float32", (1, 2, 3, 4)) != shape:
        raise ValueError("out must have farplane's shape %s, got %s" % (shape, tuple(out.shape)))
    (g,), dev = _device(farplane)
    add = out is not None
    _check_out(out, dev, "out must be a contiguous tensor on farplane's device")
    if out is None:
        out = torch.empty(shape, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.fit_accumulate(_ptr(out), _ptr(g), g.numel(), int(add), _stream()))
    return out


def fit_frames(data, farplane=None, intensity=None, mask=None, ab=None, pixels=True):
    """Per-frame sums and per-pixel maps of the fit of ``I = intensity + |farplane|^2`` to ``data`` (module docstring).

    ``data`` float32, ``farplane`` complex64, ``intensity`` float32: device tensors ``[ptheta, nscan, ndet, ndet]``, at
    least one of ``farplane`` / ``intensity``.  With one probe mode pass its farplane alone; with ``M`` modes pass the
    last mode's farplane and the ``accumulate_intensity`` of the others.  ``mask``: ``[ndet, ndet]`` in the layout of
    ``data``, nonzero = measured, shared by every frame (``None``: all measured); an unmeasured pixel enters no sum
    whatever the arrays hold there, a non-finite value at a measured pixel propagates.  ``ab``: 2-element float64 device
    tensor ``(a, b)`` of the probe rescale; the intensity is multiplied by ``float32((a / b)^2)``.

    Returns ``{"frames": [ptheta, nscan, 8] float64, "pixels": [ptheta, 4, ndet, ndet] float64}`` (``pixels=False``:
    ``None``, and the same ``frames`` bits).  Bitwise reproducible; two launches, no synchronisation.
    """
    ptheta, nscan, ndet = check_fit_frames(data, farplane, intensity, mask, ab)
    if mask is not None and not isinstance(mask, torch.Tensor) and isinstance(data, torch.Tensor):
        mask = torch.as_tensor(mask).to(data.device)                   # a NumPy mask, as CGPtychoSolver.run takes one
    (d, g, inten, m, ab_), dev = _device(data, farplane, intensity, mask, ab)
    if m is not None:
        m = (m != 0).to(torch.uint8).contiguous()
    npix = ndet * ndet
    words = int(nat.fit_work_words(ptheta, nscan, npix))
    with torch.cuda.device(dev):
        frames = torch.empty((ptheta, nscan, 8), dtype=torch.float64, device=dev)
        maps = torch.empty((ptheta, 4, ndet, ndet), dtype=torch.float64, device=dev) if pixels else None
        work = torch.empty((max(words, 1),), dtype=torch.float64, device=dev)
        nat.check(nat.fit_frames(_ptr(frames), _opt(maps), _opt(inten), _opt(g), _ptr(d), _opt(m), _opt(ab_), ptheta, nscan,
                                 npix, _ptr(work), _stream()))
    return {"frames": frames, "pixels": maps}


def flag_frames(values, nsigma=6.0):
    """Outlier frames of a per-frame figure, e.g. ``fit["frames"][..., 3]``: a bool tensor of ``values``' shape.

    ``values``: ``[ptheta, nscan]``.  Per angle, with ``med`` the median (the lower of the two middle values for an even
    count) and ``MAD`` the median of ``|v - med|``, a frame is flagged when ``|v - med| > nsigma * 1.4826 * MAD``; with
    ``MAD == 0`` every ``v != med`` is.  Plain torch on ``values``' device.
    """
    if not isinstance(values, torch.Tensor) or values.dim() != 2 or 0 in values.shape or not values.is_floating_point():
        raise ValueError("values must be a floating-point tensor [ptheta, nscan], got %s"
                         % (tuple(values.shape) if hasattr(values, "shape") else type(values).__name__,))
    if isinstance(nsigma, bool) or not isinstance(nsigma, numbers.Real) or not float(nsigma) >= 0.0:
        raise ValueError("nsigma must be a non-negative number, got %r" % (nsigma,))
    med = values.median(dim=1, keepdim=True).values
    dev = (values - med).abs()
    mad = dev.median(dim=1, keepdim=True).values
    return dev > float(nsigma) * 1.4826 * mad
