"""Illumination map and gauge fixing of a ptychographic reconstruction.

A solution ``(psi, probe)`` is only defined up to a gauge: one complex factor traded between object and probe, and a
linear phase ramp on the object paired with the opposite ramp on the probe (the intensities do not change); in the
poorly lit border of the scanned area the object means nothing.  This module measures where the object is lit
(``illumination``), fits the gauge of an object inside that region, optionally against a reference object
(``fit_gauge``), and removes it from the object and, with the opposite sign, from the probe (``apply_gauge``);
``fix_gauge`` chains the three.  Everything runs on the device on the current stream and nothing synchronises, so the
calls sit between ``CGPtychoSolver.run`` and ``frc`` in a per-angle pipeline.  Kernels: ``csrc/k_gauge.hpp``, C ABI
``ptycho_illumination`` / ``ptycho_gauge_fit`` / ``ptycho_gauge_apply``; DESIGN.md, "Illumination and gauge", states the
definitions in full.

A gauge is six float64 numbers per angle, ``(gy, gx, phi0, s, yc, xc)``: the ramp in radians per pixel along rows and
columns, the phase at the weighted centre ``(yc, xc)``, and the amplitude scale.
"""
import numbers

import torch

from . import _native as nat
from ._args import _array, _check_out, _device, _opt, _size
from .operators import _ptr, _stream

__all__ = ["illumination", "fit_gauge", "apply_gauge", "fix_gauge"]

WHICH = {"object": 0, "probe": 1}


def check_illumination(scan, probe, nz, n, out=None):
    """Validate ``illumination``'s arguments (no device use); returns ``(ptheta, nscan, nmodes, nprb, nz, n)``."""
    ss = _array(scan, "scan", "float32", (3,))
    ps = _array(probe, "probe", "complex64", (3, 4))
    nz, n = _size(nz, "nz"), _size(n, "n")
    if ss[2] != 2:
        raise ValueError("scan must be [ptheta, nscan, 2], got %s" % (ss,))
    if ps[-1] != ps[-2]:
        raise ValueError("probe must be square, got %s" % (ps,))
    if ps[0] != ss[0]:
        raise ValueError("scan and probe differ in ptheta: %s and %s" % (ss, ps))
    nmodes = ps[1] if len(ps) == 4 else 1
    if out is not None:
        os_ = _array(out, "out", "float32", (3,))
        if os_ != (ss[0], nz, n):
            raise ValueError("out must be %s, got %s" % ((ss[0], nz, n), os_))
    return ss[0], ss[1], nmodes, ps[-1], nz, n


def check_fit(psi, weight=None, ref=None):
    """Validate ``fit_gauge``'s arguments (no device use); returns ``(ptheta, nz, n)``."""
    shape = _array(psi, "psi", "complex64", (2, 3))
    if weight is not None and _array(weight, "weight", "float32", (2, 3)) != shape:
        raise ValueError("weight must have psi's shape %s, got %s" % (shape, tuple(weight.shape)))
    if ref is not None and _array(ref, "ref", "complex64", (2, 3)) != shape:
        raise ValueError("ref must have psi's shape %s, got %s" % (shape, tuple(ref.shape)))
    return (shape[0] if len(shape) == 3 else 1,) + shape[-2:]


def check_apply(x, gauge, which="object"):
    """Validate ``apply_gauge``'s arguments (no device use); returns ``(ptheta, planes per angle, ny, nx, code)``."""
    if which not in WHICH:
        raise ValueError("which must be 'object' or 'probe', got %r" % (which,))
    shape = _array(x, "x", "complex64", (2, 3) if which == "object" else (3, 4))
    gs = _array(gauge, "gauge", "float64", (1, 2))
    ptheta = 1 if len(shape) == 2 else shape[0]
    if gs[-1] != 6 or (len(gs) == 2 and gs[0] != ptheta) or (len(gs) == 1 and ptheta != 1):
        raise ValueError("gauge must be [%d, 6]%s, got %s" % (ptheta, " or [6]" if ptheta == 1 else "", gs))
    return ptheta, shape[1] if len(shape) == 4 else 1, shape[-2], shape[-1], WHICH[which]


def check_fix(psi, scan, probe, floor=0.1, ref=None):
    """Validate ``fix_gauge``'s arguments (no device use); returns ``(ptheta, nz, n)``."""
    ptheta, nz, n = check_fit(psi, None, ref)
    if check_illumination(scan, probe, nz, n)[0] != ptheta:
        raise ValueError("psi and scan differ in ptheta: %s and %s" % (tuple(psi.shape), tuple(scan.shape)))
    if isinstance(floor, bool) or not isinstance(floor, numbers.Real) or not 0.0 <= float(floor) <= 1.0:
        raise ValueError("floor must be in [0, 1], got %r" % (floor,))
    return ptheta, nz, n


def illumination(scan, probe, nz, n, out=None):
    """The diagonal weight with which the object adjoint spreads ``|probe|^2`` over an ``nz x n`` object.

    ``scan``: ``[ptheta, nscan, 2]`` float32 (row, column); ``probe``: ``[ptheta, M, nprb, nprb]`` or
    ``[ptheta, nprb, nprb]`` complex64.  With ``A = sum_m |probe_m|^2`` and each position split by ``modff`` into
    ``(sy, sx) + (fy, fx)``: ``out[t, sy+iy+a, sx+ix+b] += w_ab A[t, iy, ix]`` for the four bilinear taps ``a, b`` of
    the operators.  Positions the operators skip (negative, non-finite, ``>= 1e9``) are skipped, taps outside the object
    are dropped.  Returns a float32 device tensor ``[ptheta, nz, n]`` (``out`` if given: contiguous, written in full).
    Bitwise reproducible; one launch, no synchronisation.
    """
    ptheta, nscan, nmodes, nprb, nz, n = check_illumination(scan, probe, nz, n, out)
    (scan, probe), dev = _device(scan, probe)
    _check_out(out, dev, "out must be a contiguous tensor on the operands' device")
    if out is None:
        out = torch.empty((ptheta, nz, n), dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        nat.check(nat.illumination(_ptr(out), _ptr(scan), _ptr(probe), ptheta, nscan, nmodes, nprb, nz, n, _stream()))
    return out


def fit_gauge(psi, weight=None, ref=None):
    """The gauge ``(gy, gx, phi0, s, yc, xc)`` of ``psi`` (against ``ref`` if given), per angle, as float64 on the device.

    ``psi``, ``ref``: ``[ptheta, nz, n]`` or ``[nz, n]`` complex64; ``weight``: the same shape, float32, ``>= 0``
    (``None``: all ones).  With ``u = psi conj(ref)`` (``u = psi`` without ``ref``), all sums in float64:
    ``gx = arg sum w[y,x] w[y,x+1] u[y,x+1] conj(u[y,x])`` and ``gy`` alike along ``y`` (the wrap-robust phase-gradient
    estimator, good for ``|g| < pi`` rad / pixel), ``(yc, xc)`` the weighted centre,
    ``phi0 = arg sum w u exp(-i (gy (y - yc) + gx (x - xc)))`` and ``s = sqrt(sum w |psi|^2 / sum w |ref|^2)``
    (without ``ref``: ``/ sum w``).  An angle of total weight 0 gets the identity ``(0, 0, 0, 1, 0, 0)``.
    Returns ``[ptheta, 6]`` (``[6]`` for a 2-D ``psi``).  Bitwise reproducible; no synchronisation.
    """
    ptheta, nz, n = check_fit(psi, weight, ref)
    (p, w, r), dev = _device(psi, weight, ref)
    with torch.cuda.device(dev):
        gauge = torch.empty((ptheta, 6), dtype=torch.float64, device=dev)
        work = torch.empty((ptheta, nat.GAUGE_WORK_PER_ANGLE), dtype=torch.float64, device=dev)
        nat.check(nat.gauge_fit(_ptr(gauge), _ptr(p), _opt(r), _opt(w), ptheta, nz, n, _ptr(work), _stream()))
    return gauge[0] if len(psi.shape) == 2 else gauge


def apply_gauge(x, gauge, which="object"):
    """Remove ``gauge`` from ``x`` in place; returns ``x``.

    ``which="object"``: ``x`` is ``[ptheta, nz, n]`` or ``[nz, n]`` and becomes
    ``x exp(-i (phi0 + gy (y - yc) + gx (x - xc))) / s``.  ``which="probe"``: ``x`` is ``[ptheta, M, nprb, nprb]`` or
    ``[ptheta, nprb, nprb]`` and becomes ``x s exp(+i (gy y + gx x))`` in its own coordinates, the companion change that
    keeps every diffraction intensity (exactly at whole-pixel scan positions, up to the interpolation otherwise).
    ``x`` must be a contiguous complex64 device tensor, ``gauge`` float64 ``[ptheta, 6]`` (or ``[6]`` for one angle).
    """
    ptheta, planes, ny, nx, code = check_apply(x, gauge, which)
    (g,), dev = _device(gauge)
    _check_out(x, dev, "x must be a contiguous tensor on the gauge's device")
    g = g.reshape(ptheta, 6)
    if planes > 1:
        g = g.repeat_interleave(planes, dim=0)     # one gauge row per probe mode
    with torch.cuda.device(dev):
        nat.check(nat.gauge_apply(_ptr(x), _ptr(g), ptheta * planes, ny, nx, code, _stream()))
    return x


def fix_gauge(psi, scan, probe, floor=0.1, ref=None):
    """Fit the gauge of ``psi`` on its well-lit region and remove it from copies of ``psi`` and ``probe``.

    The weight of the fit is the illumination where it reaches ``floor`` times its maximum over the angle, zero
    elsewhere.  Without ``ref`` the object comes out with zero mean ramp, zero phase at the lit centre and unit
    weighted RMS amplitude; with ``ref`` (an object of the same shape, e.g. the fixed reconstruction of the other half
    of the data) it comes out in ``ref``'s gauge, which is what ``frc(torch.angle(a), torch.angle(b))`` needs.
    Returns ``{"psi", "probe", "gauge", "illumination", "lit"}``; ``lit`` is the bool mask.  No synchronisation.
    """
    ptheta, nz, n = check_fix(psi, scan, probe, floor, ref)
    ill = illumination(scan, probe, nz, n)
    lit = ill >= float(floor) * torch.amax(ill, dim=(-2, -1), keepdim=True)
    weight = ill * lit
    if len(psi.shape) == 2:
        ill, lit, weight = ill[0], lit[0], weight[0]
    gauge = fit_gauge(psi, weight, ref)
    return {"psi": apply_gauge(psi.clone(memory_format=torch.contiguous_format), gauge, "object"),
            "probe": apply_gauge(probe.clone(memory_format=torch.contiguous_format), gauge, "probe"),
            "gauge": gauge, "illumination": ill, "lit": lit}
