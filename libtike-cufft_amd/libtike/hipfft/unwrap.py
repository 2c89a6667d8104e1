"""Weighted least-squares phase unwrapping of a reconstruction, on the device.

The phase of a reconstructed object comes wrapped into ``(-pi, pi]``; a projection for tomography needs it unwrapped, and
the unlit border of the object is noise that must not steer the result.  ``unwrap_phase`` solves the weighted
least-squares problem of Ghiglia & Romero (1994) -- find ``x`` whose neighbour differences match the wrapped differences
of the phase, each edge weighted by the smaller weight of its two pixels -- with Jacobi-preconditioned conjugate
gradients on the pixel grid: no transform of the object's size, any rectangular shape, and weights.  ``phase_residues``
maps the residues (the loops around which the wrapped differences do not sum to zero).  Kernels: ``csrc/k_unwrap.hpp``,
C ABI ``ptycho_unwrap_*``; include/ptycho_hip.h and DESIGN.md section 15 state the definition in full, and
tests/unwrap_ref.py restates it in NumPy.  Bitwise reproducible.

Typical use, after ``fix_gauge`` has removed the ramp and the offset::

    fa = fix_gauge(psi, scan, probe)
    projection = unwrap_phase(fa["psi"], weight=fa["lit"])["phase"]
"""
import numbers

import numpy as np
import torch

from . import _native as nat
from ._args import _check_out, _dtype, _need_array, _opt, _to_device
from .operators import _ptr, _stream

__all__ = ["unwrap_phase", "phase_residues", "check_unwrap"]

PHASE_DTYPES = ("float32", "float64", "float16", "complex64")
WEIGHT_DTYPES = ("float32", "bool")
STATUS = {0: "running", 1: "converged", 2: "breakdown", 3: "maxiter"}


def _shape(x, name, dtypes):
    _need_array(x, name)
    if _dtype(x) not in dtypes:
        raise TypeError("%s must be %s, got %s" % (name, " or ".join(dtypes), _dtype(x)))
    return tuple(int(v) for v in x.shape)


def check_unwrap(x, weight=None, congruent=True, tol=1e-4, maxiter=None, check_every=256, out=None):
    """Validate ``unwrap_phase``'s arguments (no device use); returns ``(ptheta, nz, n, maxiter)``."""
    shape = _shape(x, "x", PHASE_DTYPES)
    if len(shape) not in (2, 3):
        raise ValueError("x must be [nz, n] or [ptheta, nz, n], got shape %s" % (shape,))
    ptheta = shape[0] if len(shape) == 3 else 1
    nz, n = shape[-2:]
    if nz < 2 or n < 2 or nz * n >= 2 ** 31 or not 1 <= ptheta <= 65535:
        raise ValueError("x needs nz >= 2, n >= 2, nz * n < 2^31 and ptheta in [1, 65535], got shape %s" % (shape,))
    if weight is not None and _shape(weight, "weight", WEIGHT_DTYPES) != shape:
        raise ValueError("weight must have x's shape %s, got %s" % (shape, tuple(weight.shape)))
    if not isinstance(congruent, (bool, np.bool_)):
        raise TypeError("congruent must be a bool, got %r" % (congruent,))
    if isinstance(tol, bool) or not isinstance(tol, numbers.Real) or not 0.0 <= float(tol) < float("inf"):
        raise ValueError("tol must be a finite number >= 0, got %r" % (tol,))
    if maxiter is None:
        maxiter = 8 * max(nz, n)
    elif isinstance(maxiter, bool) or not isinstance(maxiter, numbers.Integral) or not 0 <= maxiter < 2 ** 31:
        raise ValueError("maxiter must be an integer in [0, 2^31) or None, got %r" % (maxiter,))
    if isinstance(check_every, bool) or not isinstance(check_every, numbers.Integral) or not 1 <= check_every < 2 ** 31:
        raise ValueError("check_every must be a positive integer, got %r" % (check_every,))
    if out is not None and _shape(out, "out", ("float32",)) != shape:
        raise ValueError("out must have x's shape %s, got %s" % (shape, tuple(out.shape)))
    return ptheta, nz, n, int(maxiter)


def _on_device(x, weight):
    """``x`` as contiguous float32 phase and ``weight`` as contiguous float32 (or ``None``) on one device; that device."""
    (xd, weight), dev = _to_device((x, weight), "unwrap", "x and weight must be device tensors or NumPy arrays")
    with torch.cuda.device(dev):
        phase = torch.angle(xd) if xd.is_complex() else xd
        phase = phase.to(torch.float32).contiguous()
        if isinstance(x, torch.Tensor) and phase.data_ptr() == x.data_ptr():
            phase = phase.clone()                      # never alias the caller's array: out= may be x itself
        if weight is not None:
            weight = weight.to(torch.float32).contiguous()
    return phase, weight, dev


def unwrap_phase(x, weight=None, congruent=True, tol=1e-4, maxiter=None, check_every=256, out=None):
    """Unwrap the phase ``x`` by weighted least squares; only multiples of ``2 pi`` are changed (``congruent=True``).

    ``x``: ``[nz, n]`` or ``[ptheta, nz, n]``, a device tensor or a NumPy array; complex input is taken as
    ``torch.angle(x)``, real input as float32 phase.  ``weight``: the same shape, float32 or bool, e.g.
    ``fix_gauge(...)["lit"]`` or ``illumination(...)``; a weight that is not positive and finite counts as 0, ``None``
    as all ones.  An edge between two neighbours weighs the smaller of their weights; an edge of weight 0 contributes
    nothing, whatever the phase holds at its ends (NaN and Inf included).

    The solver minimises ``sum_e w_e (x_q - x_p - W(phi_q - phi_p))^2`` by preconditioned conjugate gradients from
    ``x = 0`` until ``r.z <= tol^2 r0.z0`` or ``maxiter`` iterations (``None``: ``8 max(nz, n)``); it needs
    ``O(max(nz, n))`` iterations.  Then one constant ``c`` per angle aligns ``x`` with the phase and
    ``congruent=True`` returns ``phi + 2 pi rint((x + c - phi) / 2 pi)``, ``congruent=False`` the smooth ``x + c``.  A
    pixel without a weighted edge keeps its phase.  ``c`` is one constant per angle: if the pixels of positive weight
    fall into several disconnected regions, each is unwrapped up to its own constant and only one of them can be made
    congruent reliably -- use ``congruent=False`` or one call per region.

    ``check_every`` iterations are enqueued at a time and the state is read back once per block, the only
    synchronisation; the loop ends when every angle has stopped.  Returns a dict: ``"phase"`` (float32 on the device,
    ``out`` if given: contiguous, written in full) and per angle on the host ``"iterations"``, ``"residual"``
    (``sqrt(r.z / r0.z0)``), ``"converged"``, ``"status"`` (1 converged, 2 breakdown, 3 maxiter), ``"offset"`` (``c``)
    and ``"residues"`` (the number of residues among the loops of positive weight).  For 2-D input the angle axis is
    dropped.  Bitwise reproducible.
    """
    ptheta, nz, n, maxiter = check_unwrap(x, weight, congruent, tol, maxiter, check_every, out)
    phase, w, dev = _on_device(x, weight)
    _check_out(out, dev, "out must be a contiguous tensor on the operands' device")
    with torch.cuda.device(dev):
        buf = torch.empty((int(nat.unwrap_buffer_floats(ptheta, nz, n)),), dtype=torch.float32, device=dev)
        work = torch.empty((int(nat.unwrap_work_words(ptheta, nz, n)),), dtype=torch.float64, device=dev)
        state = torch.empty((ptheta, nat.UNWRAP_STATE_WORDS), dtype=torch.float64, device=dev)
        count = torch.empty((ptheta,), dtype=torch.int64, device=dev)
        res = torch.empty((ptheta, nz, n), dtype=torch.float32, device=dev) if out is None else out
        sizes = (ptheta, nz, n)
        nat.check(nat.unwrap_residues(None, _ptr(count), _ptr(phase), _opt(w), *sizes, _stream()))
        nat.check(nat.unwrap_begin(_ptr(buf), _ptr(state), _ptr(phase), _opt(w), *sizes, _ptr(work), _stream()))
        done = 0
        while True:
            niter = min(int(check_every), maxiter - done)
            nat.check(nat.unwrap_iterate(_ptr(buf), _ptr(state), _opt(w), *sizes, niter, maxiter, float(tol), _ptr(work),
                                         _stream()))
            done += niter
            host = state.cpu()                          # the only synchronisation of the loop
            if bool((host[:, nat.UNWRAP_STATUS] != 0).all()) or done >= maxiter:
                break
        nat.check(nat.unwrap_finish(_ptr(res), _ptr(state), _ptr(buf), _ptr(phase), _opt(w), 1 if congruent else 0, *sizes,
                                    _ptr(work), _stream()))
        host = state.cpu().numpy()
        counts = count.cpu().numpy()
    status = host[:, nat.UNWRAP_STATUS].astype(np.int64)
    info = {"iterations": host[:, nat.UNWRAP_ITER].astype(np.int64), "residual": host[:, nat.UNWRAP_RELRES].copy(),
            "converged": status == 1, "status": status, "offset": host[:, nat.UNWRAP_C].copy(), "residues": counts}
    if len(x.shape) == 2:
        res = res if out is not None else res[0]
        info = {k: v[0].item() for k, v in info.items()}
    info["phase"] = res
    return info


def phase_residues(x, weight=None):
    """The residue charges of the phase ``x``: int8 ``[ptheta, nz - 1, n - 1]`` (``[nz - 1, n - 1]`` for 2-D input) on the
    device.  Loop ``(y, x)`` runs ``(y, x) -> (y, x+1) -> (y+1, x+1) -> (y+1, x) -> (y, x)``; its charge is the sum of the
    four wrapped differences over ``2 pi``, in ``{-1, 0, 1}``, and 0 unless all four pixels have positive weight.
    ``x`` and ``weight`` as in ``unwrap_phase``.  One launch, no synchronisation."""
    ptheta, nz, n, _ = check_unwrap(x, weight)
    phase, w, dev = _on_device(x, weight)
    with torch.cuda.device(dev):
        charge = torch.empty((ptheta, nz - 1, n - 1), dtype=torch.int8, device=dev)
        count = torch.empty((ptheta,), dtype=torch.int64, device=dev)
        nat.check(nat.unwrap_residues(_ptr(charge), _ptr(count), _ptr(phase), _opt(w), ptheta, nz, n, _stream()))
    return charge[0] if len(x.shape) == 2 else charge
