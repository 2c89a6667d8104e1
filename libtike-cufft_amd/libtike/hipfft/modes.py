"""Orthogonal probe modes (C ABI ptycho_orthogonalize_modes, csrc/k_modes.hpp)."""
import torch

from . import _native as nat
from .operators import _ptr, _stream


def orthogonalize_modes(probe, *companions):
    """Make the incoherent modes of every angle orthogonal, strongest first, in place.

    ``probe``: ``[ptheta, M, nprb, nprb]`` complex64 device tensor, 1 <= M <= 16.  Per angle, with ``P`` the
    ``[nprb^2, M]`` matrix of its modes, ``G = P^H P`` (float64) is diagonalised, ``G = V diag(lam) V^H``, with ``lam``
    descending (stable by index on exact ties) and each eigenvector scaled so that its component of largest magnitude
    (the lowest index on ties) is real and positive; the modes become ``P V``.  Afterwards ``P^H P = diag(lam)`` up to
    float32 rounding, ``sum(lam)`` equals ``sum_k |P_k|^2``, and the summed intensity ``sum_k |F(psi P_k)|^2`` of any
    object is unchanged (the mixing is unitary).  ``companions`` (at most two tensors of the probe's shape, dtype and
    device, e.g. a CG direction and a previous gradient) are rotated by the same ``V``.

    Returns the powers ``lam``: a ``[ptheta, M]`` float64 device tensor (the mode occupancy is ``lam / lam.sum(1)``).
    Two kernel launches on the current stream and no host synchronisation.
    """
    if not isinstance(probe, torch.Tensor) or probe.dtype != torch.complex64 or probe.ndim != 4 or not probe.is_cuda:
        raise TypeError("probe must be a [ptheta, M, nprb, nprb] complex64 device tensor")
    ptheta, nmodes = probe.shape[0], probe.shape[1]
    if not 1 <= nmodes <= nat.ORTHO_MAX_MODES:
        raise ValueError("orthogonalize_modes: %d modes, supported 1 .. %d" % (nmodes, nat.ORTHO_MAX_MODES))
    if len(companions) > 2:
        raise ValueError("orthogonalize_modes: at most two companions")
    for c in companions:
        if not isinstance(c, torch.Tensor) or c.shape != probe.shape or c.dtype != probe.dtype or c.device != probe.device:
            raise ValueError("orthogonalize_modes: every companion needs the probe's shape, dtype and device")
    npix = probe.shape[2] * probe.shape[3]
    if ptheta == 0 or npix == 0:
        return torch.zeros((ptheta, nmodes), dtype=torch.float64, device=probe.device)
    tensors = (probe,) + tuple(companions)
    work = [t if t.is_contiguous() else t.contiguous() for t in tensors]
    with torch.cuda.device(probe.device):
        powers = torch.empty((ptheta, nmodes), dtype=torch.float64, device=probe.device)
        v = torch.empty((ptheta, nmodes, nmodes), dtype=torch.complex128, device=probe.device)
        ptrs = [_ptr(w) for w in work] + [None] * (3 - len(work))
        nat.check(nat.orthogonalize_modes(ptrs[0], ptrs[1], ptrs[2], ptheta, nmodes, npix, _ptr(v), _ptr(powers), _stream()))
    for t, w in zip(tensors, work):
        if w is not t:
            t.copy_(w)
    return powers
