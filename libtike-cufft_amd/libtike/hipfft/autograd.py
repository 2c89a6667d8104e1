"""``torch.autograd`` for the forward operator: ``FwdFunction`` ties ``PtychoHIP.fwd`` to its three adjoints, so that a
loss written in torch on the farplane differentiates through the HIP kernels (``PtychoHIP.fwd_autograd``)."""
import torch
from torch.autograd.function import once_differentiable


class FwdFunction(torch.autograd.Function):
    """``farplane = op.fwd(psi, scan, probe)``.  ``backward`` receives ``G = dL/dfarplane`` in torch's convention for a
    real loss (``dL/dRe + i dL/dIm``) and returns, where asked for, ``adj(G)`` for ``psi``, ``adj_probe(G)`` for ``probe``
    (``fwd`` is linear in either, so its adjoint is the gradient) and ``adj_scan(G)`` for ``scan``."""

    @staticmethod
    def forward(ctx, op, psi, scan, probe):
        ctx.op = op
        ctx.save_for_backward(psi, scan, probe)
        return op.fwd(psi, scan, probe)

    @staticmethod
    @once_differentiable
    def backward(ctx, grad):
        op = ctx.op
        psi, scan, probe = ctx.saved_tensors
        # pointers are taken below: a lazily conjugated or strided G becomes plain memory first
        grad = grad.resolve_conj().contiguous()
        need = ctx.needs_input_grad
        grad_psi = op.adj(grad, scan, probe) if need[1] else None
        grad_scan = op.adj_scan(grad, scan, psi, probe) if need[2] else None
        grad_probe = op.adj_probe(grad, scan, psi) if need[3] else None
        return None, grad_psi, grad_scan, grad_probe
