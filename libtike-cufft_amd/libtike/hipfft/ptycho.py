"""Ptychography operators and CG solver on MI355X (HIP), keeping the Python
operator API of ``libtike.cufft`` (``/root/reference/src/libtike/cufft/ptycho.py``).

Device arrays are ``torch`` tensors on the current ROCm device (the reference
uses CuPy arrays); torch is used for allocation, elementwise glue and
``torch.distributed`` only -- the operators themselves are the HIP kernels behind
``libptychohip.so`` (C ABI in ``include/ptycho_hip.h``).  There is no CPU path:
importing this module without the shared library raises.

Solvers are context managers::

    with CGPtychoSolver(nscan, nprb, ndet, ptheta, nz, n) as slv:
        result = slv.run_batch(data, psi, scan, probe, piter=50)
"""
from .cg import CGPtychoSolver
from .modes import orthogonalize_modes
from .operators import PtychoCuFFT, PtychoHIP, TorchArrayModule, _ptr, _stream  # noqa: F401
from .registration import (_finish_registration, _upsampled_dft_batch, _zoom_real_factors,  # noqa: F401
                           _zoom_shifts_native, register_translation_batch)

__all__ = ["PtychoHIP", "PtychoCuFFT", "CGPtychoSolver", "register_translation_batch", "orthogonalize_modes", "TorchArrayModule"]
