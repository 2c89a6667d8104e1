"""Position registration (ptycho.py:163-248): zoom factorisations, torch GEMM fallback and the fused zoom kernel's glue."""
import numpy as np
import torch

from . import _native as nat
from .operators import PtychoHIP, _ptr, _stream

_ZOOM_CACHE = {}


def _zoom_factors(npts, ups, upsample_factor, sgn, device):
    """Rank-revealing factorisation ``A = L @ R`` of the zoomed-DFT matrix
    ``A[j, k] = exp(sgn 2 pi i j f_k)``, ``j < ups``, ``f = fftfreq(npts, upsample_factor)``.

    The phase ``2 pi j f_k`` spans only a few radians over the whole matrix (the window is
    1.5 detector pixels wide), so ``A`` is numerically low rank: for 150 x 256 at
    ``upsample_factor = 100`` the singular values fall below 1e-15 of the largest after 16
    terms.  Keeping every term above 1e-16 (plus two) reproduces ``A`` to float64 rounding --
    the same error level as the summation order of a float64 GEMM -- with ~10x fewer
    multiply-adds in the two contractions."""
    key = (npts, ups, upsample_factor, sgn, str(device))
    hit = _ZOOM_CACHE.get(key)
    if hit is None:
        freq = np.fft.fftfreq(npts, upsample_factor)
        A = np.exp(sgn * 2j * np.pi * np.arange(ups)[:, None] * freq[None, :])
        u, sv, vh = np.linalg.svd(A, full_matrices=False)
        rank = min(int((sv > 1e-16 * sv[0]).sum()) + 2, len(sv))
        if rank * 2 > len(sv):                       # not low rank (tiny detectors): keep A itself
            L, R = np.eye(ups, dtype=np.complex128), A
        else:
            L, R = u[:, :rank] * sv[:rank], vh[:rank]
        hit = (torch.as_tensor(np.ascontiguousarray(L), device=device), torch.as_tensor(np.ascontiguousarray(R), device=device))
        _ZOOM_CACHE[key] = hit
    return hit


def _zoom_real_factors(npts, ups, upsample_factor, device, rk=16):
    """Real low-rank factors of the centred window kernel for the fused zoom kernel
    (C ABI ``ptycho_cg_zoom``): with ``th = 2 pi fftfreq(npts, upsample_factor)`` and
    ``jc = j - (ups-1)/2``, ``cos(jc th) = Lc Vc`` and ``sin(jc th) = Ls Vs``.  Returns
    ``(vt [npts, rk], lz [ups, rk], nc)`` with the cos terms in columns ``< nc``, or ``None``
    when more than ``rk`` terms are above 1e-15 of the largest singular value (the float64
    noise floor of the kernel values themselves is ~1e-14: the phase argument reaches
    hundreds of radians)."""
    key = ("real", npts, ups, upsample_factor, rk, str(device))
    if key in _ZOOM_CACHE:
        return _ZOOM_CACHE[key]
    th = 2.0 * np.pi * np.fft.fftfreq(npts, upsample_factor)
    jc = np.arange(ups) - (ups - 1) / 2.0
    arg = jc[:, None] * th[None, :]
    uc, sc, vc = np.linalg.svd(np.cos(arg), full_matrices=False)
    us, ss, vs = np.linalg.svd(np.sin(arg), full_matrices=False)
    s0 = max(sc[0], ss[0] if len(ss) else 0.0)
    ns = int((ss > 1e-15 * s0).sum())
    ncos = int((sc > 1e-15 * s0).sum())
    hit = None
    if ncos + ns <= rk and rk - ns <= len(sc):
        nc = rk - ns                                   # spare terms go to the cos part
        lz = np.concatenate([uc[:, :nc] * sc[:nc], us[:, :ns] * ss[:ns]], axis=1)
        vt = np.concatenate([vc[:nc], vs[:ns]], axis=0).T
        hit = (torch.as_tensor(np.ascontiguousarray(vt), device=device), torch.as_tensor(np.ascontiguousarray(lz), device=device), nc)
    _ZOOM_CACHE[key] = hit
    return hit


def _upsampled_dft_batch(data, ups, upsample_factor, axis_offsets, conj=False):
    """Two matrix-multiply DFTs on an ``ups x ups`` window (``ptycho.py:163-188``).

    The reference builds a ``[nscan, ups, ndet]`` complex128 kernel per axis,
    ``exp(-2 pi i (j - off_i) f_k)``, and contracts it with ``einsum('ijk,ipk->ijp')``.
    The kernel factors as ``A[j,k] * B[i,k]`` with ``A = exp(-2 pi i j f_k)`` shared by all
    patterns and ``B = exp(+2 pi i off_i f_k)`` a per-pattern phase, and ``A`` itself is
    numerically low rank (``_zoom_factors``: ``A = L R``).  Each contraction is therefore an
    elementwise phase multiply and a dense GEMM with the thin factor ``R``; the ``ups x ups``
    window is expanded from the small core at the end.  Same float64 math, no 2.5 GB kernel
    tensors, ~10x fewer flops.  The contractions stay torch linear algebra (SURVEY.md
    section 2, C7).

    ``conj=True`` returns ``conj(_upsampled_dft_batch(conj(data), ...))`` -- what the caller
    at ``ptycho.py:225-228`` actually needs -- by conjugating the (small) phase factors
    instead of the farplane-sized operand and result."""
    nb, nrow, ncol = data.shape
    dev = data.device
    sgn = 1.0 if conj else -1.0
    Lc, Rc = _zoom_factors(ncol, ups, upsample_factor, sgn, dev)     # columns (k)
    Lr, Rr = _zoom_factors(nrow, ups, upsample_factor, sgn, dev)     # rows (p)

    def phase(off, npts):                                            # [nb, npts]
        freq = torch.fft.fftfreq(npts, upsample_factor, dtype=torch.float64, device=dev)
        return torch.exp(-sgn * 2j * np.pi * (off[:, None] * freq[None, :]).to(torch.complex128))

    # first axis (columns, k): tmp[i, p, r] = sum_k R[r, k] B1[i, k] data[i, p, k]
    # (complex64 x complex128 promotes inside the multiply: one pass, no separate cast)
    x = torch.mul(data, phase(axis_offsets[:, 1], ncol)[:, None, :])                 # [nb, p, k] c128
    tmp = torch.matmul(x, Rc.T)                                                      # [nb, p, r]
    del x
    # second axis (rows, p): core[i, r2, r] = sum_p R[r2, p] B0[i, p] tmp[i, p, r]
    tmp.mul_(phase(axis_offsets[:, 0], nrow)[:, :, None])
    core = torch.matmul(Rr, tmp)                                                     # [nb, r2, r]
    # rec[i, j2, j] = sum L[j2, r2] core[i, r2, r] L[j, r]
    return torch.matmul(torch.matmul(Lr, core), Lc.T)                                # [nb, j2, j]


def _argmax2d(a):
    flat = a.reshape(a.shape[0], -1).argmax(1)
    w = a.shape[2]
    return torch.stack((flat // w, flat % w), dim=1)


def _zoom_kernel_factors(ndet, upsample_factor, device, widest=None):
    """What the fused zoom kernel (C ABI ``ptycho_cg_zoom``) needs at this detector size: ``_zoom_real_factors``' ``(vt, lz,
    nc)`` and the width ``region`` of the zoomed window (ptycho.py:219), or ``None`` where the kernel does not apply
    (``ndet`` no multiple of 16 or above 1024, a window wider than ``widest``, or one that is not low rank)."""
    region = int(np.ceil(upsample_factor * 1.5))
    covered = not (ndet % 16 or ndet > 1024 or (widest is not None and region > widest))
    fac = _zoom_real_factors(ndet, region, upsample_factor, device) if covered else None
    return None if fac is None else fac + (region,)


def _zoom_shifts_native(op, image_product, best, upsample_factor):
    """Sub-pixel stage of the registration through the fused HIP kernels
    (``ptycho_cg_zoom``): ``best`` holds the whole-pixel peaks in ``ptycho_cg_argmax``'s packed
    form (int64, low word ``0xffffffff - flat index``); returns the float64 ``[nb, 2]`` shifts
    of ``ptycho.py:209-235``, or ``None`` if the kernels do not cover this case."""
    given = image_product is not None  # else the product lives in work slot 2 of the handle (ptycho_cg_cross with NULL)
    if given:
        nb, nrow, ncol = image_product.shape
        if (op is None or getattr(op, "_h", None) is None or not image_product.is_cuda
                or nrow != ncol or nrow != op.ndet or nb != op.ptheta * op.nscan or upsample_factor < 1
                or image_product.dtype != torch.complex64 or not image_product.is_contiguous()):
            return None
    fac = (_zoom_kernel_factors(nrow, upsample_factor, image_product.device, widest=max(256, nrow)) if given
           else _zoom_kernel_factors(op.ndet, upsample_factor, best.device))
    if fac is None:
        return None
    vt, lz, nc, region = fac
    shifts = torch.empty((best.shape[0], 2), dtype=torch.float64, device=best.device)
    nat.check(nat.cg_zoom(op._h, _ptr(image_product) if given else None, _ptr(best), _ptr(vt), _ptr(lz), nc, region,
                          float(upsample_factor), _ptr(shifts), _stream()))
    return shifts


def _finish_registration(image_product, maxima, upsample_factor, op=None):
    """Second half of ``register_translation_batch`` (``ptycho.py:209-248``): wrap the
    whole-pixel maxima, then the zoomed matrix DFT around them (fused HIP kernels when ``op``
    is given and covers the case, torch GEMMs otherwise)."""
    shape = image_product.shape
    if upsample_factor > 1 and op is not None:
        packed = 0xffffffff - (maxima[:, 0].to(torch.int64) * shape[2] + maxima[:, 1].to(torch.int64))
        shifts = _zoom_shifts_native(op, image_product, packed.contiguous(), upsample_factor)
        if shifts is not None:
            return shifts
    mid = [float(np.fix(s / 2)) for s in shape[1:]]
    shifts = maxima.to(torch.float64)
    shifts[:, 0] = torch.where(shifts[:, 0] > mid[0], shifts[:, 0] - shape[1], shifts[:, 0])
    shifts[:, 1] = torch.where(shifts[:, 1] > mid[1], shifts[:, 1] - shape[2], shifts[:, 1])
    if upsample_factor > 1:
        shifts = torch.round(shifts * upsample_factor) / upsample_factor
        region = int(np.ceil(upsample_factor * 1.5))
        dftshift = float(np.fix(region / 2.0))
        offset = dftshift - shifts * upsample_factor
        # = conj(upsampled_dft(conj(image_product))) / normalization of ptycho.py:225-229; the
        # positive normalisation does not move the arg-max and is skipped
        cross = _upsampled_dft_batch(image_product, region, upsample_factor, offset, conj=True)
        maxima = _argmax2d(torch.abs(cross)).to(torch.float64) - dftshift
        shifts = shifts + maxima / upsample_factor
    for dim in range(image_product.ndim):          # reference quirk, ptycho.py:243-245
        if shape[dim] == 1:
            shifts[dim] = 0
    return shifts


def register_translation_batch(src_image, target_image, upsample_factor=1, space="real", op=None):
    """Batched sub-pixel registration by phase cross-correlation (``ptycho.py:190-248``, same
    positional signature).  ``op``: an operator whose ``fft2`` (own HIP FFT) and fused zoom kernel
    are used; without one a temporary handle for the image size is made."""
    if op is None:
        nb, ny, nx = src_image.shape
        assert ny == nx, "square images only (the detector is square, ptychofft.cuh:31)"
        with PtychoHIP(nb, nx, nx, 1, nx + 2, nx + 2) as tmp:
            return register_translation_batch(src_image, target_image, upsample_factor, space, op=tmp)
    if space.lower() == "fourier":
        src_freq, target_freq = src_image, target_image
    elif space.lower() == "real":
        src_freq = op.fft2(src_image.to(torch.complex64))
        target_freq = op.fft2(target_image.to(torch.complex64))
    shape = src_freq.shape
    image_product = src_freq * target_freq.conj()
    cross = op.fft2(image_product, inverse=True) / float(shape[1] * shape[2])
    maxima = _argmax2d(torch.abs(cross))
    return _finish_registration(image_product, maxima, upsample_factor, op=op)
