"""NumPy float64 reference of ``libtike.hipfft.orthogonalize_modes`` / ``ptycho_orthogonalize_modes``.

Per angle t, with ``P`` the ``[nprb^2, M]`` matrix of the M modes: ``G = P^H P`` in float64, ``G = V diag(lam) V^H``
(``numpy.linalg.eigh``), ``lam`` descending and stable by index on exact ties, every column of ``V`` scaled so that its
component of largest magnitude (the lowest index on exact ties) is real and positive; the new modes are ``P V``.  The
result is unique wherever the eigenvalues are distinct.
"""
import numpy as np

__all__ = ["gram", "mixed_probe", "mode_eig", "mode_stack", "orthogonalize", "rotate"]


def gram(probe):
    """``[ptheta, M, M]`` complex128 Gram matrices ``P^H P`` of a ``[ptheta, M, nprb, nprb]`` probe."""
    p = np.asarray(probe).astype(np.complex128).reshape(probe.shape[0], probe.shape[1], -1)
    return np.einsum("tjx,tkx->tjk", p.conj(), p)


def mode_eig(g):
    """Eigenvalues (descending) and eigenvectors (columns, phase convention above) of one Hermitian matrix."""
    lam, v = np.linalg.eigh(g)
    order = sorted(range(len(lam)), key=lambda j: (-lam[j], j))
    lam, v = lam[order], v[:, order].copy()
    for j in range(v.shape[1]):
        a2 = np.abs(v[:, j]) ** 2
        k = int(np.flatnonzero(a2 == a2.max())[0])
        v[:, j] *= np.conj(v[k, j]) / np.abs(v[k, j])
        v[k, j] = v[k, j].real
    return lam, v


def rotate(x, v):
    """``y_j = sum_k V_kj x_k`` per angle, in float64: ``x`` ``[ptheta, M, nprb, nprb]``, ``v`` ``[ptheta, M, M]``."""
    x = np.asarray(x).astype(np.complex128)
    return np.einsum("tkyx,tkj->tjyx", x, v)


def orthogonalize(probe, *companions):
    """Returns ``(new_probe, new_companions, powers [ptheta, M], V [ptheta, M, M])``, all in float64 / complex128."""
    g = gram(probe)
    lams, vs = zip(*(mode_eig(gt) for gt in g))
    v = np.stack(vs)
    return rotate(probe, v), [rotate(c, v) for c in companions], np.stack(lams), v


def mixed_probe(nmodes, nprb=16, ptheta=2, seed=0):
    """Test input: random complex modes with powers 4^-k, mixed by a random unitary (not orthogonal, distinct powers)."""
    rng = np.random.default_rng(seed)
    base = rng.standard_normal((ptheta, nmodes, nprb * nprb)) + 1j * rng.standard_normal((ptheta, nmodes, nprb * nprb))
    q, _ = np.linalg.qr(base.transpose(0, 2, 1))                 # orthonormal columns
    p = q * 2.0 ** -np.arange(nmodes)
    u, _ = np.linalg.qr(rng.standard_normal((ptheta, nmodes, nmodes)) + 1j * rng.standard_normal((ptheta, nmodes, nmodes)))
    p = p @ u
    return p.transpose(0, 2, 1).reshape(ptheta, nmodes, nprb, nprb).astype(np.complex64)


def mode_stack(nprb, nmodes, seed=0):
    """Test input for the CG loop: ``[1, nmodes, nprb, nprb]`` smooth probe modes (Gaussian x Hermite orders up to 3,
    amplitudes 0.8^k), mixed by a random unitary so that they start non-orthogonal."""
    orders = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (0, 2), (2, 1), (1, 2), (3, 0), (0, 3), (3, 1), (1, 3)]
    assert nmodes <= len(orders)
    r = (np.arange(nprb) - (nprb - 1) / 2.0) / (nprb / 6.0)
    y, x = np.meshgrid(r, r, indexing="ij")
    herm = lambda n, t: [np.ones_like(t), 2 * t, 4 * t * t - 2, 8 * t ** 3 - 12 * t][n]  # noqa: E731
    env = np.exp(-(x * x + y * y) / 2)
    modes = np.stack([0.8 ** k * env * herm(ox, x) * herm(oy, y) for k, (ox, oy) in enumerate(orders[:nmodes])])
    modes /= np.abs(modes[0]).max()
    rng = np.random.default_rng(seed)
    u, _ = np.linalg.qr(rng.standard_normal((nmodes, nmodes)) + 1j * rng.standard_normal((nmodes, nmodes)))
    mixed = np.einsum("kyx,kj->jyx", modes.astype(np.complex128), u)
    return mixed[None].astype(np.complex64)
