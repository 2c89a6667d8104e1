"""NumPy restatement of the weighted least-squares phase unwrapper (include/ptycho_hip.h).

``unwrap(phase, weight, ...)`` states setup, PCG, finish and residues in float64; with ``dtype=np.float32`` the arrays
(phi, x, r, p, q, 1 / D, b) and ``W`` are float32 as on the device, while the dot products, alpha, beta and the stopping
tests stay float64: the float32 restatement that the GPU tests take their tolerances from.  One angle per call.
"""
import numpy as np

TWO_PI = 2.0 * np.pi


def make_truth(nz, n, amp):
    """A smooth bump on a ramp: ``amp exp(-((y - 0.45 nz)^2 + (x - 0.55 n)^2) / (2 (0.18 min(nz, n))^2)) + 0.21 x - 0.13 y``."""
    y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    s = 0.18 * min(nz, n)
    return amp * np.exp(-((y - 0.45 * nz) ** 2 + (x - 0.55 * n) ** 2) / (2.0 * s * s)) + 0.21 * x - 0.13 * y


def wrap(a, dtype=np.float64):
    """``W(a) = a - 2 pi rint(a / 2 pi)`` with every operation rounded to ``dtype``."""
    a = np.asarray(a, dtype)
    two_pi = dtype(TWO_PI)
    with np.errstate(invalid="ignore"):
        return (a - two_pi * np.rint(a / two_pi)).astype(dtype)


def effective_weight(weight, shape, dtype=np.float64):
    """``w' = w where w > 0 and finite, else 0`` (a select); all ones without a weight."""
    if weight is None:
        return np.ones(shape, dtype)
    w = np.asarray(weight, dtype)
    with np.errstate(invalid="ignore"):
        return np.where((w > 0) & np.isfinite(w), w, dtype(0)).astype(dtype)


def edges(phase, weight=None, dtype=np.float64):
    """``(wx, dx, wy, dy)``: weights and wrapped differences of the x-edges ``[nz, n-1]`` and the y-edges ``[nz-1, n]``;
    an edge of weight 0 has difference 0 whatever the phase holds."""
    f = np.asarray(phase, dtype)
    w = effective_weight(weight, f.shape, dtype)
    wx, wy = np.minimum(w[:, :-1], w[:, 1:]), np.minimum(w[:-1], w[1:])
    with np.errstate(invalid="ignore"):
        dx = np.where(wx > 0, wrap(f[:, 1:] - f[:, :-1], dtype), dtype(0)).astype(dtype)
        dy = np.where(wy > 0, wrap(f[1:] - f[:-1], dtype), dtype(0)).astype(dtype)
    return wx, dx, wy, dy


def _gather(wx, ex, wy, ey, sign):
    """Per pixel ``left + sign right + up + sign down`` of the edge values ``w e``, added in that order."""
    out = np.zeros((wy.shape[0] + 1, wx.shape[1] + 1), wx.dtype)
    tx, ty = wx * ex, wy * ey
    out[:, 1:] += tx                        # the edge to the left
    out[:, :-1] += tx if sign > 0 else -tx  # the edge to the right
    out[1:] += ty                           # the edge above
    out[:-1] += ty if sign > 0 else -ty     # the edge below
    return out


def rhs(wx, dx, wy, dy):
    """``b_p = sum_{e into p} w_e d_e - sum_{e out of p} w_e d_e``."""
    return _gather(wx, dx, wy, dy, -1)


def diagonal(wx, wy):
    return _gather(wx, np.ones_like(wx), wy, np.ones_like(wy), +1)


def apply_L(p, wx, wy):
    """``(L p)_p = sum_{e at p} w_e (p_p - p_other)``, edges in the order left, right, up, down."""
    ex, ey = p[:, 1:] - p[:, :-1], p[1:] - p[:-1]          # value at the far end minus the near end
    return _gather(wx, ex, wy, ey, -1)


def _dot(a, b):
    return float(np.sum(a.astype(np.float64) * b.astype(np.float64)))


def pcg(wx, wy, b, tol=1e-4, maxiter=None, dtype=np.float64):
    """Jacobi-preconditioned CG from ``x = 0``; returns ``(x, info)`` with iterations, status, relres, D."""
    D = diagonal(wx, wy)
    with np.errstate(divide="ignore"):
        minv = np.where(D > 0, dtype(1) / D, dtype(0)).astype(dtype)
    if maxiter is None:
        maxiter = 8 * max(b.shape)
    x = np.zeros_like(b)
    r = b.copy()
    z = (minv * r).astype(dtype)
    p = z.copy()
    rz0 = rz = _dot(r, z)
    it, status = 0, 0
    tol2 = tol * tol
    if rz0 == 0.0:
        status = 1
    elif not np.isfinite(rz0):
        status = 2
    while status == 0:
        if rz <= tol2 * rz0:
            status = 1
            break
        if it >= maxiter:
            status = 3
            break
        q = apply_L(p, wx, wy).astype(dtype)
        pq = _dot(p, q)
        if not (pq > 0.0) or not np.isfinite(pq):
            status = 2
            break
        alpha = rz / pq
        x = (x + dtype(alpha) * p).astype(dtype)
        r = (r - dtype(alpha) * q).astype(dtype)
        z = (minv * r).astype(dtype)
        rz_new = _dot(r, z)
        beta = rz_new / rz
        rz = rz_new
        it += 1
        p = (z + dtype(beta) * p).astype(dtype)
    relres = float(np.sqrt(rz / rz0)) if rz0 > 0 else 0.0
    return x, {"iterations": it, "status": status, "converged": status == 1, "residual": relres, "D": D, "rz0": rz0}


def residues(phase, weight=None, dtype=np.float64):
    """``(charge map int8 [nz-1, n-1], count)``; a loop counts only if its four pixels have ``w' > 0``."""
    f = np.asarray(phase, dtype)
    w = effective_weight(weight, f.shape, dtype)
    with np.errstate(invalid="ignore"):
        s = (((wrap(f[:-1, 1:] - f[:-1, :-1], dtype) + wrap(f[1:, 1:] - f[:-1, 1:], dtype))
              + wrap(f[1:, :-1] - f[1:, 1:], dtype)) + wrap(f[:-1, :-1] - f[1:, :-1], dtype))
        k = np.rint(s / dtype(TWO_PI))
    lit = (w[:-1, :-1] > 0) & (w[:-1, 1:] > 0) & (w[1:, :-1] > 0) & (w[1:, 1:] > 0)
    charge = np.where(lit & np.isfinite(k), k, 0).astype(np.int8)
    return charge, int(np.abs(charge.astype(np.int64)).sum())


def unwrap(phase, weight=None, congruent=True, tol=1e-4, maxiter=None, dtype=np.float64):
    """The whole definition for one angle.  Returns a dict: ``phase`` (float32), ``x``, ``k`` (``(x + c - phi) / 2 pi``
    before the rounding, NaN where ``D = 0``), ``offset``, ``iterations``, ``status``, ``converged``, ``residual``,
    ``residues``, ``D``."""
    f32 = np.asarray(phase, np.float32)
    f = f32.astype(dtype)
    w = effective_weight(weight, f.shape, dtype)
    wx, dx, wy, dy = edges(f, weight, dtype)
    b = rhs(wx, dx, wy, dy).astype(dtype)
    x, info = pcg(wx, wy, b, tol, maxiter, dtype)
    D = info["D"]
    on = D > 0
    f64, x64 = f32.astype(np.float64), x.astype(np.float64)
    z = np.sum(np.where(on & (w > 0), w.astype(np.float64), 0.0)[on] * np.exp(1j * (f64[on] - x64[on])))
    c = 0.0 if z == 0 else float(np.angle(z))
    with np.errstate(invalid="ignore"):
        kf = np.where(on, (x64 + c - f64) / TWO_PI, np.nan)
        full = f64 + TWO_PI * np.rint(kf) if congruent else x64 + c
    out = np.where(on, full.astype(np.float32), f32)
    return {"phase": out, "x": x, "k": kf, "offset": c, "iterations": info["iterations"], "status": info["status"],
            "converged": info["converged"], "residual": info["residual"], "residues": residues(f32, weight, dtype)[1],
            "D": D}


def system(wx, wy):
    """The sparse ``L`` of the edge weights (scipy CSR), pixels in row-major order."""
    import scipy.sparse as sp
    nz, n = wy.shape[0] + 1, wx.shape[1] + 1
    idx = np.arange(nz * n).reshape(nz, n)
    rows, cols, vals = [], [], []
    for a, b_, w in ((idx[:, :-1], idx[:, 1:], wx), (idx[:-1], idx[1:], wy)):
        a, b_, w = a.ravel(), b_.ravel(), w.ravel().astype(np.float64)
        rows += [a, b_, a, b_]
        cols += [a, b_, b_, a]
        vals += [w, w, -w, -w]
    return sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nz * n, nz * n))
