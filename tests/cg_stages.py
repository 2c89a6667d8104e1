"""Plain NumPy reference of every fused CG stage of the C ABI (``include/ptycho_hip.h``, fused- and native-stage blocks),
one function per stage, on the farplanes the stages see.

Every stage of the device reads work slots that hold column passes of ``fwd(psi, scan, probe)``; the row pass it fuses
completes the 2-D DFT, so a stage is defined on the farplane ``G = op.fwd(psi, scan, probe, ndet)``.  ``farplane`` makes
it.  The semantics restate the epilogue comments of ``k_rows_fused`` (``csrc/k_rows.hpp``):

* ``stats``: ``I = |G|^2``; ``{sum sqrt(I d), sum I}``.
* ``project``: ``s = a / b`` (1 when ``ab`` is None), ``I' = I s^2``, ``fpsi = (G s)(1 / s) = G``;
  gaussian ``r = fpsi - sqrt(d) fpsi / (sqrt(I') + 1e-32)``, cost ``sum (sqrt I' - sqrt d)^2``;
  poisson_ml ``r = fpsi - d fpsi / (I' + 1e-32)``, cost ``sum (I' - d ln(I' + 1e-32))``.
* ``linesearch``: ``t1 = s G1``, ``t2 = G2``, ``p1 = |t1|^2``, ``p2 = |t2|^2``, ``p3 = 2 Re(t1 conj t2)``; costs
  ``f(p1 + y_j^2 p2 + y_j p3)`` for ``y_j = gamma0 2^-j``, ``j < ncand``, then ``f(p1)``.  Gaussian
  ``f(x) = sum (sqrt|x| - sqrt d)^2``; poisson_ml ``f(x) = sum (|x| - d ln(|x| + 1e-32) - (d - d ln(d + 1e-32)))``:
  the pixel's constant is subtracted, as the kernel does.
* ``intensity_modes``, ``project_multi``, ``linesearch_modes``: the same over probe modes.
* ``cross``: the image product ``u1 conj(u1 + gamma d1)`` and the first maximum of ``|IDFT2(product)|`` per position.
* ``zoom``: the sub-pixel stage of the registration (``ptycho_cg_zoom``): the whole-pixel peak wrapped to
  ``[-N/2, N/2]`` (an index above ``fix(N/2)`` loses ``N``; ``N/2`` itself stays positive), the ``ups x ups`` window
  ``|conj(upsampled_dft(conj(product)))|`` around it and ``shift = peak + (argmax - fix(ups/2)) / upsample_factor``.
* ``finish``: the tail of the object step for angle 0 (``ptycho_cg_obj_finish``): the registration of
  ``fwd(psi, 1)[0]`` against ``fwd(psi, 1)[0] + gamma fwd(dpsi, 1)[0]`` and ``psi + gamma dpsi`` as float32 arithmetic.

With a mask (nonzero = measured) data, the intensity and the line-search terms are selected to 0 at unmeasured pixels
before any arithmetic (never multiplied: the data there may be NaN) and the residual is 0 there.

``precision="double"`` evaluates everything in float64.  ``precision="single"`` evaluates the same formulas elementwise in
float32 on float32 farplanes, with float64 sums: its distance from the float64 value is what a correct float32 kernel
is expected to show, and the GPU tests bound the device's error by a small multiple of it.  The step length ``gamma0``
and the scale ``a / b`` are rounded to float32 in both precisions, because the device takes them as float32: the two
precisions then define the same operation.

Every function returns sums as float64 and, where a tolerance needs it, ``scale``: the sum of the magnitudes of the
terms, the size that a float32 evaluation's error is proportional to (a cost near its minimum is much smaller).
"""
import numpy as np

from oracle import ptycho_oracle as op

__all__ = ["farplane", "stats", "project", "linesearch", "intensity_modes", "project_multi", "linesearch_modes",
           "cross", "zoom", "finish", "axpy32", "peak_product", "shifted_pair", "edge_indices", "wrap_index", "EPS"]

EPS = 1e-32   # the regulariser of the residuals, the cost's logarithm and the line-search constant


def _types(precision):
    if precision == "double":
        return np.complex128, np.float64
    if precision == "single":
        return np.complex64, np.float32
    raise ValueError(precision)


def farplane(psi, scan, prb, ndet, precision="double"):
    """``op.fwd`` in the given precision: what the row stages of a slot filled from (psi, scan, prb) transform."""
    return op.fwd(psi, scan, prb, ndet, precision)


def _keep(mask, x):
    if mask is None:
        return x
    return np.where(np.asarray(mask) != 0, x, np.zeros((), dtype=x.dtype))


def _data(d, mask, precision):
    _, ft = _types(precision)
    return _keep(mask, np.asarray(d).astype(ft))


def _scale(ab):
    """(s, 1/s) as the kernels form them: a / b and b / a of the float32 values of a, b."""
    if ab is None:
        return 1.0, 1.0
    a, b = np.float32(ab[0]), np.float32(ab[1])
    return np.float32(a / b), np.float32(b / a)


def _sum(x):
    return float(np.sum(np.asarray(x, dtype=np.float64)))


def stats(G, d, mask=None, precision="double"):
    """``ptycho_cg_stats``: ``{sum sqrt(I d), sum I}``, ``I = |G|^2`` (0 at unmeasured pixels)."""
    ct, ft = _types(precision)
    G = np.asarray(G).astype(ct)
    d = _data(d, mask, precision)
    inten = _keep(mask, (G.real * G.real + G.imag * G.imag).astype(ft))
    return np.array([_sum(np.sqrt(inten * d)), _sum(inten)])


def _project(fp, inten, d, model, precision):
    """residual, cost terms and their magnitudes of the projection with intensity ``inten`` (= I')."""
    ct, ft = _types(precision)
    eps = ft(EPS)
    if model == "gaussian":
        sd, si = np.sqrt(d), np.sqrt(inten)
        r = fp - (fp * sd) * (ft(1) / (si + eps))
        terms = (si - sd) ** 2
        mag = terms
    elif model == "poisson_ml":
        r = fp - (fp * d) * (ft(1) / (inten + eps))
        lg = d * np.log(inten + eps)
        terms = inten - lg
        mag = np.abs(inten) + np.abs(lg)
    else:
        raise ValueError(model)
    return r.astype(ct), terms, mag


def project(G, d, ab=None, model="gaussian", mask=None, precision="double"):
    """``ptycho_cg_project`` from a slot made with the probe before its rescale.  Returns ``(r, cost, scale)``: the
    projected residual farplane (``ptycho_cg_adj_cols`` turns it into the gradient), the cost and the sum of the
    magnitudes of the cost's terms."""
    ct, ft = _types(precision)
    s, sinv = _scale(ab)
    G = np.asarray(G).astype(ct)
    d = _data(d, mask, precision)
    inten = (G.real * G.real + G.imag * G.imag).astype(ft) * ft(s) * ft(s)
    inten = _keep(mask, inten)
    fp = (G * ft(s)) * ft(sinv)
    r, terms, mag = _project(fp, inten, d, model, precision)
    return _keep(mask, r), _sum(terms), _sum(mag)


def _ls_costs(p1, p2, p3, d, gamma0, ncand, model, precision):
    _, ft = _types(precision)
    eps = ft(EPS)
    g0 = np.float32(gamma0)
    if model == "gaussian":
        sd = np.sqrt(d)

        def f(x):
            t = (np.sqrt(np.abs(x)) - sd) ** 2
            return _sum(t), _sum(t)
    elif model == "poisson_ml":
        lc = d * np.log(d + eps)
        c = d - lc

        def f(x):
            ax = np.abs(x)
            lg = d * np.log(ax + eps)
            return _sum((ax - c) - lg), _sum(ax + np.abs(lg) + np.abs(d) + np.abs(lc))
    else:
        raise ValueError(model)
    costs, scale = [], []
    for j in range(ncand):
        y = ft(np.ldexp(np.float64(g0), -j))
        v, m = f(p1 + p2 * (y * y) + p3 * y)
        costs.append(v)
        scale.append(m)
    v, m = f(p1)
    costs.append(v)
    scale.append(m)
    return np.array(costs), np.array(scale)


def linesearch(G1, G2, d, ab, gamma0, ncand, model="gaussian", mask=None, precision="double"):
    """``ptycho_cg_linesearch``: ``ncand + 1`` costs and the magnitudes of their terms."""
    ct, ft = _types(precision)
    s, _ = _scale(ab)
    t1 = _keep(mask, np.asarray(G1).astype(ct) * ft(s))
    t2 = _keep(mask, np.asarray(G2).astype(ct))
    d = _data(d, mask, precision)
    p1 = (t1.real * t1.real + t1.imag * t1.imag).astype(ft)
    p2 = (t2.real * t2.real + t2.imag * t2.imag).astype(ft)
    p3 = (ft(2) * (t1.real * t2.real + t1.imag * t2.imag)).astype(ft)
    return _ls_costs(p1, p2, p3, d, gamma0, ncand, model, precision)


def intensity_modes(Gs, d=None, mask=None, precision="double"):
    """``ptycho_cg_intensity_modes``: the array ``sum_k |G_k|^2`` (written before the mask is applied) and, with ``d``,
    the sums ``{sum sqrt(inten d), sum inten}`` over measured pixels."""
    ct, ft = _types(precision)
    inten = None
    for G in Gs:
        G = np.asarray(G).astype(ct)
        i = (G.real * G.real + G.imag * G.imag).astype(ft)
        inten = i if inten is None else inten + i
    if d is None:
        return inten, None
    dd = _data(d, mask, precision)
    im = _keep(mask, inten)
    return inten, np.array([_sum(np.sqrt(im * dd)), _sum(im)])


def project_multi(G, inten, d, ab=None, slot_unscaled=1, model="gaussian", mask=None, precision="double"):
    """``ptycho_cg_project_multi``: ``I' = inten s^2``; ``fpsi = (G s)(1/s)`` for a slot made with the probe before its
    rescale (``slot_unscaled = 1``), ``G (1/s)`` for one made with the rescaled probe.  Returns ``(r, cost, scale)``."""
    ct, ft = _types(precision)
    s, sinv = _scale(ab)
    G = np.asarray(G).astype(ct)
    d = _data(d, mask, precision)
    i2 = _keep(mask, np.asarray(inten).astype(ft) * (ft(s) * ft(s)))
    fp = (G * ft(s)) * ft(sinv) if slot_unscaled else G * ft(sinv)
    r, terms, mag = _project(fp, i2, d, model, precision)
    return _keep(mask, r), _sum(terms), _sum(mag)


def linesearch_modes(G1s, G2s, d, ab, gamma0, ncand, model="gaussian", mask=None, inten=None, precision="double"):
    """``ptycho_cg_linesearch_modes`` / ``_chunk``: ``t1_k = s G1_k``, ``t2_k = G2_k``; ``p1 = inten`` if given (not
    rescaled), else ``sum_k |t1_k|^2``; ``p2 = sum_k |t2_k|^2``; ``p3 = sum_k 2 Re(t1_k conj t2_k)``."""
    ct, ft = _types(precision)
    s, _ = _scale(ab)
    p1 = p2 = p3 = None
    for G1, G2 in zip(G1s, G2s):
        t1 = np.asarray(G1).astype(ct) * ft(s)
        t2 = np.asarray(G2).astype(ct)
        q1 = (t1.real * t1.real + t1.imag * t1.imag).astype(ft)
        q2 = (t2.real * t2.real + t2.imag * t2.imag).astype(ft)
        q3 = (ft(2) * (t1.real * t2.real + t1.imag * t2.imag)).astype(ft)
        p1, p2, p3 = (q1, q2, q3) if p1 is None else (p1 + q1, p2 + q2, p3 + q3)
    if inten is not None:
        p1 = np.asarray(inten).astype(ft)
    p1, p2, p3 = (_keep(mask, p) for p in (p1, p2, p3))
    return _ls_costs(p1, p2, p3, _data(d, mask, precision), gamma0, ncand, model, precision)


def cross(U1, D1, gamma, precision="double"):
    """``ptycho_cg_cross`` + ``ptycho_cg_argmax``: the image product ``u1 conj(u1 + gamma d1)``, the flat index
    ``y ndet + x`` of the first maximum of ``|IDFT2(product)|`` (unnormalised) per position, that maximum, and the
    second largest value (the margin that makes the arg-max well defined)."""
    ct, ft = _types(precision)
    U1 = np.asarray(U1).astype(ct)
    D1 = np.asarray(D1).astype(ct)
    u2 = U1 + D1 * ft(np.float32(gamma))
    ip = (U1 * np.conj(u2)).astype(ct)
    ndet = ip.shape[-1]
    a = np.abs(op.ifft2_unnorm(ip)).reshape(-1, ndet * ndet)
    idx = np.argmax(a, axis=1)
    top = a[np.arange(a.shape[0]), idx]
    second = np.partition(a, -2, axis=1)[:, -2]
    return ip, idx, top, second


def zoom(ip, idx, upsample_factor, precision="double"):
    """``ptycho_cg_zoom`` (``ptycho.py:209-235``): ``ip`` ``[nb, N, N]`` image products, ``idx`` the flat index
    ``y N + x`` of the whole-pixel peak per position.  The product is taken in the given precision (complex64 for
    "single"); everything after it is float64, as on the device.  Returns ``(window, peak, shifts, gap)``: the
    ``[nb, ups, ups]`` magnitudes, the flat arg-max of each window (first maximum), the float64 ``[nb, 2]`` shifts and
    per position the relative gap ``(top - second) / top`` between the largest and the second-largest window value
    (``inf`` for an all-zero window, whose arg-max is index 0 by the first-maximum rule)."""
    from oracle.cg_oracle import upsampled_dft_batch
    ct, _ = _types(precision)
    ip = np.asarray(ip).astype(ct).astype(np.complex128)
    nb, nrow, ncol = ip.shape
    idx = np.asarray(idx, dtype=np.int64)
    shifts = np.stack((idx // ncol, idx % ncol), axis=1).astype(np.float64)
    mid = [np.fix(nrow / 2), np.fix(ncol / 2)]
    shifts[shifts[:, 0] > mid[0], 0] -= nrow
    shifts[shifts[:, 1] > mid[1], 1] -= ncol
    shifts = np.round(shifts * upsample_factor) / upsample_factor
    ups = int(np.ceil(upsample_factor * 1.5))
    dftshift = np.fix(ups / 2.0)
    offset = dftshift - shifts * upsample_factor
    window = np.zeros((nb, ups, ups))
    live = np.nonzero(ip.reshape(nb, -1).any(axis=1))[0]      # an all-zero product has an all-zero window: no need to sum it
    if live.size:
        window[live] = np.abs(upsampled_dft_batch(ip[live].conj(), ups, upsample_factor, offset[live]).conj())
    flat = window.reshape(nb, -1)
    peak = flat.argmax(1)
    top = flat[np.arange(nb), peak]
    second = np.partition(flat, -2, axis=1)[:, -2]
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(top > 0, (top - second) / top, np.inf)
    maxima = np.stack((peak // ups, peak % ups), axis=1).astype(np.float64) - dftshift
    return window, peak, shifts + maxima / upsample_factor, gap


def axpy32(x, d, gamma):
    """``x + float32(gamma) d`` as ``k_cg_axpy`` forms it: per real component a float32 product, rounded, then a float32
    sum, rounded -- no fused multiply-add."""
    x = np.asarray(x).astype(np.complex64)
    d = np.asarray(d).astype(np.complex64)
    g = np.float32(gamma)
    out = np.empty_like(x)
    out.real = x.real + (g * d.real).astype(np.float32)
    out.imag = x.imag + (g * d.imag).astype(np.float32)
    return out


def finish(psi, dpsi, gamma, scan, ndet, upsample_factor=100, precision="double", nprb=None):
    """``ptycho_cg_obj_finish`` for angle 0 (``ptycho.py:398-405``): ``tmp1 = fwd(psi, 1)[0]``,
    ``tmp2 = tmp1 + float32(gamma) fwd(dpsi, 1)[0]`` with the all-ones probe of ``nprb`` pixels (default ``ndet``), the
    registration of the two in Fourier space, and the object update.  Returns a dict: ``ip`` the image product
    ``[nscan, ndet, ndet]``, ``idx`` / ``top`` / ``second`` the whole-pixel stage of ``cross``, ``window`` / ``peak`` /
    ``shifts`` / ``gap`` of ``zoom`` and ``psi`` = ``axpy32(psi, dpsi, gamma)`` (all angles)."""
    psi = np.asarray(psi)
    nprb = ndet if nprb is None else nprb
    ones = np.ones((psi.shape[0], nprb, nprb), np.complex64)
    scan = np.asarray(scan)
    U = farplane(psi[:1], scan[:1], ones[:1], ndet, precision)
    D = farplane(np.asarray(dpsi)[:1], scan[:1], ones[:1], ndet, precision)
    ip, idx, top, second = cross(U, D, gamma, precision)
    window, peak, shifts, gap = zoom(ip[0], idx, upsample_factor, precision)
    return dict(ip=ip[0], idx=idx, top=top, second=second, window=window, peak=peak, shifts=shifts, gap=gap,
                psi=axpy32(psi, dpsi, gamma))


# ---- inputs of the registration tests ------------------------------------------------------------------------------------
def edge_indices(n):
    """Whole-pixel peak indices at which the wrap to ``[-n/2, n/2]`` and the fftfreq ordering can go wrong."""
    return [0, 1, n // 2 - 1, n // 2, n // 2 + 1, n - 1]


def wrap_index(i, n):
    """``ptycho.py:212-216``: an index above ``fix(n / 2)`` loses ``n``; ``n / 2`` itself stays positive."""
    i = np.asarray(i, dtype=np.int64)
    return np.where(i > n // 2, i - n, i)


def peak_product(rng, ndet, true):
    """Image products ``[nb, ndet, ndet]`` (complex64) whose correlation peaks at the shifts ``true`` ``[nb, 2]`` (pixels,
    within ``[-ndet/2, ndet/2]``): a smooth positive base times the phase ramp of the shift, plus 5 % complex noise."""
    true = np.asarray(true, dtype=np.float64)
    nb = true.shape[0]
    ky = np.fft.fftfreq(ndet)[None, :, None]
    kx = np.fft.fftfreq(ndet)[None, None, :]
    base = rng.standard_normal((nb, ndet, ndet)) ** 2 + 0.1
    ip = base * np.exp(-2j * np.pi * (ky * true[:, 0, None, None] + kx * true[:, 1, None, None]))
    return (ip + 0.05 * (rng.standard_normal(ip.shape) + 1j * rng.standard_normal(ip.shape))).astype(np.complex64)


def shifted_pair(rng, shape, shift, gamma):
    """``(psi, dpsi)``, complex64 ``shape`` = ``[ptheta, nz, n]``: ``psi`` is white (zero mean: the correlation of two
    patches peaks at the shift only), ``psi2`` is ``psi`` moved by ``shift`` pixels with a Fourier phase ramp plus 5 %
    noise, and ``dpsi = (psi2 - psi) / float32(gamma)``, so that ``psi + gamma dpsi`` is ``psi2`` up to rounding."""
    def white():
        return rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    psi = white().astype(np.complex64)
    ky = np.fft.fftfreq(shape[-2])[:, None]
    kx = np.fft.fftfreq(shape[-1])[None, :]
    psi2 = np.fft.ifft2(np.fft.fft2(psi) * np.exp(-2j * np.pi * (ky * shift[0] + kx * shift[1])))
    psi2 = (psi2 + 0.05 * white()).astype(np.complex64)
    return psi, ((psi2 - psi) / np.float32(gamma)).astype(np.complex64)
