"""NumPy restatement of ``libtike.hipfft.resample`` (csrc/k_resample.hpp): B-spline prefilter with mirror extension, affine
warp in the geometry of ``scipy.ndimage.affine_transform``, moments.  ``dtype=np.float64`` is the reference;
``dtype=np.float32`` runs the same recursion and taps in the device's precision (coordinates stay float64 in both), which
gives the yardstick ``e32`` of tests/test_hip_resample.py.  The whole line is filtered exactly here; the device cuts lines
into segments with warm-ups (csrc/host_resample.cpp checks that plan against this filter to 1e-8).
"""
import numpy as np

CLAMP = 2.0 ** -20
FAR = 2.0 ** 30


def poles(order):
    """The poles of the B-spline prefilter, closed forms in float64."""
    return {0: [], 1: [], 2: [np.sqrt(8.0) - 3.0], 3: [np.sqrt(3.0) - 2.0],
            4: [np.sqrt(664.0 - np.sqrt(438976.0)) + np.sqrt(304.0) - 19.0,
                np.sqrt(664.0 + np.sqrt(438976.0)) - np.sqrt(304.0) - 19.0],
            5: [np.sqrt(67.5 - np.sqrt(4436.25)) + np.sqrt(26.25) - 6.5,
                np.sqrt(67.5 + np.sqrt(4436.25)) - np.sqrt(26.25) - 6.5]}[order]


def gain(order):
    g = 1.0
    for z in poles(order):
        g *= (1.0 - z) * (1.0 - 1.0 / z)
    return g


def _types(x, dtype):
    real = np.dtype(dtype)
    return real, (np.result_type(real, np.complex64) if np.iscomplexobj(x) else real)


def filter_axis(x, order, axis, dtype=np.float64):
    """Coefficients along one axis: gain, then per pole the causal and the anticausal recursion, both started exactly."""
    real, full = _types(x, dtype)
    v = np.moveaxis(np.asarray(x), axis, 0).astype(full) * real.type(gain(order))
    n = v.shape[0]
    for z64 in poles(order):
        z = real.type(z64)
        zn1 = z ** (n - 1)
        c0 = v[0] + zn1 * v[n - 1]
        zi, z2 = z, zn1 * zn1 / z
        for i in range(1, n - 1):
            c0 = c0 + (zi + z2) * v[i]
            zi, z2 = zi * z, z2 / z
        v[0] = c0 / (real.type(1) - zn1 * zn1)
        for i in range(1, n):
            v[i] = v[i] + z * v[i - 1]
        v[n - 1] = (z * v[n - 2] + v[n - 1]) * (z / (z * z - real.type(1)))
        for i in range(n - 2, -1, -1):
            v[i] = z * (v[i + 1] - v[i])
    return np.moveaxis(v, 0, axis)


def prefilter(x, order, dtype=np.float64):
    """``scipy.ndimage.spline_filter(mode="mirror")`` over the last two axes: columns, then rows."""
    real, full = _types(x, dtype)
    if order < 2:
        return np.asarray(x).astype(full)
    with np.errstate(under="ignore"):
        return filter_axis(filter_axis(x, order, -2, dtype), order, -1, dtype)


def weights(t, order, dtype=np.float64):
    """``[order + 1, ...]``: the centred cardinal B-spline at ``t + order // 2 - a``, by the recursion over the degree."""
    real = np.dtype(dtype).type
    t = np.asarray(t, dtype=dtype)
    w = [np.ones_like(t)] + [np.zeros_like(t) for _ in range(order)]
    dn = t + real(order // 2)
    for k in range(1, order + 1):
        dk, half, inv = dn - real(0.5) * real(order - k), real(0.5) * real(k + 1), real(1) / real(k)
        for a in range(k, -1, -1):
            left = w[a - 1] if a >= 1 else real(0)
            right = w[a] if a <= k - 1 else real(0)
            w[a] = ((half + dk - real(a)) * left + (half - dk + real(a)) * right) * inv
    return np.stack(w)


def reflect(i, n):
    """Mirror reflection of integer indices into ``[0, n)``, period ``2 n - 2``."""
    p = 2 * n - 2
    i = np.mod(i, p)
    return np.where(i < n, i, p - i)


def coordinates(matrix, offset, shape):
    """Source coordinates ``(sy, sx)`` of every output pixel: ``(m0 oy + m1 ox) + off`` in float64."""
    m, off = np.asarray(matrix, np.float64), np.asarray(offset, np.float64)
    oy, ox = np.meshgrid(np.arange(shape[0], dtype=np.float64), np.arange(shape[1], dtype=np.float64), indexing="ij")
    return (m[0, 0] * oy + m[0, 1] * ox) + off[0], (m[1, 0] * oy + m[1, 1] * ox) + off[1]


def inside(sy, sx, ny, nx, mode):
    """The coordinates after constant mode's clamp, and which of them are evaluated."""
    if mode == "mirror":
        return sy, sx, (np.abs(sy) < FAR) & (np.abs(sx) < FAR)
    sy = np.where((sy < 0) & (sy >= -CLAMP), 0.0, sy)
    sx = np.where((sx < 0) & (sx >= -CLAMP), 0.0, sx)
    sy = np.where((sy > ny - 1) & (sy <= ny - 1 + CLAMP), ny - 1.0, sy)
    sx = np.where((sx > nx - 1) & (sx <= nx - 1 + CLAMP), nx - 1.0, sx)
    return sy, sx, (sy >= 0) & (sy <= ny - 1) & (sx >= 0) & (sx <= nx - 1)


def sample(coef, sy, sx, order, mode="constant", cval=0.0, dtype=np.float64):
    """The spline with coefficients ``coef`` (``[ny, nx]``) at ``(sy, sx)``: rows first, taps in index order."""
    real, full = _types(coef, dtype)
    coef = np.asarray(coef).astype(full)
    ny, nx = coef.shape
    sy, sx, ok = inside(sy, sx, ny, nx, mode)
    sy, sx = np.where(ok, sy, 0.0), np.where(ok, sx, 0.0)
    fy = np.floor(sy if order & 1 else sy + 0.5)
    fx = np.floor(sx if order & 1 else sx + 0.5)
    wy, wx = weights((sy - fy).astype(real), order, real), weights((sx - fx).astype(real), order, real)
    by, bx = fy.astype(np.int64) - order // 2, fx.astype(np.int64) - order // 2
    acc = np.zeros(sy.shape, full)
    for a in range(order + 1):
        iy = reflect(by + a, ny)
        row = np.zeros(sy.shape, full)
        for b in range(order + 1):
            row = wx[b] * coef[iy, reflect(bx + b, nx)] + row
        acc = wy[a] * row + acc
    return np.where(ok, acc, full.type(cval))


def warp(x, matrix=None, offset=None, shape=None, order=3, mode="constant", cval=0.0, prefilter_=True, dtype=np.float64):
    """``libtike.hipfft.resample.warp`` for ``x`` ``[..., ny, nx]``; ``matrix`` / ``offset`` one for all or one per image."""
    x = np.asarray(x)
    lead, (ny, nx) = x.shape[:-2], x.shape[-2:]
    shape = (ny, nx) if shape is None else tuple(shape)
    m = np.broadcast_to(np.eye(2) if matrix is None else np.asarray(matrix, np.float64), lead + (2, 2)).reshape(-1, 2, 2)
    o = np.broadcast_to(np.zeros(2) if offset is None else np.asarray(offset, np.float64), lead + (2,)).reshape(-1, 2)
    imgs = x.reshape((-1, ny, nx))
    out = []
    for i in range(imgs.shape[0]):
        coef = prefilter(imgs[i], order, dtype) if prefilter_ else imgs[i]
        sy, sx = coordinates(m[i], o[i], shape)
        out.append(sample(coef, sy, sx, order, mode, cval, dtype))
    return np.stack(out).reshape(lead + shape)


def rotate_map(angle, in_shape, out_shape=None, center=None):
    """``(matrix, offset)`` of ``scipy.ndimage.rotate(reshape=False)``: ``center`` of the input lands on the output's centre."""
    out_shape = in_shape if out_shape is None else out_shape
    a = np.deg2rad(angle)
    m = np.array([[np.cos(a), np.sin(a)], [-np.sin(a), np.cos(a)]])
    centre = (np.asarray(in_shape, np.float64) - 1) / 2 if center is None else np.asarray(center, np.float64)
    return m, centre - m @ ((np.asarray(out_shape, np.float64) - 1) / 2)


def zoom_map(in_shape, factor):
    """``(matrix, offset, out_shape)`` of ``scipy.ndimage.zoom``: corner-aligned."""
    f = np.broadcast_to(np.asarray(factor, np.float64), (2,))
    out = tuple(int(round(n * v)) for n, v in zip(in_shape, f))
    z = [(n - 1) / (k - 1) if k > 1 else 1.0 for n, k in zip(in_shape, out)]
    return np.diag(z), np.zeros(2), out


def moments(x, weight=None, which="value"):
    """``sum w, sum w y, sum w x, sum w y^2, sum w x^2`` per image in float64 of the float32 masses ``w``."""
    x = np.asarray(x)
    if np.iscomplexobj(x):
        re, im = x.real.astype(np.float32), x.imag.astype(np.float32)
        w = re * re + im * im
    else:
        w = x.astype(np.float32)
        w = {"value": w, "positive": np.where(w > 0, w, np.float32(0)), "power": w * w}[which]
    if weight is not None:
        w = w * np.asarray(weight, np.float32)
    w = w.astype(np.float64)
    y, xx = np.meshgrid(np.arange(x.shape[-2], dtype=np.float64), np.arange(x.shape[-1], dtype=np.float64), indexing="ij")
    return np.stack([(w * k).sum((-2, -1)) for k in (np.ones_like(y), y, xx, y * y, xx * xx)], -1)
