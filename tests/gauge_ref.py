"""NumPy restatement of the illumination map and the gauge fit / apply of ``libtike.hipfft.gauge``, written from the
definitions ("Illumination and gauge"), in float64 by default.  ``dtype=np.float32`` runs the same code in
single precision: the tests size their tolerances by the distance between the two.  Not collected by pytest.

A gauge is ``(gy, gx, phi0, s, yc, xc)`` per angle.
"""
import numpy as np


def _complex(dtype):
    return np.complex128 if np.dtype(dtype) == np.float64 else np.complex64


def split(p):
    """``modff`` split of one float32 scan coordinate: ``(valid, integer part, fraction)``; the position is skipped
    for a negative integer part (``-0.0`` is not negative), a non-finite value or an integer part ``>= 1e9``."""
    f, i = np.modf(np.float32(p))
    valid = bool(not (i < 0) and i < np.float32(1.0e9) and i == i)
    return valid, int(i) if valid else 0, np.float32(f)


def amp2(probe, dtype=np.float64):
    """``A[t] = sum_m |probe[t, m]|^2`` of a ``[ptheta, M, nprb, nprb]`` or ``[ptheta, nprb, nprb]`` probe, modes in order."""
    p = np.asarray(probe)
    if p.ndim == 3:
        p = p[:, None]
    a = np.zeros((p.shape[0],) + p.shape[2:], dtype)
    for m in range(p.shape[1]):
        re, im = p[:, m].real.astype(dtype), p[:, m].imag.astype(dtype)
        a = a + (re * re + im * im)
    return a


def illumination(scan, probe, nz, n, dtype=np.float64):
    """``out[t, sy+iy+a, sx+ix+b] += w_ab A[t, iy, ix]``: loops over angles, positions and the four taps; taps outside
    the object are dropped."""
    scan = np.asarray(scan, np.float32)
    a2 = amp2(probe, dtype)
    nprb = a2.shape[-1]
    out = np.zeros((scan.shape[0], nz, n), dtype)
    one = dtype(1)
    for t in range(scan.shape[0]):
        for py, px in scan[t]:
            vy, sy, fy = split(py)
            vx, sx, fx = split(px)
            if not (vy and vx):
                continue
            wy = (one - dtype(fy), dtype(fy))
            wx = (one - dtype(fx), dtype(fx))
            for a in (0, 1):
                for b in (0, 1):
                    w = wx[b] * wy[a]
                    h, wd = min(nprb, nz - sy - a), min(nprb, n - sx - b)
                    if h <= 0 or wd <= 0:
                        continue
                    out[t, sy + a:sy + a + h, sx + b:sx + b + wd] += w * a2[t, :h, :wd]
    return out


def _arg(c):
    return 0.0 if c == 0 else float(np.angle(c))


def fit(psi, weight=None, ref=None, dtype=np.float64):
    """``[ptheta, 6]`` float64 (``[6]`` for 2-D ``psi``); every sum formed in ``dtype``."""
    cdt = _complex(dtype)
    shape = np.shape(psi)
    nz, n = shape[-2:]
    p3 = np.asarray(psi).reshape(-1, nz, n).astype(cdt)
    r3 = None if ref is None else np.asarray(ref).reshape(-1, nz, n).astype(cdt)
    w3 = np.ones(p3.shape, dtype) if weight is None else np.asarray(weight).reshape(-1, nz, n).astype(dtype)
    y = np.arange(nz, dtype=dtype)[:, None]
    x = np.arange(n, dtype=dtype)[None, :]
    out = np.zeros((p3.shape[0], 6))
    for t in range(p3.shape[0]):
        p, w = p3[t], w3[t]
        u = p if r3 is None else p * np.conj(r3[t])
        W = w.sum()
        if not W > 0:
            out[t] = (0, 0, 0, 1, 0, 0)
            continue
        gx = _arg((w[:, :-1] * w[:, 1:] * u[:, 1:] * np.conj(u[:, :-1])).sum())
        gy = _arg((w[:-1] * w[1:] * u[1:] * np.conj(u[:-1])).sum())
        yc, xc = (w * y).sum() / W, (w * x).sum() / W
        ramp = dtype(gy) * (y - yc) + dtype(gx) * (x - xc)
        phi0 = _arg((w * u * np.exp(-1j * ramp).astype(cdt)).sum())
        num = (w * np.abs(p) ** 2).sum()
        den = W if r3 is None else (w * np.abs(r3[t]) ** 2).sum()
        s = np.sqrt(num / den) if num > 0 and den > 0 else 1.0
        out[t] = (gy, gx, phi0, s, yc, xc)
    return out[0] if len(shape) == 2 else out


def apply(x, gauge, which="object", dtype=np.float64):
    """A gauge-fixed copy of ``x``: the object form for ``[ptheta, nz, n]`` / ``[nz, n]``, the probe companion for
    ``[ptheta, M, nprb, nprb]`` / ``[ptheta, nprb, nprb]``."""
    cdt = _complex(dtype)
    x = np.asarray(x)
    ny, nx = x.shape[-2:]
    g = np.asarray(gauge, np.float64).reshape(-1, 6).astype(dtype)
    lead = x.shape[:-2] if x.ndim > 2 else (1,)
    v = x.reshape((g.shape[0], -1, ny, nx)).astype(cdt)
    yy = np.arange(ny, dtype=dtype)[:, None]
    xx = np.arange(nx, dtype=dtype)[None, :]
    out = np.empty_like(v)
    for t in range(g.shape[0]):
        gy, gx, phi0, s, yc, xc = g[t]
        if which == "object":
            f = np.exp(-1j * (phi0 + gy * (yy - yc) + gx * (xx - xc))) / s
        elif which == "probe":
            f = s * np.exp(1j * (gy * yy + gx * xx))
        else:
            raise ValueError(which)
        out[t] = v[t] * f.astype(cdt)
    return out.reshape(lead + (ny, nx)) if x.ndim > 2 else out.reshape(ny, nx)


def fix(psi, scan, probe, floor=0.1, ref=None, dtype=np.float64):
    """The steps of ``fix_gauge`` for ``[ptheta, nz, n]`` inputs."""
    nz, n = np.shape(psi)[-2:]
    ill = illumination(scan, probe, nz, n, dtype)
    lit = ill >= dtype(floor) * ill.max(axis=(-2, -1), keepdims=True)
    g = fit(psi, ill * lit, ref, dtype)
    return {"psi": apply(psi, g, "object", dtype), "probe": apply(probe, g, "probe", dtype), "gauge": g,
            "illumination": ill, "lit": lit}


def angle_diff(a, b):
    """``|a - b|`` taken as angles, in ``[0, pi]``."""
    return np.abs(np.angle(np.exp(1j * (np.asarray(a, np.float64) - np.asarray(b, np.float64)))))


# ---- the illumination cases shared by tests/test_gauge_cpu.py (index walk on the host) and tests/test_hip_gauge.py ------
def random_probe(rng, ptheta, nmodes, nprb):
    """Complex64 ``[ptheta, nmodes, nprb, nprb]`` (``[ptheta, nprb, nprb]`` for ``nmodes = None``), later modes weaker."""
    m = 1 if nmodes is None else nmodes
    p = rng.standard_normal((ptheta, m, nprb, nprb)) + 1j * rng.standard_normal((ptheta, m, nprb, nprb))
    p = (p / (1 + np.arange(m))[None, :, None, None]).astype(np.complex64)
    return p[:, 0] if nmodes is None else p


def case_a_scan():
    """ptheta 2, object 40 x 56, nprb 16, nscan 9: whole-pixel and fractional positions, one at (nz - nprb, n - nprb) + 0.5
    whose +1 taps leave the object, one partly outside beyond that, one negative, one NaN, two identical."""
    nz, n, nprb = 40, 56, 16
    first = [(3.0, 5.0), (10.0, 20.0), (7.25, 30.75), (nz - nprb + 0.5, n - nprb + 0.5), (30.5, 50.25), (-3.25, 4.0),
             (np.nan, 8.0), (12.5, 12.5), (12.5, 12.5)]
    second = [(12.125, 33.0), (12.125, 33.0), (0.0, 0.0), (5.0, np.inf), (nz - nprb + 0.5, n - nprb + 0.5), (2.0, -1.5),
              (35.75, 1.5), (20.0, 17.0), (0.5, 39.875)]
    return np.array([first, second], np.float32), nz, n, nprb


def case_b_scan(seed=5):
    """ptheta 1, object 300 x 333, nprb 128, nscan 200 random positions, some reaching past the far edges."""
    nz, n, nprb = 300, 333, 128
    rng = np.random.default_rng(seed)
    scan = rng.uniform(0, 1, (1, 200, 2)) * np.array([nz - nprb + 20, n - nprb + 20])
    return scan.astype(np.float32), nz, n, nprb
