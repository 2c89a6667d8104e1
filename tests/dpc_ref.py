"""NumPy restatement of ``libtike.hipfft.dpc`` (include/ptycho_hip.h): the moments of every
diffraction pattern in float64, the scan map in float32 with the device's operations in the device's order (so that it
can be compared bit for bit), the integration of a gradient field with the conjugate gradients of tests/unwrap_ref.py,
and ``first_look`` / ``initial_object`` on top of them.  Not collected by pytest.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gauge_ref  # noqa: E402
import unwrap_ref  # noqa: E402

F32 = np.float32


# ---- frame moments ------------------------------------------------------------------------------------------------------
def moment_k(ndet):
    """Signed frequency indices of an ``ndet``-point transform with DC at 0: ``np.fft.fftfreq(ndet) * ndet`` as integers."""
    r = np.arange(ndet)
    return np.where(r < ndet - ndet // 2, r, r - ndet).astype(np.float64)


def moment_terms(data, mask=None, darkfield=None):
    """The eight terms of every pixel, float64 ``[ptheta, nscan, 8, ndet, ndet]``; an unmeasured pixel has ``I = 0`` by a
    select."""
    d = np.asarray(data, np.float32).astype(np.float64)
    ndet = d.shape[-1]
    if mask is not None:
        d = np.where(np.asarray(mask) != 0, d, 0.0)
    k = moment_k(ndet)
    ky, kx = k[:, None] * np.ones(ndet), np.ones(ndet)[:, None] * k[None, :]
    dark = np.zeros((ndet, ndet), bool) if darkfield is None or darkfield < 0 else ky * ky + kx * kx > float(darkfield) ** 2
    if mask is not None:
        dark = dark & (np.asarray(mask) != 0)
    with np.errstate(invalid="ignore"):
        terms = [d, d * ky, d * kx, d * (ky * ky), d * (kx * kx), d * (ky * kx), np.where(dark, d, 0.0), np.zeros_like(d)]
    return np.stack(terms, axis=2)


def frame_moments(data, mask=None, darkfield=None):
    """``(moments, bound)``: float64 ``[ptheta, nscan, 8]`` and per figure the worst-case distance ``npix 2^-53 sum |term|``
    of a float64 sum of the same terms in another order."""
    t = moment_terms(data, mask, darkfield)
    npix = t.shape[-1] * t.shape[-2]
    return t.sum(axis=(-2, -1)), npix * 2.0 ** -53 * np.abs(t).sum(axis=(-2, -1))


def centers(moments):
    """``[ptheta, nscan, 2]``: columns 1 and 2 over column 0, NaN for an empty frame."""
    with np.errstate(invalid="ignore", divide="ignore"):
        c = moments[..., 1:3] / moments[..., 0:1]
    return np.where(moments[..., 0:1] != 0, c, np.nan)


# ---- scan map -------------------------------------------------------------------------------------------------------------
def scan_map(values, scan, probe, nz, n, keep=None, weight=None):
    """``(weight [ptheta, nz, n], out [ptheta, nval, nz, n], num)`` in float32: positions in order, taps in the order (0,0)
    (0,1) (1,0) (1,1), ``A = sum_m (re^2 + im^2)``, ``num_c = num_c + (w_ab A) v_c`` with every operation rounded (NumPy
    fuses nothing), ``out_c = num_c / weight`` where ``weight > 0``, else 0.

    ``num`` is the device's to the bit.  The weight is the illumination of the kept positions; on the device it is formed
    by the illumination kernel, some of whose multiply-adds the compiler fuses, so the float32 weight formed here
    (``gauge_ref``'s, nothing fused) is close to it but not its bits: give the device's ``weight`` to get the device's
    ``out`` bit for bit."""
    scan = np.asarray(scan, F32)
    values = np.asarray(values, F32)
    ptheta, nscan, nval = values.shape
    a2 = gauge_ref.amp2(probe, F32)
    nprb = a2.shape[-1]
    own = np.zeros((ptheta, nz, n), F32)
    num = np.zeros((ptheta, nval, nz, n), F32)
    one = F32(1)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(ptheta):
            for j in range(nscan):
                if keep is not None and not keep[t, j]:
                    continue
                vy, sy, fy = gauge_ref.split(scan[t, j, 0])
                vx, sx, fx = gauge_ref.split(scan[t, j, 1])
                if not (vy and vx):
                    continue
                wy, wx = (F32(one - fy), fy), (F32(one - fx), fx)
                for a in (0, 1):
                    for b in (0, 1):
                        w = F32(wx[b] * wy[a])
                        h, wd = min(nprb, nz - sy - a), min(nprb, n - sx - b)
                        if h <= 0 or wd <= 0:
                            continue
                        ys, xs = slice(sy + a, sy + a + h), slice(sx + b, sx + b + wd)
                        wa = (w * a2[t, :h, :wd]).astype(F32)
                        own[t, ys, xs] += wa
                        for c in range(nval):
                            num[t, c, ys, xs] = (num[t, c, ys, xs] + (wa * values[t, j, c]).astype(F32)).astype(F32)
        weight = own if weight is None else np.asarray(weight, F32)
        lit = weight > 0
        out = np.where(lit[:, None], num / np.where(lit, weight, one)[:, None], F32(0)).astype(F32)
    return weight, out, num


# ---- integration of a gradient field ------------------------------------------------------------------------------------------
def gradient_edges(gy, gx, weight=None, dtype=np.float64):
    """``(wx, dx, wy, dy)`` as ``unwrap_ref.edges``, with ``d_e = (g_p + g_q) / 2`` of ``gx`` along rows and ``gy`` along
    columns; an edge of weight 0 has difference 0 whatever the field holds."""
    gy, gx = np.asarray(gy, dtype), np.asarray(gx, dtype)
    w = unwrap_ref.effective_weight(weight, gy.shape, dtype)
    wx, wy = np.minimum(w[:, :-1], w[:, 1:]), np.minimum(w[:-1], w[1:])
    half = dtype(0.5)
    with np.errstate(invalid="ignore", over="ignore"):
        dx = np.where(wx > 0, half * (gx[:, :-1] + gx[:, 1:]), dtype(0)).astype(dtype)
        dy = np.where(wy > 0, half * (gy[:-1] + gy[1:]), dtype(0)).astype(dtype)
    return wx, dx, wy, dy


def integrate(gy, gx, weight=None, tol=1e-4, maxiter=None, dtype=np.float64):
    """One angle: the least-squares surface of the gradient field minus its weighted mean, 0 where ``D = 0``."""
    gy32, gx32 = np.asarray(gy, F32), np.asarray(gx, F32)
    w = unwrap_ref.effective_weight(weight, gy32.shape, dtype)
    wx, dx, wy, dy = gradient_edges(gy32.astype(dtype), gx32.astype(dtype), weight, dtype)
    b = unwrap_ref.rhs(wx, dx, wy, dy).astype(dtype)
    x, info = unwrap_ref.pcg(wx, wy, b, tol, maxiter, dtype)
    on = info["D"] > 0
    x64, w64 = x.astype(np.float64), np.where(on, w.astype(np.float64), 0.0)
    tot = w64.sum()
    c = float((w64 * np.where(on, x64, 0.0)).sum() / tot) if tot > 0 else 0.0
    out = np.where(on, (x64 - c).astype(F32), F32(0))
    return {"phase": out, "x": x, "offset": c, "iterations": info["iterations"], "status": info["status"],
            "converged": info["converged"], "residual": info["residual"], "D": info["D"]}


# ---- first look -------------------------------------------------------------------------------------------------------------
def first_look(data, scan, probe, nz, n, mask=None, reference="mean", keep=None, floor=0.05, darkfield=None, tol=1e-4,
               maxiter=None, dtype=np.float64):
    """The steps of ``first_look``; the moments are float64 and the map float32 whatever ``dtype`` is, which the integration
    alone follows."""
    data = np.asarray(data, F32)
    ptheta, nscan, ndet = data.shape[:3]
    mom, _ = frame_moments(data, mask, darkfield)
    cen = centers(mom)
    used = np.ones((ptheta, nscan), bool) if keep is None else np.asarray(keep) != 0
    with np.errstate(invalid="ignore"):
        used = used & (mom[..., 0] > 0) & np.isfinite(mom[..., :3]).all(-1)
    if isinstance(reference, str):
        m = np.where(used[..., None], mom[..., :3], 0.0).sum(axis=1)
        with np.errstate(invalid="ignore", divide="ignore"):
            c0 = np.where(m[:, 0:1] > 0, m[:, 1:3] / m[:, 0:1], 0.0)
    else:
        c0 = np.broadcast_to(np.asarray(reference, np.float64), (ptheta, 2))
    g = (2.0 * np.pi / ndet) * (cen - c0[:, None, :])
    values = np.stack([mom[..., 0], mom[..., 6], g[..., 0], g[..., 1]], -1)
    values = np.where(used[..., None], values, 0.0).astype(F32)
    weight, out, _ = scan_map(values, scan, probe, nz, n, used)
    top = weight.max(axis=(-2, -1), keepdims=True)
    lit = (weight >= F32(floor) * top) & (weight > 0)
    w = np.where(lit, weight / np.where(top > 0, top, F32(1)), F32(0)).astype(F32)
    power = F32((np.abs(np.asarray(probe, np.complex64).astype(np.complex128)) ** 2).reshape(ptheta, -1).sum(1))
    res = [integrate(out[t, 2], out[t, 3], w[t], tol, maxiter, dtype) for t in range(ptheta)]
    look = {"moments": mom, "transmission": (out[:, 0] / power[:, None, None]).astype(F32), "darkfield": out[:, 1],
            "dpc_y": out[:, 2], "dpc_x": out[:, 3], "phase": np.stack([r["phase"] for r in res]), "illumination": weight,
            "lit": lit, "reference": c0}
    for key in ("iterations", "residual", "converged", "status"):
        look[key] = np.array([r[key] for r in res])
    return look


def initial_object(look, amplitude=True):
    amp = np.sqrt(np.maximum(look["transmission"], F32(0))) if amplitude else np.ones_like(look["transmission"])
    psi = (amp * np.exp(1j * look["phase"].astype(np.float64))).astype(np.complex64)
    return np.where(look["lit"], psi, np.complex64(1))


# ---- the scenario of the issue ------------------------------------------------------------------------------------------------
def scenario(seed=3):
    """Object 96 x 112 with 7.7 rad of phase, a curved Gaussian probe of 16 pixels, 864 jittered raster positions."""
    nz, n, nprb, ndet = 96, 112, 16, 32
    y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    phi = (5 * np.exp(-((y - 50) ** 2 + (x - 60) ** 2) / (2 * 18.0 ** 2)) - 3 * np.exp(-((y - 30) ** 2 + (x - 35) ** 2) / (2 * 10.0 ** 2))
           + 0.02 * (x - 56))
    amp = 1 - 0.3 * np.exp(-((y - 60) ** 2 + (x - 40) ** 2) / (2 * 12.0 ** 2))
    psi = (amp * np.exp(1j * phi)).astype(np.complex64)[None]
    r = np.arange(nprb) - (nprb - 1) / 2
    r2 = r[:, None] ** 2 + r[None, :] ** 2
    probe = (np.exp(-r2 / (2 * 3.0 ** 2)) * np.exp(0.03j * r2)).astype(np.complex64)[None]
    py, px = np.meshgrid(np.arange(0, nz - nprb - 1, 3.0), np.arange(0, n - nprb - 1, 3.0), indexing="ij")
    grid = np.stack([py.ravel(), px.ravel()], -1)
    scan = (grid + np.random.default_rng(seed).uniform(0, 0.9, grid.shape)).astype(np.float32)[None]
    return {"psi": psi, "phi": phi, "amp": amp, "probe": probe, "scan": scan, "nz": nz, "n": n, "nprb": nprb, "ndet": ndet}


def weighted_rms_error(phase, truth, weight, ramp=False):
    """Relative rms of ``phase - truth`` under ``weight`` after the weighted mean of both is removed; ``ramp=True`` removes
    the weighted least-squares plane of the difference as well (a ramp on the object is gauge)."""
    w = np.asarray(weight, np.float64)
    a = phase.astype(np.float64) - np.average(phase.astype(np.float64), weights=w)
    b = truth - np.average(truth, weights=w)
    d = a - b
    if ramp:
        y, x = np.meshgrid(np.arange(float(w.shape[0])), np.arange(float(w.shape[1])), indexing="ij")
        on = w > 0
        basis = np.stack([np.ones_like(x), y, x], -1)[on]
        coef = np.linalg.lstsq(basis * np.sqrt(w[on])[:, None], d[on] * np.sqrt(w[on]), rcond=None)[0]
        d = np.where(on, d - (coef[0] + coef[1] * y + coef[2] * x), 0.0)
    return float(np.sqrt((w * d ** 2).sum() / (w * b ** 2).sum()))


def weighted_correlation(a, b, weight):
    w = np.asarray(weight, np.float64)
    a = a.astype(np.float64) - np.average(a.astype(np.float64), weights=w)
    b = b.astype(np.float64) - np.average(b.astype(np.float64), weights=w)
    return float((w * a * b).sum() / np.sqrt((w * a * a).sum() * (w * b * b).sum()))
