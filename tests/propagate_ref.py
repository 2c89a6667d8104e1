"""Float64 NumPy restatement of the propagation semantics (include/ptycho_hip.h) and the analytic
Gaussian beam the tests hold it to.  ``precision="single"`` restates the same computation in complex64 arithmetic (the
phase of the transfer function stays float64, as on the device): its error is the yardstick of the device's."""
import numpy as np


def turns(S, zl, q0, method):
    """Reduced phase of the transfer function in turns ``[S, S]`` (float64) and the mask of propagating frequencies."""
    k = np.fft.fftfreq(S) * S
    k2 = k[:, None] ** 2 + k[None, :] ** 2
    q = q0 * k2
    if method == "fresnel":
        t, ok = -0.5 * zl * q, np.ones((S, S), dtype=bool)
    elif method == "angular":
        ok = q <= 1.0
        qs = np.where(ok, q, 0.0)
        t = -zl * qs / (1.0 + np.sqrt(1.0 - qs))
    else:
        raise ValueError(method)
    return t - np.rint(t), ok


def transfer(S, z, wavelength, pixel_size, method="fresnel"):
    """``H`` ``[S, S]`` complex128 (DC at ``[0, 0]``, modulus 1 or 0; the device folds 1 / S^2 into it)."""
    t, ok = turns(S, z / wavelength, (wavelength / (S * pixel_size)) ** 2, method)
    return np.where(ok, np.exp(2j * np.pi * t), 0.0)


def propagate(u, z, wavelength, pixel_size, method="fresnel", precision="double"):
    """``IDFT(DFT(u) H)`` of the last two axes of ``u``."""
    S = u.shape[-1]
    H = transfer(S, z, wavelength, pixel_size, method)
    if precision == "single":
        Hs = (H / (S * S)).astype(np.complex64)
        spec = np.fft.fft2(u.astype(np.complex64))
        assert spec.dtype == np.complex64
        return np.fft.ifft2(spec * Hs, norm="forward")
    return np.fft.ifft2(np.fft.fft2(u.astype(np.complex128)) * H)


def intensity32(plane):
    """``v = |plane|^2`` as the device forms it: complex64, ``round(round(re re) + round(im im))`` in float32."""
    p = np.asarray(plane).astype(np.complex64)
    re, im = p.real.astype(np.float32), p.imag.astype(np.float32)
    return re * re + im * im


def metrics(plane):
    """The eight float64 words of one ``[S, S]`` plane: sums of v, v^2, v y, v x, v y^2, v x^2, max v and the flat index
    of its first maximum (NaN skipped by the max; -inf and -1 if nothing compares)."""
    v32 = intensity32(plane)
    S = v32.shape[-1]
    v = v32.astype(np.float64)
    y = np.arange(S, dtype=np.float64)[:, None]
    x = np.arange(S, dtype=np.float64)[None, :]
    if np.all(np.isnan(v32)):
        top, idx = -np.inf, -1.0
    else:
        idx = float(np.nanargmax(v32))
        top = float(v32.reshape(-1)[int(idx)])
    return np.array([v.sum(), (v * v).sum(), (v * y).sum(), (v * x).sum(), (v * y * y).sum(), (v * x * x).sum(), top, idx])


def sharpness(m):
    return m[..., 1] / m[..., 0] ** 2


def width(m):
    cy, cx = m[..., 2] / m[..., 0], m[..., 3] / m[..., 0]
    return np.sqrt(np.maximum(m[..., 4] / m[..., 0] - cy ** 2 + m[..., 5] / m[..., 0] - cx ** 2, 0.0))


def focus(z, sharp):
    """``(best, focus, bracketed)``: arg-max of the sharpness over the distances ``z`` and the vertex of the parabola
    through its three neighbours (``z[best]`` at an end of the range or without a maximum)."""
    z, sharp = np.asarray(z, dtype=np.float64), np.asarray(sharp, dtype=np.float64)
    b = int(np.argmax(sharp))
    if b == 0 or b == len(z) - 1:
        return b, float(z[b]), False
    c = np.polyfit(z[b - 1:b + 2] - z[b], sharp[b - 1:b + 2] / sharp[b], 2)
    if not c[0] < 0:
        return b, float(z[b]), False
    return b, float(z[b] - c[1] / (2.0 * c[0])), True


def gaussian_beam(S, w0, wavelength, pixel_size, z, centre=None):
    """``u(r, z) = (-i zR / (z - i zR)) exp(i k r^2 / (2 (z - i zR)))``, ``zR = k w0^2 / 2``, sampled on ``S x S`` pixels
    of ``pixel_size`` about ``centre`` (default ``S // 2``): ``|u|`` at the waist is ``exp(-r^2 / w0^2)``."""
    c = S // 2 if centre is None else centre
    ax = (np.arange(S) - c) * pixel_size
    r2 = ax[:, None] ** 2 + ax[None, :] ** 2
    k = 2.0 * np.pi / wavelength
    zr = k * w0 * w0 / 2.0
    qz = z - 1j * zr
    return (-1j * zr / qz) * np.exp(1j * k * r2 / (2.0 * qz))


def rayleigh(w0, wavelength):
    return np.pi * w0 * w0 / wavelength
