"""NumPy restatement of the fit residuals (``ptycho_fit_frames`` of include/ptycho_hip.h, ``libtike.hipfft.fit``) and the
inputs that tests/test_fit_cpu.py and tests/test_hip_fit.py share.

``frames_pixels(..., dtype=np.float64)`` is the reference: the intensity is formed in float64 from the complex64
farplanes, every term and every sum in float64.  ``dtype=np.float32`` follows the kernel's formulae: ``|g|^2 = re * re +
im * im`` with each operation rounded to float32, the modes added in order, the scale ``float32((a / b)^2)``, every term
in float32 (``ln x = ln 2 * log2 x``), every sum in float64.  Both also return, per quantity, the sum of the absolute
magnitudes that enter it, which is what an error bound has to be relative to (the quantities cancel).
"""
import numpy as np

LN2_32 = np.float32(0.693147180559945309)
TINY = 1e-32
ULP = 2.0 ** -23

#: (ptheta, nscan, ndet, M), the smallest shapes at which the partition of csrc/k_fit.hpp can go wrong: one wave tile
#: and one frame (A); 324 pixels, a ragged wave tile, two angles (B); five wave tiles over two workgroups, the last one
#: ragged, and two frame ranges (C); 32 wave tiles in eight workgroups, fewer frames than a range (D); two wave tiles and
#: five frame ranges (E); 225 pixels, not a multiple of four: the loads without 16-byte alignment (F)
CASES = {"A": (1, 1, 16, 1), "B": (2, 33, 18, 2), "C": (1, 130, 48, 3), "D": (1, 7, 128, 1), "E": (1, 600, 32, 1),
         "F": (1, 5, 15, 1)}


def _abs2(g, dtype):
    if dtype == np.float64:
        return g.real.astype(np.float64) ** 2 + g.imag.astype(np.float64) ** 2
    re, im = g.real.astype(np.float32), g.imag.astype(np.float32)
    return re * re + im * im            # float32 arrays: each operation rounds


def intensity(g_modes, dtype=np.float64):
    """``sum_m |g_m|^2`` with the modes added in order, starting from the first."""
    total = None
    for g in g_modes:
        v = _abs2(np.asarray(g), dtype)
        total = v if total is None else total + v
    return total


def frames_pixels(g_modes, data, mask=None, ab=None, dtype=np.float64):
    """``{"frames" [ptheta, nscan, 8], "pixels" [ptheta, 4, ndet, ndet], "frames_mag", "pixels_mag"}``, all float64.

    ``g_modes``: sequence of complex64 ``[ptheta, nscan, ndet, ndet]``; ``data``: float32, same shape; ``mask``:
    ``[ndet, ndet]``, nonzero = measured, or None; ``ab``: ``(a, b)`` or None.
    """
    assert dtype in (np.float64, np.float32)
    I = intensity(g_modes, dtype)
    d = np.asarray(data, np.float32).astype(dtype)
    if ab is not None:
        s = float(ab[0]) / float(ab[1])
        I = I * (np.float32(s * s) if dtype == np.float32 else s * s)
    tiny = dtype(TINY)
    with np.errstate(all="ignore"):
        sI, sd = np.sqrt(I), np.sqrt(d)
        diff = sI - sd
        if dtype == np.float32:
            lnI, lnd = LN2_32 * np.log2(I + tiny), LN2_32 * np.log2(d + tiny)
        else:
            lnI, lnd = np.log(I + tiny), np.log(d + tiny)
        terms = [I, d, np.sqrt(I * d), diff * diff, I - d * lnI, d - d * lnd, np.abs(diff), sd]
        mags = [np.abs(I), np.abs(d), np.abs(terms[2]), I + d, I + d * (1 + np.abs(lnI)), d * (1 + np.abs(lnd)), sI + sd, sd]
        maps = [I, d, diff, diff * diff]
        map_mags = [np.abs(I), np.abs(d), sI + sd, I + d]
    assert all(t.dtype == dtype for t in terms + maps)
    m = np.ones(d.shape[-2:], bool) if mask is None else np.asarray(mask) != 0
    keep = lambda x: np.where(m, x.astype(np.float64), 0.0)   # noqa: E731  a select: NaN at an unmeasured pixel is dropped
    return {"frames": np.stack([keep(t).sum((-2, -1)) for t in terms], -1),
            "frames_mag": np.stack([keep(t).sum((-2, -1)) for t in mags], -1),
            "pixels": np.stack([keep(t).sum(1) for t in maps], 1),
            "pixels_mag": np.stack([keep(t).sum(1) for t in map_mags], 1)}


def make_case(name, seed=0, plant=True):
    """``(g_modes [M, ptheta, nscan, ndet, ndet] complex64, data float32)`` of ``CASES[name]``.

    Random farplanes whose amplitude falls by two decades from the detector's corner (DC) to its centre,
    ``d = Poisson(1.3 I)``.  Planted where the shape has room: frame 1 with ``g = 0, d = 0``, frame 2 with ``d = 0`` and
    ``I > 0``, and in every frame a few pixels with ``I = 0, d > 0``.
    """
    ptheta, nscan, ndet, nmodes = CASES[name]
    rng = np.random.default_rng(1000 + seed + sum(ord(c) for c in name))
    f = np.minimum(np.arange(ndet), ndet - np.arange(ndet)) / (ndet / 2.0)
    env = 30.0 * 10.0 ** (-2.0 * np.minimum(1.0, np.hypot(f[:, None], f[None, :])))
    shape = (nmodes, ptheta, nscan, ndet, ndet)
    g = ((rng.standard_normal(shape) + 1j * rng.standard_normal(shape)) * env / np.sqrt(2.0 * nmodes)).astype(np.complex64)
    if plant:
        dark = rng.choice(ndet * ndet, 5, replace=False)
        g.reshape(nmodes, ptheta, nscan, -1)[..., dark] = 0
    data = rng.poisson(1.3 * intensity(g)).astype(np.float32)
    if plant:
        data.reshape(ptheta, nscan, -1)[..., dark] = rng.integers(1, 9, (ptheta, nscan, 5)).astype(np.float32)
        if nscan > 2:
            g[:, :, 1] = 0
            data[:, 1] = 0
            data[:, 2] = 0
    return g, data


def make_mask(ndet, seed=0):
    """Whole rows, a block and scattered pixels unmeasured (0); uint8 ``[ndet, ndet]``."""
    rng = np.random.default_rng(2000 + seed + ndet)
    m = np.ones((ndet, ndet), np.uint8)
    m[ndet // 3] = 0
    m[-2] = 0
    m[2:2 + ndet // 4, ndet // 2:ndet // 2 + ndet // 5] = 0
    m.reshape(-1)[rng.choice(ndet * ndet, max(3, ndet * ndet // 50), replace=False)] = 0
    return m


def flag(values, nsigma=6.0):
    """``flag_frames`` restated: per row, ``|v - median| > nsigma * 1.4826 * MAD`` with the lower median of an even count."""
    v = np.asarray(values, np.float64)
    low = lambda x: np.sort(x, axis=1)[:, (x.shape[1] - 1) // 2][:, None]   # noqa: E731  torch.median's convention
    dev = np.abs(v - low(v))
    return dev > nsigma * 1.4826 * low(dev)
