"""NumPy restatement of the frame preparation (``ptycho_prepare_frames`` of include/ptycho_hip.h,
``libtike.hipfft.prepare.prepare_frames``) and the inputs of its tests.

``prepare`` follows the definition operation by operation: float32 terms, each operation rounded, the bin summed in the
order ``by`` outer, ``bx`` inner from the first term, float64 sums.  ``data`` and ``mask`` of the device are these bits;
the float64 sums of the device are formed in another order and agree within ``N * 2^-52 * mag``, ``mag`` the sum of the
absolute terms (``frames_mag`` / ``pixels_mag``) and ``N`` their number.
"""
import numpy as np

#: name -> (ptheta, nscan, ndet): the shapes whose partition tests/test_prepare_cpu.py walks
CASES = {"A": (1, 1, 16), "B": (2, 3, 24), "C": (1, 290, 16), "D": (1, 2, 15), "E": (1, 3, 32), "F": (1, 7, 64),
         "G": (1, 2, 24), "H": (2, 3, 16)}


def window_origin(shape, ndet, center=None, bin=1):
    H, W = shape[-2:]
    cy, cx = (H // 2, W // 2) if center is None else center
    return cy - (ndet // 2) * bin, cx - (ndet // 2) * bin


def prepare(raw, ndet, center=None, bin=1, dark=None, gain=None, bad=None, index=None, saturation=None, scale=1.0,
            clip=True):
    """The outputs of ``prepare_frames`` as host arrays, plus ``frames_mag`` / ``pixels_mag`` (sums of absolute terms of
    columns / maps 0 and 1) and ``centred``, the window before the shift."""
    raw4 = raw if raw.ndim == 4 else raw[None]
    ptheta, nraw, H, W = raw4.shape
    y0, x0 = window_origin(raw4.shape, ndet, center, bin)
    nb = ndet * bin
    ys, xs = y0 + np.arange(nb), x0 + np.arange(nb)
    inside = ((ys >= 0) & (ys < H))[:, None] & ((xs >= 0) & (xs < W))[None, :]
    yc, xc = np.clip(ys, 0, H - 1)[:, None], np.clip(xs, 0, W - 1)[None, :]
    take = lambda a, fill: np.full((nb, nb), fill, np.float32) if a is None else a[yc, xc].astype(np.float32)  # noqa: E731
    dk, gn = take(dark, 0.0), take(gain, 1.0)
    is_bad = np.zeros((nb, nb), bool) if bad is None else np.asarray(bad)[yc, xc] != 0
    idx = np.broadcast_to(np.arange(nraw), (ptheta, nraw)) if index is None else np.asarray(index).reshape(ptheta, -1)
    nscan = idx.shape[1]
    valid = (idx >= 0) & (idx < nraw)
    win = np.stack([raw4[t][np.where(valid[t], idx[t], 0)][:, yc, xc] for t in range(ptheta)]).astype(np.float32)
    with np.errstate(all="ignore"):
        t = ((win - dk) * gn).astype(np.float32).reshape(ptheta, nscan, ndet, bin, ndet, bin)
        v = None
        for by in range(bin):
            for bx in range(bin):
                term = t[:, :, :, by, :, bx]
                v = term.copy() if v is None else (v + term).astype(np.float32)
        if clip:
            v = np.where(v < 0, np.float32(0), v)
        v = (v * np.float32(scale)).astype(np.float32)
        sat = np.zeros(win.shape, bool) if saturation is None else win >= np.float32(saturation)
        nsat = sat.reshape(ptheta, nscan, ndet, bin, ndet, bin).sum((3, 5))
        meas = (inside & ~is_bad).reshape(ndet, bin, ndet, bin).all((1, 3))
        ok = meas[None, None] & valid[:, :, None, None]
        v = np.where(ok, v, np.float32(0)).astype(np.float32)
        nsat = np.where(ok, nsat, 0)
        v2 = (v * v).astype(np.float32)
        low = np.where(ok, v, np.float32(-np.inf))                      # fmax skips a NaN; -inf: nothing measured
        v64, v264 = v.astype(np.float64), v2.astype(np.float64)
        frames = np.stack([v64.sum((2, 3)), v264.sum((2, 3)), np.fmax.reduce(low.reshape(ptheta, nscan, -1), axis=2,
                           initial=-np.inf).astype(np.float64), nsat.sum((2, 3)).astype(np.float64)], -1)
        frames = np.where(valid[:, :, None], frames, 0.0)              # an index out of range: four zeros
        frames_mag = np.stack([np.abs(v64).sum((2, 3)), np.abs(v264).sum((2, 3))], -1)
        pmax = np.where(meas[None], np.fmax.reduce(low, axis=1, initial=-np.inf).astype(np.float64), 0.0)
        pixels = np.stack([v64.sum(1), v264.sum(1), pmax, (nsat > 0).sum(1).astype(np.float64)], 1)
        pixels_mag = np.stack([np.abs(v64).sum(1), np.abs(v264).sum(1)], 1)
    shift = lambda a: np.fft.ifftshift(a, axes=(-2, -1))  # noqa: E731
    return {"data": np.ascontiguousarray(shift(v)), "mask": np.ascontiguousarray(shift(meas)).astype(np.uint8),
            "frames": frames, "pixels": np.ascontiguousarray(shift(pixels)), "frames_mag": frames_mag,
            "pixels_mag": np.ascontiguousarray(shift(pixels_mag)), "centred": v, "measured": meas}


def make_case(name):
    """``(raw, kwargs)`` of case ``name``: ``prepare(raw, **kwargs)`` / ``prepare_frames(raw, **kwargs)``.  Seeded."""
    rng = np.random.default_rng(1000 + ord(name))
    ptheta, nscan, ndet = CASES[name]
    if name == "A":      # less than one wave tile (256 pixels is exactly one), one frame, every default
        return rng.integers(0, 65536, (1, 16, 16), dtype=np.uint16), {"ndet": 16}
    if name == "B":      # three wave tiles, the last partial; odd frame count; non-square raw; index: a repeat, out of range
        raw = rng.integers(-50, 5000, (2, 5, 40, 36)).astype(np.int32)
        index = np.array([[3, 3, 7], [4, -1, 0]], np.int64)
        return raw, {"ndet": 24, "center": (19, 17), "index": index, "scale": 0.5}
    if name == "C":      # three frame ranges, the last one shorter; clip, dark, gain, bad pixels, garbage under them
        raw = (rng.random((nscan, 32, 32)) * 40 - 4).astype(np.float32)
        dark = (rng.random((32, 32)) * 8).astype(np.float32)
        gain = (0.5 + rng.random((32, 32))).astype(np.float32)
        bad = np.zeros((32, 32), np.uint8)
        bad[[3, 3, 17, 30, 12], [4, 5, 16, 1, 31]] = [1, 7, 255, 1, 2]
        raw[:, 3, 4], raw[5, 3, 5], raw[:, 17, 16] = np.nan, np.inf, -np.inf
        dark[30, 1], gain[12, 31] = np.nan, np.inf
        return raw, {"ndet": 16, "bin": 2, "dark": dark, "gain": gain, "bad": bad, "scale": 0.25}
    if name == "D":      # odd ndet: scalar path, ifftshift != fftshift; uint32 above 2^24 rounds on conversion
        raw = rng.integers(2 ** 24, 2 ** 32, (nscan, 20, 21), dtype=np.uint32)
        raw[0, 10, 10] = 2 ** 32 - 1
        return raw, {"ndet": 15}
    if name == "E":      # bin 4, the window overhangs the top and the right edge; saturated pixels
        raw = rng.integers(0, 50000, (nscan, 100, 90), dtype=np.uint16)
        raw[0, 5, 20], raw[0, 6, 21], raw[2, 30, 50], raw[1, 2, 89] = 60000, 65535, 60000, 61000
        raw[1, 90, 30] = 65535                                                    # outside the window: not counted
        return raw, {"ndet": 32, "bin": 4, "center": (20, 80), "saturation": 60000}
    if name == "F":      # odd x0 and W: scalar loads, 16-byte stores
        return rng.integers(0, 65536, (nscan, 80, 83), dtype=np.uint16), {"ndet": 64, "center": (40, 41)}
    if name == "G":      # bin 4 with vector loads, the window overhangs every edge by whole runs; gain
        raw = rng.integers(0, 65536, (nscan, 64, 64), dtype=np.uint16)
        gain = (0.5 + rng.random((64, 64))).astype(np.float32)
        return raw, {"ndet": 24, "bin": 4, "center": (40, 44), "gain": gain, "saturation": 65000}
    if name == "H":      # bin 2 of 16-bit counts with vector loads, two angles, dark above some counts, a bad pixel
        raw = rng.integers(0, 3000, (2, nscan, 40, 40), dtype=np.uint16)
        dark = (rng.random((40, 40)) * 2000).astype(np.float32)
        bad = np.zeros((40, 40), bool)
        bad[9, 9] = bad[20, 21] = True
        return raw, {"ndet": 16, "bin": 2, "dark": dark, "bad": bad, "clip": False, "saturation": 2990.5}
    raise KeyError(name)


def sums_close(got, want, mag, nterms):
    """Float64 sums in any order: ``|got - want| <= nterms * 2^-52 * mag``; non-finite entries must be the same."""
    fin = np.isfinite(want)
    same = np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)])
    with np.errstate(invalid="ignore"):
        return same and bool((np.abs(got - want)[fin] <= nterms * 2.0 ** -52 * mag[fin]).all())
