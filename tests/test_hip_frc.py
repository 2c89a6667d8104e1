"""Fourier ring correlation on the GPU (``libtike.hipfft.frc``, csrc/k_frc.hpp) against the float64 restatement of
tests/frc_ref.py, plus the properties that fix its meaning: a shifted copy correlates fully once aligned, a known
signal-to-noise ratio crosses where theory puts it, and two reconstructions from data of a higher dose resolve finer.

Tolerances.  Ring sums are compared at the device's own alignment (the restatement takes ``shift=``), ring by ring, in
units of ``sqrt(PA_k PB_k)``: the device may be ``FACTOR`` times the float32 restatement's own error off (with a floor
``SUM_FLOOR`` for rings where float32 happens to be almost exact), and never more than ``SUM_MAX``.  The curve is held to
``FRC_TOL``, the alignment to the CPU oracle's registration within one upsampling step (1/100 px).  The observed errors
behind these figures are in profiles/r05/frc.txt.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import frc_ref as ref  # noqa: E402
from hip_common import bound, dev, pt  # noqa: E402, F401

pytestmark = pytest.mark.gpu

SUM_FLOOR = 1e-5
SUM_MAX = 1e-4
FRC_TOL = 2e-4
SHIFT_TOL = 0.01 + 1e-9


def lowpass(shape, rng, cutoff):
    """Complex field with power spectrum 1 / (1 + (|f| / cutoff)^4), |f| in cycles per pixel, unit variance."""
    nz, n = shape[-2:]
    f = np.hypot(np.fft.fftfreq(nz)[:, None], np.fft.fftfreq(n)[None, :])
    w = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    x = np.fft.ifft2(np.fft.fft2(w) / np.sqrt(1 + (f / cutoff) ** 4))
    return x / x.std()


def fourier_shift(x, d):
    """Periodic shift of the last two axes: out(y, x) = in(y - dy, x - dx)."""
    nz, n = x.shape[-2:]
    ramp = np.exp(-2j * np.pi * (np.fft.fftfreq(nz)[:, None] * d[0] + np.fft.fftfreq(n)[None, :] * d[1]))
    return np.fft.ifft2(np.fft.fft2(x) * ramp)


def pair(ptheta, nz, n, complex_, seed, d=(0.6, -1.3), noise=0.3):
    rng = np.random.default_rng(seed)
    s = lowpass((ptheta, nz, n), rng, 0.15)
    a = s + noise * (rng.standard_normal(s.shape) + 1j * rng.standard_normal(s.shape))
    b = fourier_shift(s, d) + noise * (rng.standard_normal(s.shape) + 1j * rng.standard_normal(s.shape))
    if complex_:
        return a.astype(np.complex64), b.astype(np.complex64)
    return a.real.astype(np.float32), b.real.astype(np.float32)


# S, ptheta, complex input, taper, align: every S of the issue (100 Bluestein, 112 mixed radix), 1 and 3 angles
CASES = [
    (16, 1, True, 0.25, True),
    (64, 3, True, 0.0, True),
    (100, 1, False, 1.0, True),
    (112, 3, True, 0.25, False),
    (256, 1, True, 1.0, True),
    (256, 3, False, 0.25, True),
    (1000, 1, True, 0.25, True),
    (1000, 3, False, 0.0, False),
    (2048, 1, True, 0.25, True),
    (2048, 3, False, 1.0, True),
]


def sum_error(sums, want):
    scale = np.sqrt(want[..., 2] * want[..., 3])
    ok = scale > 0
    return (np.abs(sums[..., :4] - want[..., :4]).max(axis=-1)[ok] / scale[ok]).max()


@pytest.mark.parametrize("s,ptheta,complex_,taper,align", CASES)
def test_frc_matches_the_restatement(pt, s, ptheta, complex_, taper, align):
    lib = sys.modules["libtike.hipfft.frc"]
    a, b = pair(ptheta, s + 7, s + 12, complex_, seed=s + ptheta)
    if ptheta == 1:
        a, b = a[0], b[0]                                   # 2-D input: one angle, no angle axis in the result
    region = (3, 5, s)
    ta, tb = dev(a), dev(b)
    got = pt.frc(ta, tb, region=region, taper=taper, align=align)
    sums, shift = lib.ring_sums(ta, tb, region, taper, align)
    r64 = ref.frc(a, b, region, taper, align, shift=shift)
    r32 = ref.frc(a, b, region, taper, align, precision="single", shift=shift)
    assert np.array_equal(sums[..., 4], r64["sums"][..., 4])
    e_dev, e32 = sum_error(sums, r64["sums"]), sum_error(r32["sums"], r64["sums"])
    e_frc = np.abs(np.reshape(got["frc"], (ptheta, -1)) - r64["frc"]).max()
    print("S %d ptheta %d complex %s taper %.2f align %s: sums err %.2e (float32 restatement %.2e), frc err %.2e"
          % (s, ptheta, complex_, taper, align, e_dev, e32, e_frc))
    assert e_dev <= bound(e32, SUM_FLOOR, SUM_MAX), (e_dev, e32)
    assert e_frc <= FRC_TOL
    assert np.array_equal(got["count"], r64["count"])
    assert np.allclose(got["frequency"], np.arange(s // 2 + 1) / s)
    assert np.allclose(np.reshape(got["threshold"], (ptheta, -1)), r64["threshold"])
    assert np.shape(got["frc"]) == ((s // 2 + 1,) if ptheta == 1 else (ptheta, s // 2 + 1))
    assert np.array_equal(np.reshape(got["shift"], (ptheta, 2)), shift)
    if align:
        want = ref.frc(a, b, region, taper, True)["shift"]
        print("  shift", shift.tolist(), "oracle", want.tolist())
        assert np.abs(shift - want).max() <= SHIFT_TOL
        if s >= 256:
            assert np.abs(shift - np.array([-0.6, 1.3])).max() < 0.1   # b(x) = a(x - d): b moves by -d onto a
    else:
        assert np.all(shift == 0)
    if not complex_:
        assert np.all(np.reshape(got["phase"], -1) == 0)


@pytest.mark.parametrize("s,ptheta", [(100, 1), (256, 3), (2048, 1)])
def test_two_calls_are_bitwise_identical(pt, s, ptheta):
    a, b = pair(ptheta, s, s, True, seed=7)
    ta, tb = dev(a), dev(b)
    r1 = pt.frc(ta, tb)
    r2 = pt.frc(ta, tb)
    for key in r1:
        assert np.array_equal(r1[key], r2[key]), key


def test_shifted_copy_correlates_once_aligned(pt):
    s, d = 256, (3.37, -1.18)
    rng = np.random.default_rng(11)
    w = rng.standard_normal((s, s)) + 1j * rng.standard_normal((s, s))
    a, b = w.astype(np.complex64), fourier_shift(w, d).astype(np.complex64)
    on = pt.frc(dev(a), dev(b), region=(0, 0, s), taper=0.0, align=True)
    k = np.arange(s // 2 + 1)
    assert np.abs(on["shift"] + np.array(d)).max() < 0.01, on["shift"]      # b(x) = a(x - d): b moves by -d
    assert on["frc"][k <= 0.9 * s / 2].min() > 0.999, on["frc"].min()
    off = pt.frc(dev(a), dev(b), region=(0, 0, s), taper=0.0, align=False)
    print("shifted copy: aligned k_c %.2f (crossed %s), unaligned k_c %.2f" % (on["crossing"], on["crossed"],
                                                                             off["crossing"]))
    assert off["crossed"] and off["crossing"] < 0.25 * on["crossing"]
    assert np.all(off["shift"] == 0)


def test_known_snr_crosses_where_theory_puts_it(pt):
    s, k0, var = 512, 60.0, 0.1
    rng = np.random.default_rng(13)
    f = np.hypot(*np.meshgrid(ref.freqs(s), ref.freqs(s), indexing="ij"))
    power = 1.0 / (1 + (f / k0) ** 4)                      # E|S(f)|^2 / S^2; white noise: var
    w = rng.standard_normal((s, s)) + 1j * rng.standard_normal((s, s))
    sig = np.fft.ifft2(np.fft.fft2(w / np.sqrt(2)) * np.sqrt(power))
    noise = lambda: np.sqrt(var / 2) * (rng.standard_normal((s, s)) + 1j * rng.standard_normal((s, s)))  # noqa: E731
    a, b = (sig + noise()).astype(np.complex64), (sig + noise()).astype(np.complex64)
    got = pt.frc(dev(a), dev(b), taper=0.0, align=False)
    want = ref.frc(a, b, taper=0.0, align=False)
    ring = ref.rings(s).ravel()
    keep = ring <= s // 2
    ps = np.bincount(ring[keep], power.ravel()[keep])
    cnt = np.bincount(ring[keep])
    expect = ps / (ps + var * cnt)                          # SNR / (1 + SNR), ring-averaged
    k_an, _ = ref.crossing(expect, ref.threshold(cnt, "half-bit"))
    print("known SNR: k_c device %.3f, restatement %.3f, analytic %.3f" % (got["crossing"], want["crossing"][0], k_an))
    assert got["crossed"]
    assert abs(got["crossing"] - want["crossing"][0]) <= 0.1
    assert abs(got["crossing"] - k_an) <= 0.1 * k_an


def test_higher_dose_resolves_finer_end_to_end(pt):
    """The reference's tests/test_fsc.py scheme at a small size: one scan, two independent Poisson realisations at each
    of two doses 100x apart, each reconstructed (gaussian model, 24 iterations from a flat object), then ``frc`` of each
    pair over the lit square.  Doses and iterations were calibrated with the CPU oracle solver (profiles/r05/frc.txt):
    at dose 0.03 the pair is photon-limited (half period 14.9 px), at dose 3 it is limited by the 24 iterations
    (3.64 px).  Above dose ~100 the position correction (always on, as in the reference) moves single positions by up
    to 15 px in some realisations and the half period no longer orders with the dose: those doses are not used."""
    import torch
    from libtike.hipfft import synthetic as syn
    from oracle import ptycho_oracle as op
    p = syn.make_problem(8, 8, 6, 32, ndet=32, seed=7)
    nz, n, nscan = p["nz"], p["n"], p["nscan"]
    clean = np.abs(op.fwd(p["psi"], p["scan"], p["probe"], 32, "double")) ** 2
    half = {}
    for dose in (0.03, 3.0):
        recs = []
        for r in range(2):
            rng = np.random.default_rng(1000 + r)
            data = (rng.poisson(clean * dose) / dose).astype(np.float32)
            with pt.CGPtychoSolver(nscan, 32, 32, 1, nz, n) as slv:
                slv.verbose = False
                res = slv.run(dev(data), dev(np.ones((1, nz, n), np.complex64)), dev(p["scan"].copy()),
                              dev(p["probe"][:, None].copy()), piter=24)
                recs.append(res["psi"])
        out = pt.frc(recs[0], recs[1], region=(16, 16, 48))
        print("dose %g: k_c %.3f, half period %.3f px, crossed %s, shift %s"
              % (dose, out["crossing"][0], out["half_period_px"][0], out["crossed"][0], out["shift"][0]))
        assert out["crossed"].all()
        half[dose] = out["half_period_px"][0]
        assert torch.isfinite(torch.view_as_real(recs[0])).all()
    assert half[3.0] < 0.5 * half[0.03], half
