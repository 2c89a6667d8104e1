"""Illumination map and gauge fixing on the GPU (``libtike.hipfft.gauge``, csrc/k_gauge.hpp) against the NumPy restatement
of tests/gauge_ref.py, plus the properties that fix their meaning: skipped positions add nothing, the map is the
diagonal of adj o fwd, a planted gauge comes back, gauge-fixed object and probe give the same intensities, and two
copies of one object in different gauges agree after ``fix_gauge``.

Tolerances follow the scheme of tests/test_hip_frc.py: the device may be ``FACTOR`` times the float32 restatement's own
distance from the float64 one off, with a floor for the cases where float32 happens to be almost exact, and never more
than a cap.  Floors and caps are reasoned from the number formats; profiles/r06/gauge.txt records, case by case, the
device's observed error beside the float32 restatement's, and every observed error lies below its floor or its
``FACTOR`` multiple.

``ILL_FLOOR = 1e-6`` is 8 float32 roundings of the largest pixel (a pixel of cases A and C sums at most 36 products, and
fused multiply-adds on the device round differently from the restatement's separate multiply and add);
``ILL_CAP = 1e-4`` is what 1700 float32 additions could lose at worst, more than twice case B's 800 per pixel.
The fit sums in float64 on the device, so it sits at the float64 restatement up to summation order, which the float32
restatement's error says nothing about: ``FIT_FLOOR = 1e-7`` is one float32 rounding of the inputs, and
``FIT_CAP = 1e-6`` (radians per pixel for the ramp, radians, relative scale, pixels of the centre) keeps a ramp error
over the largest object tested, 1100 pixels, near 1e-3 rad, a tenth of the 0.01 rad noise that the end-to-end test
resolves.  ``apply_gauge`` forms its factor in float64 and rounds once: ``APPLY_FLOOR = 2.4e-7`` is two float32
roundings (the product and its scale) of the largest element, ``APPLY_CAP = 1e-3``.
A planted gauge is recovered up to the float32 rounding of the planted ``psi``: every element's phase moves by at most
``2^-23``, a product of two by ``2^-22``, so the ramp is within ``PLANT_G = 2^-22`` rad / pixel, the scale within
``2^-23`` relative, and the phase within ``2^-23 + PLANT_G (nz + n)`` (the ramp's error times the farthest pixel).
The intensity invariance has no floor: ``FACTOR`` times the float32 restatement's own invariance error, taken through
the single-precision oracle transform.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gauge_ref as ref  # noqa: E402
from hip_common import FACTOR, REL_MAX, bound, dev, host, pt  # noqa: E402, F401

pytestmark = pytest.mark.gpu

ILL_FLOOR, ILL_CAP = 1e-6, 1e-4
FIT_FLOOR, FIT_CAP = 1e-7, 1e-6
APPLY_FLOOR, APPLY_CAP = 2.4e-7, 1e-3
PLANT_G, PLANT_S = 2.0 ** -22, 2.0 ** -23
LIT_CAP = 1e-3                # at most 0.1 % of the pixels may sit within rounding of the lit threshold


# ---- illumination -----------------------------------------------------------------------------------------------------
def ill_case(name):
    """scan, probe, nz, n of cases A (M = 1, 3), B and C of the issue."""
    if name == "B":
        scan, nz, n, nprb = ref.case_b_scan()
        return scan, ref.random_probe(np.random.default_rng(21), 1, 2, nprb), nz, n
    scan, nz, n, nprb = ref.case_a_scan()
    nmodes = {"A1": 1, "A3": 3, "C": None}[name]                     # C: a 3-D probe is one mode
    return scan, ref.random_probe(np.random.default_rng(20), 2, nmodes, nprb), nz, n


_ILL = {}


def ill_reference(name):
    """The case with its float64 and float32 restatements, computed once."""
    if name not in _ILL:
        scan, probe, nz, n = ill_case(name)
        _ILL[name] = (scan, probe, nz, n, ref.illumination(scan, probe, nz, n),
                      ref.illumination(scan, probe, nz, n, np.float32))
    return _ILL[name]


def rel_max(got, want):     # not hip_common.rel_max: per plane, each relative to its own largest pixel
    return (np.abs(got.astype(np.float64) - want).max(axis=(-2, -1)) / np.abs(want).max(axis=(-2, -1))).max()


@pytest.mark.parametrize("name", ["A1", "A3", "B", "C"])
def test_illumination_matches_the_restatement(pt, name):
    scan, probe, nz, n, r64, r32 = ill_reference(name)
    got = pt.illumination(dev(scan), dev(probe), nz, n)
    assert got.dtype.is_floating_point and got.element_size() == 4 and tuple(got.shape) == r64.shape
    e_dev, e32 = rel_max(host(got), r64), rel_max(r32, r64)
    print("gauge illumination %s: device err %.2e (float32 restatement %.2e)" % (name, e_dev, e32))
    assert e_dev <= bound(e32, ILL_FLOOR, ILL_CAP), (e_dev, e32)
    into = dev(np.full(r64.shape, np.nan, np.float32))               # out=: written in full, the same bits
    assert pt.illumination(dev(scan), dev(probe), nz, n, out=into) is into
    assert np.array_equal(host(into), host(got))


@pytest.mark.parametrize("name", ["A3", "B"])
def test_skipped_positions_contribute_nothing_and_calls_repeat_bitwise(pt, name):
    scan, probe, nz, n, _, _ = ill_reference(name)
    scan = scan.copy()
    if name == "B":
        scan[0, ::7, 0] = np.nan
        scan[0, 3::11, 1] = -2.5
    first = host(pt.illumination(dev(scan), dev(probe), nz, n))
    assert np.array_equal(first, host(pt.illumination(dev(scan), dev(probe), nz, n)))
    keep = np.array([[ref.split(p[0])[0] and ref.split(p[1])[0] for p in s] for s in scan])
    assert 0 < keep.sum() < keep.size
    for t in range(scan.shape[0]):                                   # per angle: the kept count differs between angles
        kept = np.ascontiguousarray(scan[t][keep[t]][None])
        alone = host(pt.illumination(dev(kept), dev(probe[t:t + 1]), nz, n))
        assert np.array_equal(alone[0], first[t])


@pytest.mark.parametrize("ndet", [16, 32])
def test_illumination_is_the_diagonal_of_adj_fwd(pt, ndet):
    import torch
    nprb, nz, n, nscan, nmodes = 16, 40, 56, 24, 2
    rng = np.random.default_rng(22)
    scan = (rng.uniform(0, 1, (2, nscan, 2)) * np.array([nz - nprb - 1, n - nprb - 1])).astype(np.float32)
    scan[:, :4] = np.floor(scan[:, :4])                              # some whole-pixel ones; all strictly inside
    probe = ref.random_probe(rng, 2, nmodes, nprb)
    ill = host(pt.illumination(dev(scan), dev(probe), nz, n))
    ones = torch.ones((2, nz, n), dtype=torch.complex64, device="cuda")
    total = np.zeros((2, nz, n))
    with pt.PtychoHIP(nscan, nprb, ndet, 2, nz, n) as op:
        for m in range(nmodes):
            prb = dev(probe[:, m])
            total += host(op.adj(op.fwd(ones, dev(scan), prb), dev(scan), prb)).real
    e = rel_max(ill, total)
    print("gauge operator identity ndet %d: err %.2e" % (ndet, e))
    assert e <= REL_MAX, e           # adj against the oracle, relative to the maximum


# ---- fit ----------------------------------------------------------------------------------------------------------------
def smooth_pair(ptheta, nz, n, seed):
    """An object with amplitude and phase texture and a ramp, a reference without the ramp, a weight with a zero border."""
    rng = np.random.default_rng(seed)
    y, x = np.arange(nz)[:, None], np.arange(n)[None, :]
    base = (1 + 0.3 * rng.standard_normal((ptheta, nz, n))) * np.exp(0.2j * rng.standard_normal((ptheta, nz, n)))
    g = rng.uniform(-0.5, 0.5, (ptheta, 2))
    ramp = np.exp(1j * (0.7 + g[:, 0, None, None] * y + g[:, 1, None, None] * x))
    psi = 1.3 * base * ramp * (1 + 0.05 * rng.standard_normal((ptheta, nz, n)))
    w = rng.uniform(0.1, 1.0, (ptheta, nz, n))
    w[:, :2] = w[:, -3:] = w[:, :, :4] = w[:, :, -1:] = 0
    return psi.astype(np.complex64), base.astype(np.complex64), w.astype(np.float32)


def gauge_error(got, want):
    """Largest of: ramp and phase as angles (rad), scale (relative), centre (pixels)."""
    got, want = np.reshape(got, (-1, 6)), np.reshape(want, (-1, 6))
    return max(ref.angle_diff(got[:, :3], want[:, :3]).max(), (np.abs(got[:, 3] - want[:, 3]) / want[:, 3]).max(),
               np.abs(got[:, 4:] - want[:, 4:]).max())


_FIT = {}


@pytest.mark.parametrize("use_ref", [False, True])
@pytest.mark.parametrize("use_weight", [False, True])
@pytest.mark.parametrize("ptheta,nz,n", [(3, 33, 47), (1, 257, 130), (1, 1024, 1030), (2, 1100, 64)])
def test_fit_matches_the_restatement(pt, ptheta, nz, n, use_weight, use_ref):
    if (ptheta, nz, n) not in _FIT:
        _FIT[(ptheta, nz, n)] = smooth_pair(ptheta, nz, n, nz)
    psi, base, w = _FIT[(ptheta, nz, n)]
    if ptheta == 1:
        psi, base, w = psi[0], base[0], w[0]                          # 2-D input: no angle axis in the result
    w, r = (w if use_weight else None), (base if use_ref else None)
    got = pt.fit_gauge(dev(psi), None if w is None else dev(w), None if r is None else dev(r))
    assert got.dtype.is_floating_point and got.element_size() == 8
    assert tuple(got.shape) == ((6,) if ptheta == 1 else (ptheta, 6))
    r64, r32 = ref.fit(psi, w, r), ref.fit(psi, w, r, np.float32)
    e_dev, e32 = gauge_error(host(got), r64), gauge_error(r32, r64)
    print("gauge fit %dx%dx%d weight %s ref %s: device err %.2e (float32 restatement %.2e)"
          % (ptheta, nz, n, use_weight, use_ref, e_dev, e32))
    assert e_dev <= bound(e32, FIT_FLOOR, FIT_CAP), (e_dev, e32)
    again = pt.fit_gauge(dev(psi), None if w is None else dev(w), None if r is None else dev(r))
    assert np.array_equal(host(got), host(again))                     # repeated calls: the same bits


def plant(rng, ptheta, nz, n, gy, gx, phi=0.9, s0=1.7):
    r = (rng.standard_normal((ptheta, nz, n)) + 1j * rng.standard_normal((ptheta, nz, n))).astype(np.complex64)
    w = np.zeros((ptheta, nz, n), np.float32)
    w[:, 3:-4, 5:-2] = rng.uniform(0.2, 1.0, (ptheta, nz - 7, n - 7))
    y, x = np.arange(nz)[:, None], np.arange(n)[None, :]
    w64 = w.astype(np.float64)
    yc = (w64 * y).sum((1, 2), keepdims=True) / w64.sum((1, 2), keepdims=True)
    xc = (w64 * x).sum((1, 2), keepdims=True) / w64.sum((1, 2), keepdims=True)
    psi = s0 * r.astype(np.complex128) * np.exp(1j * (phi + gy * (y - yc) + gx * (x - xc)))
    return psi.astype(np.complex64), r, w, np.array([gy, gx, phi, s0])


def assert_planted(got, want, nz, n, what):
    got = np.reshape(got, (-1, 6))
    eg = ref.angle_diff(got[:, :2], want[:2]).max()
    ep = ref.angle_diff(got[:, 2], want[2]).max()
    es = (np.abs(got[:, 3] - want[3]) / want[3]).max()
    print("gauge planted %s: ramp err %.2e, phase err %.2e, scale err %.2e" % (what, eg, ep, es))
    assert eg <= PLANT_G and es <= PLANT_S and ep <= PLANT_S + PLANT_G * (nz + n), (eg, ep, es)


@pytest.mark.parametrize("nz,n", [(33, 47), (1100, 64)])
@pytest.mark.parametrize("gy,gx", [(0.31, -0.27), (2.5, -2.5)])
def test_fit_recovers_a_planted_gauge(pt, gy, gx, nz, n):
    """(0.31, -0.27): the case of tests/test_gauge_cpu.py; 2.5 rad / pixel: the wrapped phase aliases, the estimator
    works on neighbour products and does not care.  1100 rows are more than the 1024 workgroups of a reduction pass:
    workgroups own two rows, and the finish adds more partial rows than it has threads."""
    psi, r, w, want = plant(np.random.default_rng(23), 2, nz, n, gy, gx)
    assert_planted(host(pt.fit_gauge(dev(psi), dev(w), dev(r))), want, nz, n, "%dx%d (%g, %g)" % (nz, n, gy, gx))


def test_zero_weight_gives_the_identity_and_leaves_the_other_angles_alone(pt):
    psi, base, w = smooth_pair(3, 33, 47, 24)
    w0 = w.copy()
    w0[1] = 0
    got = host(pt.fit_gauge(dev(psi), dev(w0), dev(base)))
    assert np.array_equal(got[1], [0, 0, 0, 1, 0, 0])
    full = host(pt.fit_gauge(dev(psi), dev(w), dev(base)))
    assert np.array_equal(got[[0, 2]], full[[0, 2]])
    alone = host(pt.fit_gauge(dev(psi[2]), dev(w[2]), dev(base[2])))
    assert np.array_equal(alone, full[2])


# ---- apply --------------------------------------------------------------------------------------------------------------
GAUGES = np.array([[0.31, -0.27, 0.9, 1.7, 15.2, 22.9], [-2.5, 1.0, -3.0, 0.4, 0.0, 0.0], [0.0, 0.0, 0.0, 1.0, 3.0, 4.0]])


@pytest.mark.parametrize("which,shape", [("object", (3, 33, 47)), ("object", (257, 130)), ("probe", (3, 2, 16, 16)),
                                         ("probe", (3, 16, 16))])
def test_apply_matches_the_restatement(pt, which, shape):
    rng = np.random.default_rng(25)
    x = (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)
    g = GAUGES[0] if len(shape) == 2 else GAUGES
    xd = dev(x)
    assert pt.apply_gauge(xd, dev(g), which) is xd                   # in place
    r64, r32 = ref.apply(x, g, which), ref.apply(x, g, which, np.float32)
    e_dev = np.abs(host(xd) - r64).max() / np.abs(r64).max()
    e32 = np.abs(r32 - r64).max() / np.abs(r64).max()
    print("gauge apply %s %s: device err %.2e (float32 restatement %.2e)" % (which, shape, e_dev, e32))
    assert e_dev <= bound(e32, APPLY_FLOOR, APPLY_CAP), (e_dev, e32)


def test_object_fixed_by_apply_has_no_ramp_left(pt):
    nz, n = 33, 47
    psi, r, w, _ = plant(np.random.default_rng(26), 2, nz, n, 0.31, -0.27)
    g = pt.fit_gauge(dev(psi), dev(w), dev(r))
    fixed = pt.apply_gauge(dev(psi), g, "object")
    assert_planted(host(pt.fit_gauge(fixed, dev(w), dev(r))), np.array([0.0, 0.0, 0.0, 1.0]), nz, n, "after apply")


# ---- fix_gauge ------------------------------------------------------------------------------------------------------------
def intensities(fwd, psi, scan, probe):
    return sum(np.abs(fwd(psi, scan, probe[:, m])) ** 2 for m in range(probe.shape[1]))


def test_fixed_object_and_probe_give_the_same_intensities(pt):
    from oracle import ptycho_oracle as oracle
    nprb, nz, n, nscan = 32, 80, 96, 12
    rng = np.random.default_rng(27)
    psi = (rng.standard_normal((1, nz, n)) + 1j * rng.standard_normal((1, nz, n))).astype(np.complex64)
    probe = ref.random_probe(rng, 1, 2, nprb)
    scan = np.stack([rng.integers(0, nz - nprb, nscan), rng.integers(0, n - nprb, nscan)], -1)[None].astype(np.float32)
    psi_d, probe_d = dev(psi), dev(probe)
    out = pt.fix_gauge(psi_d, dev(scan), probe_d)
    assert set(out) == {"psi", "probe", "gauge", "illumination", "lit"}
    assert np.array_equal(host(psi_d), psi) and np.array_equal(host(probe_d), probe)   # copies are fixed, inputs kept
    with pt.PtychoHIP(nscan, nprb, nprb, 1, nz, n) as op:
        fwd = lambda f, s, p: host(op.fwd(dev(f), dev(s), dev(p)))  # noqa: E731
        before = intensities(fwd, psi, scan, probe)
        after = intensities(fwd, host(out["psi"]), scan, host(out["probe"]))
    e_dev = np.abs(after - before).max() / before.max()
    # the float32 restatement's own invariance error, through the single-precision oracle transform: the same roundings
    # the two device transforms carry
    f32 = ref.fix(psi, scan, probe, dtype=np.float32)
    o32 = lambda f, s, p: oracle.fwd(f, s, p, nprb, "single")  # noqa: E731
    b32 = intensities(o32, psi, scan, probe)
    e32 = np.abs(intensities(o32, f32["psi"], scan, f32["probe"]) - b32).max() / b32.max()
    print("gauge intensity invariance: device err %.2e (float32 restatement %.2e), gauge %s"
          % (e_dev, e32, host(out["gauge"]).tolist()))
    assert e_dev <= FACTOR * e32, (e_dev, e32)


def two_gauges(seed=28):
    """One object seen twice: ``b`` is ``a`` in another gauge plus 1 % noise.  Probe with a smooth envelope, jittered
    raster: the lit threshold cuts through a slope, not a plateau."""
    nprb, nz, n = 32, 96, 112
    rng = np.random.default_rng(seed)
    y, x = np.arange(nz)[:, None], np.arange(n)[None, :]
    a = (1 + 0.2 * np.sin(y / 5.0) * np.cos(x / 7.0)) * np.exp(0.5j * np.cos(y / 9.0 + x / 11.0))
    noise = 0.01 * (rng.standard_normal((nz, n)) + 1j * rng.standard_normal((nz, n)))
    b = 1.6 * a * np.exp(1j * (1.2 + 0.05 * (y - 40) - 0.08 * (x - 60))) * (1 + noise)
    r = np.hypot(*np.meshgrid(np.arange(nprb) - 15.5, np.arange(nprb) - 15.5, indexing="ij"))
    probe = ref.random_probe(rng, 1, 2, nprb) * 0.2 + np.exp(-(r / 9.0) ** 2)[None, None]
    grid = np.stack(np.meshgrid(np.arange(6, 56, 7.0), np.arange(8, 72, 7.0), indexing="ij"), -1).reshape(-1, 2)
    scan = (grid + rng.uniform(-1.5, 1.5, grid.shape)).astype(np.float32)[None]
    return a[None].astype(np.complex64), b[None].astype(np.complex64), scan, probe.astype(np.complex64), nz, n


def phase_rms(x, a, weight):
    d = np.angle(x.astype(np.complex128) * np.conj(a.astype(np.complex128)))
    return float(np.sqrt((weight * d ** 2).sum() / weight.sum()))


def test_fix_gauge_brings_two_copies_into_one_gauge(pt):
    a, b, scan, probe, nz, n = two_gauges()
    r64 = ref.fix(b, scan, probe, 0.1, a)
    r32 = ref.fix(b, scan, probe, 0.1, a, np.float32)
    w64 = r64["illumination"] * r64["lit"]
    want = phase_rms(r64["psi"], a, w64)
    out = pt.fix_gauge(dev(b), dev(scan), dev(probe), floor=0.1, ref=dev(a))
    got, before = phase_rms(host(out["psi"]), a, w64), phase_rms(b, a, w64)
    print("gauge fix_gauge: phase rms before %.3f, device %.5f, float64 restatement %.5f" % (before, got, want))
    assert got <= 1.5 * want and before > 10 * 1.5 * want
    assert abs(want - 0.01) < 0.003                                  # the noise level that was put in
    # the mask: equal to the restatement's except where the illumination is within rounding of the threshold
    ill64 = r64["illumination"]
    peak = ill64.max()
    e32 = rel_max(r32["illumination"], ill64)
    near = np.abs(ill64 - 0.1 * peak) <= bound(e32, ILL_FLOOR, ILL_CAP) * peak * (1 + 0.1)   # the pixel's and the peak's error
    lit = host(out["lit"])
    assert lit.dtype == np.bool_ and lit.shape == ill64.shape
    print("gauge fix_gauge: lit fraction %.3f, pixels near the threshold %d of %d, float32 restatement differs at %d"
          % (lit.mean(), near.sum(), near.size, (r32["lit"] != r64["lit"]).sum()))
    assert near.mean() <= LIT_CAP and (r32["lit"] != r64["lit"]).mean() <= LIT_CAP
    assert np.array_equal(lit[~near], r64["lit"][~near])
    assert rel_max(host(out["illumination"]), ill64) <= bound(e32, ILL_FLOOR, ILL_CAP)
