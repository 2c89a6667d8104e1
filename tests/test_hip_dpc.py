"""First look on the device (``libtike.hipfft.dpc``, csrc/k_dpc.hpp) against the NumPy restatement of tests/dpc_ref.py.

Tolerances.
* Moments: every figure is a float64 sum of terms that both sides form alike, in another order: the worst case of that
  is ``npix 2^-53 sum |term|`` per figure, which is the bound.
* Scan map: bit for bit.  The numerator is float32 with every operation rounded, in one order, so the restatement has the
  device's bits; the weight is ``illumination``'s bits because the illumination kernel itself forms it (the compiler
  fuses some of that kernel's multiply-adds, so no NumPy statement has its bits: the restatement's own float32 weight is
  held to the illumination tolerance of tests/test_hip_gauge.py), the numerators (``normalize=False``) are compared bit
  for bit with the restatement's, and ``out`` with the restatement's numerator over the device's weight.
* Integration: the scheme of tests/test_hip_unwrap.py, ``FACTOR`` times the float32 restatement's own distance from the
  float64 one, with the floor that the issue sets for each comparison (1e-6 for the planted surfaces, whose values stay
  below 2 where a float32 spacing is 1.2e-7; 1e-5 for the first look, whose phase spans 8 rad over 300 iterations).
* End to end: phase within 0.09 (weighted relative rms) of the truth and a first logged cost of at most 0.25 of the cost
  logged from ``psi = 1``: the bounds of tests/test_dpc_cpu.py, measured there as 0.043 and 0.04.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dpc_ref as ref  # noqa: E402
import gauge_ref  # noqa: E402
from hip_common import FACTOR, bound, dev, host, pt, same_bits  # noqa: E402, F401

pytestmark = pytest.mark.gpu


# ---- 1. moments -------------------------------------------------------------------------------------------------------------
MOMENT_SHAPES = [(1, 1, 16), (2, 33, 18), (1, 130, 48), (1, 7, 128), (1, 600, 32), (1, 5, 15)]


def moment_case(shape):
    rng = np.random.default_rng(sum(shape))
    data = rng.gamma(0.7, 40.0, shape + shape[-1:]).astype(np.float32)
    mask = rng.uniform(size=shape[-1:] * 2) > 0.15
    return data, mask


@pytest.mark.parametrize("shape", MOMENT_SHAPES)
def test_moments_against_the_restatement(pt, shape):
    data, mask = moment_case(shape)
    ndet = shape[-1]
    for m, radius in ((None, None), (mask, None), (None, 0.3 * ndet), (mask, 0.3 * ndet)):
        want, bound = ref.frame_moments(data, m, radius)
        got = pt.frame_moments(dev(data), None if m is None else dev(m), radius)
        mom = host(got["moments"])
        err = np.abs(mom - want)
        print("moments %s mask %s darkfield %s: largest error over bound %.3f" % (shape, m is not None, radius,
                                                                                 (err / np.maximum(bound, 1e-300)).max()))
        assert mom.shape == shape[:2] + (8,) and mom.dtype == np.float64
        assert (err <= bound).all(), (err / np.maximum(bound, 1e-300)).max()
        assert (mom[..., 7] == 0).all() and ((mom[..., 6] == 0).all() if radius is None else (mom[..., 6] > 0).any())
        assert same_bits(host(got["sum"]), mom[..., 0]) and same_bits(host(got["darkfield"]), mom[..., 6])
        assert np.allclose(host(got["center"]), ref.centers(want), rtol=1e-12, atol=1e-12)
    # NumPy arrays in: the same bits
    assert same_bits(host(pt.frame_moments(data, mask, 0.3 * ndet)["moments"]), mom)


@pytest.mark.parametrize("shape", [(2, 33, 18), (1, 130, 48), (1, 5, 15)])
def test_moments_nan_views_permutations_repeats(pt, shape):
    data, mask = moment_case(shape)
    base = host(pt.frame_moments(dev(data), dev(mask), 3.0)["moments"])
    dirty = data.copy()
    dirty[:, :, ~mask] = np.resize(np.array([np.nan, np.inf, -np.inf], np.float32), dirty[:, :, ~mask].shape)
    assert same_bits(host(pt.frame_moments(dev(dirty), dev(mask), 3.0)["moments"]), base)     # unmeasured: never matters
    y, x = (int(v[0]) for v in np.nonzero(mask))
    dirty[-1, 1 % shape[1], y, x] = np.nan                               # measured: stays in its frame
    got = host(pt.frame_moments(dev(dirty), dev(mask), 3.0)["moments"])
    bad = np.zeros(shape[:2], bool)
    bad[-1, 1 % shape[1]] = True
    assert np.isnan(got[bad][:, 0]).all() and same_bits(got[~bad], base[~bad])
    assert np.isnan(host(pt.frame_moments(dev(dirty), dev(mask))["center"])[bad]).all()
    # an unaligned view (offset of one float): scalar loads, the same bits
    flat = torch.empty(data.size + 1, dtype=torch.float32, device="cuda")
    view = flat[1:].view(data.shape)
    view.copy_(dev(data))
    assert view.data_ptr() % 16 == 4 and view.is_contiguous()
    assert same_bits(host(pt.frame_moments(view, dev(mask), 3.0)["moments"]), base)
    # permuting frames permutes rows; repeated calls give the same bits
    perm = np.random.default_rng(0).permutation(shape[1])
    assert same_bits(host(pt.frame_moments(dev(data[:, perm]), dev(mask), 3.0)["moments"]), base[:, perm])
    assert same_bits(host(pt.frame_moments(dev(data), dev(mask), 3.0)["moments"]), base)
    empty = data.copy()
    empty[0, 0] = 0
    assert np.isnan(host(pt.frame_moments(dev(empty))["center"])[0, 0]).all()


# ---- 2. scan map ------------------------------------------------------------------------------------------------------------
def map_case(nz, n, nprb, nmodes, nscan, nval, ptheta=1, seed=0):
    rng = np.random.default_rng(seed + nz + nprb + nscan)
    probe = gauge_ref.random_probe(rng, ptheta, nmodes, nprb)
    scan = (rng.uniform(0, 1, (ptheta, nscan, 2)) * np.array([nz - nprb + 4, n - nprb + 4])).astype(np.float32)
    scan[0, 0] = (nz - nprb + 0.5, n - nprb + 0.5)          # on the border: the +1 taps are dropped
    scan[0, 1] = (nz - nprb, n - nprb)                       # whole-pixel, flush with the corner
    scan[0, 2] = (-2.5, 3.0)
    scan[-1, 3] = (np.nan, 4.0)
    scan[-1, 4] = (0.0, 0.0)
    scan[-1, nscan - 1] = (3.25, n + 5.0)                    # beyond the object
    values = rng.normal(1.0, 2.0, (ptheta, nscan, nval)).astype(np.float32)
    values[0, 2] = np.nan                                    # a skipped position may hold anything
    return values, scan, probe


MAP_CASES = [(37, 70, 5, 1, 130, 1), (37, 70, 16, 2, 300, 4), (64, 128, 16, 1, 130, 2), (64, 128, 5, 2, 300, 4)]


@pytest.mark.parametrize("nz, n, nprb, nmodes, nscan, nval", MAP_CASES)
def test_scan_map_bit_for_bit(pt, nz, n, nprb, nmodes, nscan, nval):
    ptheta = 2 if nprb == 5 else 1
    values, scan, probe = map_case(nz, n, nprb, nmodes, nscan, nval, ptheta)
    w, out = pt.scan_map(dev(values), dev(scan), dev(probe), nz, n)
    w, out = host(w), host(out)
    assert same_bits(w, host(pt.illumination(dev(scan), dev(probe), nz, n)))                   # the illumination's bits
    rw, rout, rnum = ref.scan_map(values, scan, probe, nz, n, weight=w)
    assert out.shape == (ptheta, nval, nz, n) and same_bits(out, rout)
    nw, num = pt.scan_map(dev(values), dev(scan), dev(probe), nz, n, normalize=False)          # the numerators themselves
    assert same_bits(host(nw), w) and same_bits(host(num), rnum)
    own, _, _ = ref.scan_map(values[..., :1], scan, probe, nz, n)                              # nothing fused: close, not equal
    r64 = gauge_ref.illumination(scan, probe, nz, n)
    e_dev, e32 = np.abs(w - r64).max() / r64.max(), np.abs(own - r64).max() / r64.max()
    print("scan map %s: weight err %.2e (float32 restatement %.2e), %d lit pixels" % ((nz, n, nprb, nmodes, nscan, nval),
                                                                                      e_dev, e32, (w > 0).sum()))
    assert e_dev <= bound(e32, 1e-6, 1e-4)           # ILL_FLOOR, ILL_CAP of tests/test_hip_gauge.py
    assert (w > 0).any() and (w == 0).any() and np.isfinite(out).all()
    assert all((out[t][:, w[t] == 0] == 0).all() for t in range(ptheta))
    # with keep: the call on the kept subset, bit for bit, and the excluded positions may hold anything
    keep = np.random.default_rng(5).uniform(size=(ptheta, nscan)) > 0.3
    keep[:, :5] = True
    if ptheta == 2:
        keep[1] = keep[0]                                                                       # one subset size for both angles
    dirty = values.copy()
    dirty[~keep] = np.inf
    kw, kout = pt.scan_map(dev(dirty), dev(scan), dev(probe), nz, n, keep=dev(keep))
    sub = keep[0]
    sw, sout = pt.scan_map(dev(values[:, sub]), dev(scan[:, sub]), dev(probe), nz, n)
    assert same_bits(host(kw), host(sw)) and same_bits(host(kout), host(sout))
    assert same_bits(host(kout), ref.scan_map(values, scan, probe, nz, n, keep, weight=host(kw))[1])
    assert same_bits(host(pt.scan_map(dev(dirty), dev(scan), dev(probe), nz, n, keep=dev(keep), normalize=False)[1]),
                     ref.scan_map(values, scan, probe, nz, n, keep)[2])
    assert same_bits(host(pt.scan_map(dirty, scan, probe, nz, n, keep=keep.astype(np.uint8))[1]), host(kout))   # NumPy in
    again = pt.scan_map(dev(values), dev(scan), dev(probe), nz, n)
    assert same_bits(host(again[0]), w) and same_bits(host(again[1]), out)


def test_scan_map_constants_channels_and_shapes(pt):
    nz, n, nprb, nscan = 37, 70, 16, 130
    values, scan, probe = map_case(nz, n, nprb, 2, nscan, 4)
    values[..., 1] = -3.75
    values[0, 2] = np.nan
    w, out = pt.scan_map(dev(values), dev(scan), dev(probe), nz, n)
    w, out = host(w), host(out)
    lit = w[0] > 0
    assert np.abs(out[0, 1][lit] / -3.75 - 1).max() <= 1e-6 and (out[0, 1][~lit] == 0).all()
    for c in range(4):                                                    # a channel alone, and 2-D values: the same bits
        one = pt.scan_map(dev(values[..., c]), dev(scan), dev(probe), nz, n)
        assert one[1].shape == (1, nz, n) and same_bits(host(one[1]), out[:, c]) and same_bits(host(one[0]), w)
    six = np.concatenate([values, values[..., :2]], -1)                   # more than four channels: split over calls
    got = host(pt.scan_map(dev(six), dev(scan), dev(probe), nz, n)[1])
    assert got.shape == (1, 6, nz, n) and same_bits(got[:, :4], out) and same_bits(got[:, 4:], out[:, :2])
    three = host(pt.scan_map(dev(values[..., :3]), dev(scan), dev(probe[:, 0]), nz, n)[1])   # nval 3, a 3-D probe
    assert same_bits(three, ref.scan_map(values[..., :3], scan, probe[:, 0], nz, n,
                                         weight=host(pt.illumination(dev(scan), dev(probe[:, 0]), nz, n)))[1])


# ---- 3. integration ---------------------------------------------------------------------------------------------------------
def planted(shape, kind):
    y, x = np.meshgrid(np.arange(float(shape[0])), np.arange(float(shape[1])), indexing="ij")
    u, v = x / shape[1], y / shape[0]
    if kind == "plane":
        return 1.3 * u - 0.8 * v, np.full(shape, -0.8 / shape[0]), np.full(shape, 1.3 / shape[1])
    q, dq = 2.0 * u * u - 1.5 * u + 0.4, (4.0 * u - 1.5) / shape[1]       # a quadratic in x times a linear in y: the mean of
    lin, dl = 1.0 - 0.7 * v, -0.7 / shape[0]                             # the analytic gradient at the two ends of an edge
    return q * lin, q * dl, dq * lin                                      # is the difference along it exactly


def border_weight(shape, rng=None):
    w = np.zeros(shape, np.float32)
    w[2:-2, 3:-3] = 1.0 if rng is None else rng.uniform(0.2, 1.0, (shape[0] - 4, shape[1] - 6))
    return w


@pytest.mark.parametrize("shape", [(17, 130), (64, 64)])
@pytest.mark.parametrize("kind", ["plane", "quadratic"])
@pytest.mark.parametrize("weighted", [False, True])
def test_integrate_gradient_recovers_a_planted_surface(pt, shape, kind, weighted):
    s, gy, gx = planted(shape, kind)
    gy, gx = gy.astype(np.float32), gx.astype(np.float32)
    w = border_weight(shape, np.random.default_rng(3)) if weighted else None
    if weighted:                                                          # a zero-weight border holding NaN has no effect
        gy, gx = np.where(w > 0, gy, np.nan).astype(np.float32), np.where(w > 0, gx, np.nan).astype(np.float32)
    got = pt.integrate_gradient(dev(gy), dev(gx), None if w is None else dev(w), tol=1e-7)
    r64, r32 = ref.integrate(gy, gx, w, tol=1e-7), ref.integrate(gy, gx, w, tol=1e-7, dtype=np.float32)
    on = np.ones(shape, bool) if w is None else w > 0
    ww = np.ones(shape) if w is None else w.astype(np.float64)
    want = np.where(on, s - (ww * s)[on].sum() / ww[on].sum(), 0.0)
    out = host(got["phase"])
    e_dev, e32 = np.abs(out - want).max(), np.abs(r32["phase"] - want).max()
    d_dev, d32 = np.abs(out - r64["phase"]).max(), np.abs(r32["phase"] - r64["phase"]).max()
    print("integrate %s %s weighted %s: err %.2e (float32 restatement %.2e), from the float64 restatement %.2e (%.2e), "
          "%d iterations (%d, %d)" % (shape, kind, weighted, e_dev, e32, d_dev, d32, got["iterations"], r64["iterations"],
                                      r32["iterations"]))
    assert out.shape == shape and out.dtype == np.float32 and got["converged"] and got["status"] == 1
    assert set(got) == {"phase", "iterations", "residual", "converged", "status"}
    assert e_dev <= max(FACTOR * e32, 1e-6) and d_dev <= max(FACTOR * d32, 1e-6)
    assert abs(got["iterations"] - r32["iterations"]) <= 2 and (out[~on] == 0).all() and np.isfinite(out).all()
    if weighted:                                                          # other garbage outside: the same bits
        gy2, gx2 = np.where(w > 0, gy, 7.0).astype(np.float32), np.where(w > 0, gx, -np.inf).astype(np.float32)
        other = pt.integrate_gradient(dev(gy2), dev(gx2), dev(w), tol=1e-7)
        assert same_bits(host(other["phase"]), out) and other["iterations"] == got["iterations"]


def test_integrate_gradient_controls(pt):
    shape = (17, 130)
    s, gy, gx = planted(shape, "quadratic")
    gy, gx = np.stack([gy, -gy]).astype(np.float32), np.stack([gx, 2 * gx]).astype(np.float32)
    both = pt.integrate_gradient(dev(gy), dev(gx))
    assert both["phase"].shape == (2,) + shape and np.asarray(both["iterations"]).shape == (2,) and both["converged"].all()
    one = pt.integrate_gradient(dev(gy[1]), dev(gx[1]))                   # an angle alone: the same bits, no angle axis
    assert same_bits(host(one["phase"]), host(both["phase"])[1]) and one["iterations"] == both["iterations"][1]
    a = pt.integrate_gradient(dev(gy), dev(gx), maxiter=5, check_every=2)
    b = pt.integrate_gradient(gy, gx, maxiter=5)                          # NumPy arrays are copied to the device
    assert (a["iterations"] == 5).all() and (a["status"] == 3).all() and same_bits(host(a["phase"]), host(b["phase"]))
    r32 = ref.integrate(gy[0], gx[0], maxiter=5, dtype=np.float32)
    assert abs(a["residual"][0] - r32["residual"]) <= 1e-3 * r32["residual"]
    into = torch.full(shape, float("nan"), dtype=torch.float32, device="cuda")
    got = pt.integrate_gradient(dev(gy[0]), dev(gx[0]), out=into)
    assert got["phase"] is into and same_bits(host(into), host(both["phase"])[0])
    zero = pt.integrate_gradient(dev(gy[0]), dev(gx[0]), weight=dev(np.zeros(shape, np.float32)))
    assert (host(zero["phase"]) == 0).all() and zero["iterations"] == 0 and zero["converged"]
    m = border_weight(shape) > 0                                          # a bool mask is a weight of 0 / 1
    assert same_bits(host(pt.integrate_gradient(dev(gy[0]), dev(gx[0]), dev(m))["phase"]),
                     host(pt.integrate_gradient(dev(gy[0]), dev(gx[0]), dev(m.astype(np.float32)))["phase"]))


# ---- 4. end to end ----------------------------------------------------------------------------------------------------------
_memo = {}


def scenario(pt):
    """The scenario with data from the solver's own forward, the device's first look and the restatement's in float64 and
    float32, computed once and never changed."""
    if not _memo:
        sc = ref.scenario()
        with pt.CGPtychoSolver(sc["scan"].shape[1], sc["nprb"], sc["ndet"], 1, sc["nz"], sc["n"]) as slv:
            far = slv.fwd(dev(sc["psi"]), dev(sc["scan"]), dev(sc["probe"]))
            data = (torch.abs(far) ** 2).contiguous()
        args = (sc["scan"], sc["probe"], sc["nz"], sc["n"])
        _memo.update(sc=sc, data=data, look=pt.first_look(data, dev(sc["scan"]), dev(sc["probe"]), sc["nz"], sc["n"]),
                     r64=ref.first_look(host(data), *args), r32=ref.first_look(host(data), *args, dtype=np.float32))
    return _memo["sc"], _memo["data"], _memo["look"], _memo["r64"], _memo["r32"]


def test_first_look_equals_the_restatement(pt):
    sc, data, look, r64, r32 = scenario(pt)
    lit = r64["lit"]
    assert np.array_equal(host(look["lit"]), lit) and 0.5 < lit.mean() < 1 and look["converged"].all()
    assert np.abs(host(look["moments"]) - r64["moments"]).max() <= 1e-12 * np.abs(r64["moments"]).max()
    for key in ("transmission", "darkfield", "dpc_y", "dpc_x", "illumination", "phase"):
        got, want = host(look[key]), r64[key]
        e_dev, e32 = np.abs(got - want)[lit].max(), np.abs(r32[key] - want)[lit].max()
        print("first look %s: device err %.2e (float32 restatement %.2e)" % (key, e_dev, e32))
        assert got.shape == (1, sc["nz"], sc["n"]) and got.dtype == np.float32
        assert e_dev <= max(FACTOR * e32, 1e-5), key
    assert abs(int(look["iterations"][0]) - int(r32["iterations"][0])) <= 2
    assert (host(look["phase"])[~lit] == 0).all()
    again = pt.first_look(data, dev(sc["scan"]), dev(sc["probe"]), sc["nz"], sc["n"])
    assert all(same_bits(host(again[k]), host(look[k])) for k in ("phase", "transmission", "dpc_y", "dpc_x", "moments"))


def test_first_look_finds_the_object(pt):
    """The bound on the phase is for the probe's own centre as the reference, as measured in tests/test_dpc_cpu.py (0.043);
    the mean-frame reference removes a ramp, which is gauge, so there the ramp of the difference is taken out first."""
    sc, data, look, r64, _ = scenario(pt)
    ill = host(look["illumination"])[0]
    w = np.where(host(look["lit"])[0], ill, 0)
    # the documented recipe for the reference of a known probe
    with pt.CGPtychoSolver(1, sc["nprb"], sc["ndet"], 1, sc["nz"], sc["n"]) as slv:
        one = slv.fwd(torch.ones_like(dev(sc["psi"])), dev(np.array([[[8.0, 8.0]]], np.float32)), dev(sc["probe"]))
    c0 = host(pt.frame_moments((torch.abs(one) ** 2).contiguous())["center"])[0, 0]
    fixed = pt.first_look(data, dev(sc["scan"]), dev(sc["probe"]), sc["nz"], sc["n"], reference=tuple(c0))
    rms = ref.weighted_rms_error(host(fixed["phase"])[0], sc["phi"], w)
    rms_mean = ref.weighted_rms_error(host(look["phase"])[0], sc["phi"], w, ramp=True)
    acorr = ref.weighted_correlation(np.sqrt(np.maximum(host(look["transmission"])[0], 0)), sc["amp"], w)
    print("first look on the device: phase rms %.4f (probe reference %s), %.4f (mean reference, ramp removed), amplitude "
          "correlation %.5f, %d iterations, span %.2f rad" % (rms, c0, rms_mean, acorr, fixed["iterations"][0],
                                                              np.ptp(host(fixed["phase"])[0][w > 0])))
    assert rms <= 0.09 and rms_mean <= 0.09 and acorr >= 0.99 and np.ptp(host(fixed["phase"])[0][w > 0]) > 2 * np.pi
    psi0 = pt.initial_object(look)
    assert psi0.dtype == torch.complex64 and psi0.shape == (1, sc["nz"], sc["n"]) and psi0.is_contiguous()
    assert np.abs(host(psi0) - ref.initial_object({k: host(look[k]) for k in ("transmission", "phase", "lit")})).max() <= 1e-6
    assert (host(psi0)[~host(look["lit"])] == 1).all()
    flat = host(pt.initial_object(look, amplitude=False))
    assert np.abs(np.abs(flat) - 1).max() <= 1e-6


def test_reconstruction_starts_at_a_quarter_of_the_cost(pt):
    sc, data, look, _, _ = scenario(pt)
    costs = {}
    for name, psi0 in (("ones", torch.ones_like(dev(sc["psi"]))), ("first look", pt.initial_object(look))):
        with pt.CGPtychoSolver(sc["scan"].shape[1], sc["nprb"], sc["ndet"], 1, sc["nz"], sc["n"]) as slv:
            slv.verbose = False
            slv.run(data, psi0.clone(), dev(sc["scan"]).clone(), dev(sc["probe"])[:, None].clone(), piter=1)
            costs[name] = slv.history[0][3]
    print("first logged cost: %.1f from psi = 1, %.1f from initial_object (ratio %.4f)"
          % (costs["ones"], costs["first look"], costs["first look"] / costs["ones"]))
    assert costs["first look"] <= 0.25 * costs["ones"]


# ---- 5. argument errors -----------------------------------------------------------------------------------------------------
def test_argument_errors_on_the_device(pt):
    sc = ref.scenario()
    data = torch.zeros((1, 4, 8, 8), dtype=torch.float32, device="cuda")
    scan, probe = dev(sc["scan"][:, :4]), dev(sc["probe"])
    with pytest.raises(ValueError, match="device tensors or NumPy arrays"):
        pt.frame_moments(torch.zeros((1, 4, 8, 8)))
    with pytest.raises(ValueError, match="mask must be"):
        pt.frame_moments(data, mask=torch.ones((8, 7), device="cuda"))
    with pytest.raises(ValueError, match="darkfield"):
        pt.frame_moments(data, darkfield=-2)
    with pytest.raises(ValueError, match="values must be"):
        pt.scan_map(torch.zeros((1, 5), device="cuda"), scan, probe, 96, 112)
    with pytest.raises(ValueError, match="keep must be"):
        pt.scan_map(torch.zeros((1, 4), device="cuda"), scan, probe, 96, 112, keep=torch.ones((1, 3), dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="gx must have"):
        pt.integrate_gradient(torch.zeros((8, 8), device="cuda"), torch.zeros((8, 9), device="cuda"))
    with pytest.raises(ValueError, match="contiguous"):
        pt.integrate_gradient(torch.zeros((8, 9), device="cuda"), torch.zeros((8, 9), device="cuda"),
                              out=torch.zeros((9, 8), device="cuda").T)
    with pytest.raises(ValueError, match="reference must be"):
        pt.first_look(data, scan, probe, 96, 112, reference="median")
    with pytest.raises(ValueError, match="differ|values must be"):
        pt.first_look(data, dev(sc["scan"][:, :5]), probe, 96, 112)
    # every frame empty: nothing lit, an object of ones
    look = pt.first_look(data, scan, probe, 96, 112)
    assert not host(look["lit"]).any() and (host(pt.initial_object(look)) == 1).all()
