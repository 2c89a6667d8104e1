"""Phase unwrapping on the device (``libtike.hipfft.unwrap``, csrc/k_unwrap.hpp) against the NumPy restatement of
tests/unwrap_ref.py: clean and weighted phases recovered up to one integer per angle, garbage outside the support without
effect, residues, disconnected regions, the controls of the iteration, and the chain ``fix_gauge`` -> ``unwrap_phase``.

Tolerances.  A congruent result is ``phi + 2 pi k`` formed in float64 and rounded once, and ``phi`` is within
``2^-24 pi`` of ``W(truth)``: it may sit one float32 spacing of its largest value from ``truth + 2 pi m``, no more.
The least-squares result ``x`` follows the scheme of tests/test_hip_gauge.py: the device may be ``FACTOR`` times the
float32 restatement's own distance ``d32`` from the float64 one off (after removal of the mean: the solution is defined up
to a constant), with a floor and never more than a cap.  ``x`` reaches about 60 rad, where one float32 spacing is ``2^-18
= 3.8e-6``, and every iteration rounds ``x += alpha p`` once: ``FLOOR = 3e-5`` is eight such spacings (fused multiply-adds
on the device round differently from the restatement's separate multiply and add), ``CAP = 1e-3`` is what 500 iterations
lose if each one loses half a spacing in the same direction -- the cases here stop after 330 to 370 iterations.
profiles/r10/unwrap.txt records, case by case, the device's observed error beside ``d32``.
Observed on an MI355X (case 3): device 3.1e-5 rad against d32 3.2e-5 rad, 362 iterations in all three.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import unwrap_ref as ref  # noqa: E402
from hip_common import bound, dev, host, pt  # noqa: E402, F401

pytestmark = pytest.mark.gpu

FLOOR, CAP = 3e-5, 1e-3
TWO_PI = 2.0 * np.pi
SHAPE = (67, 129)


def centred(a, m=None):
    a = a.astype(np.float64)
    return a - (a.mean() if m is None else a[m].mean())


def ellipse():
    y, x = np.meshgrid(np.arange(SHAPE[0]), np.arange(SHAPE[1]), indexing="ij")
    return (((y - 33) / 30.0) ** 2 + ((x - 64) / 60.0) ** 2 < 1).astype(np.float32)


_memo = {}


def noisy():
    """Case 3's input with its float64 and float32 restatements, computed once and never changed."""
    if "noisy" not in _memo:
        truth = ref.make_truth(*SHAPE, 25)
        phi = ref.wrap(truth + np.random.default_rng(11).normal(0, 0.6, truth.shape)).astype(np.float32)
        _memo["noisy"] = (truth, phi, ref.unwrap(phi, tol=1e-6, congruent=False),
                          ref.unwrap(phi, tol=1e-6, congruent=False, dtype=np.float32))
    return _memo["noisy"]


def one_integer(out, truth, m=None):
    """``(out - truth) / 2 pi`` on ``m``: the integer (all the same) and the largest deviation from it in radians."""
    k = (out.astype(np.float64) - truth) / TWO_PI
    k = k if m is None else k[m]
    assert np.ptp(np.rint(k)) == 0, (np.rint(k).min(), np.rint(k).max())
    return int(np.rint(k.flat[0])), float(np.abs(k - np.rint(k)).max() * TWO_PI)


# ---- 1. clean, unweighted ---------------------------------------------------------------------------------------------------
def test_clean_phase_three_angles(pt):
    truth = np.stack([ref.make_truth(*SHAPE, amp) for amp in (25.0, 12.0, -18.0)])
    phi = ref.wrap(truth).astype(np.float32)
    got = pt.unwrap_phase(dev(phi))
    out = host(got["phase"])
    assert out.shape == phi.shape and out.dtype == np.float32 and got["phase"].is_cuda
    for t in range(3):
        r32 = ref.unwrap(phi[t], dtype=np.float32)
        _, err = one_integer(out[t], truth[t])
        print("unwrap clean angle %d: %d iterations (float32 restatement %d), deviation %.2e rad, residual %.2e"
              % (t, got["iterations"][t], r32["iterations"], err, got["residual"][t]))
        assert err <= np.spacing(np.float32(np.abs(out[t]).max()))
        assert got["converged"][t] and got["status"][t] == 1 and got["residues"][t] == 0
        assert abs(int(got["iterations"][t]) - r32["iterations"]) <= 2
        assert got["residual"][t] <= 1e-4
    for key in ("iterations", "residual", "converged", "status", "offset", "residues"):
        assert np.asarray(got[key]).shape == (3,)
    single = pt.unwrap_phase(dev(phi[1]))                              # one angle alone: the same bits, no angle axis
    assert single["phase"].shape == SHAPE and np.array_equal(host(single["phase"]), out[1])
    assert single["iterations"] == got["iterations"][1] and isinstance(single["converged"], bool)


@pytest.mark.parametrize("shape, amp", [((65, 257), 20.0), ((17, 65), 6.0), ((2, 2), 1.0), ((2, 300), 1.0), ((300, 2), 1.0),
                                        ((64, 128), 20.0)])
def test_clean_phase_other_shapes(pt, shape, amp):
    truth = ref.make_truth(*shape, amp)
    assert max(np.abs(np.diff(truth, axis=0)).max(), np.abs(np.diff(truth, axis=1)).max()) < 2.0
    phi = ref.wrap(truth).astype(np.float32)
    got = pt.unwrap_phase(phi)                                         # a NumPy array is copied to the device
    r32 = ref.unwrap(phi, dtype=np.float32)
    out = host(got["phase"])
    _, err = one_integer(out, truth)
    print("unwrap clean %dx%d: %d iterations (float32 restatement %d), deviation %.2e rad"
          % (shape + (got["iterations"], r32["iterations"], err)))
    assert err <= np.spacing(np.float32(np.abs(out).max()))
    assert got["converged"] and got["residues"] == 0 and abs(got["iterations"] - r32["iterations"]) <= 2


# ---- 2. weighted support ----------------------------------------------------------------------------------------------------
def test_weighted_support_ignores_what_lies_outside(pt):
    truth = ref.make_truth(*SHAPE, 25)
    w = ellipse()
    m = w > 0
    rng = np.random.default_rng(2)
    a = np.where(m, ref.wrap(truth), rng.uniform(-np.pi, np.pi, truth.shape)).astype(np.float32)
    b = np.where(m, ref.wrap(truth), rng.uniform(-np.pi, np.pi, truth.shape)).astype(np.float32)
    off = np.flatnonzero(~m.ravel())
    off = off[::len(off) // 20][:20]
    b.ravel()[off[::2]], b.ravel()[off[1::2]] = np.nan, np.inf
    assert np.isnan(b).sum() == 10 and np.isinf(b).sum() == 10 and not np.array_equal(a[~m], b[~m])
    ga, gb = pt.unwrap_phase(dev(a), weight=dev(w)), pt.unwrap_phase(dev(b), weight=dev(w))
    oa, ob = host(ga["phase"]), host(gb["phase"])
    D = ref.unwrap(a, w)["D"]
    assert (D > 0)[m].all() and not (D > 0)[~m].any()
    _, err = one_integer(oa, truth, m)
    print("unwrap ellipse: %d iterations, deviation %.2e rad inside" % (ga["iterations"], err))
    assert err <= np.spacing(np.float32(np.abs(oa[m]).max())) and ga["converged"] and ga["residues"] == 0
    assert np.array_equal(oa[m], ob[m])                                 # garbage outside: the same bits inside
    assert ga["iterations"] == gb["iterations"] and ga["residual"] == gb["residual"] and ga["offset"] == gb["offset"]
    assert np.array_equal(oa[~m], a[~m]) and np.array_equal(ob[~m], b[~m], equal_nan=True)   # D = 0: out == phi
    assert np.isfinite(ob[np.isfinite(b)]).all()
    w2 = w.copy()
    w2[~m] = np.resize(np.array([-1.0, np.nan, -np.inf, 0.0], np.float32), (~m).sum())   # these count as 0
    gc = pt.unwrap_phase(dev(b), weight=dev(w2))
    assert np.array_equal(host(gc["phase"]), ob, equal_nan=True) and gc["iterations"] == gb["iterations"]
    gd = pt.unwrap_phase(dev(b), weight=dev(m))                         # a bool mask is a weight of 0 / 1
    assert np.array_equal(host(gd["phase"]), ob, equal_nan=True)


# ---- 3. residues inside -----------------------------------------------------------------------------------------------------
def test_least_squares_solution_with_residues(pt):
    truth, phi, r64, r32 = noisy()
    got = pt.unwrap_phase(dev(phi), tol=1e-6, congruent=False)
    e_dev = np.abs(centred(host(got["phase"])) - centred(r64["phase"])).max()
    d32 = np.abs(centred(r32["phase"]) - centred(r64["phase"])).max()
    print("unwrap noisy least squares: device err %.2e rad (float32 restatement %.2e), %d iterations (%d, %d), %d residues"
          % (e_dev, d32, got["iterations"], r64["iterations"], r32["iterations"], got["residues"]))
    assert e_dev <= bound(d32, FLOOR, CAP), (e_dev, d32)
    assert got["converged"] and got["residues"] == r64["residues"] > 0


def test_congruent_integers_with_residues(pt):
    truth, phi, r64, _ = noisy()
    got = pt.unwrap_phase(dev(phi), tol=1e-6)
    k = np.rint((host(got["phase"]).astype(np.float64) - phi) / TWO_PI)
    near = np.abs(r64["k"] - np.floor(r64["k"]) - 0.5) < 0.01
    print("unwrap noisy congruent: %.2f %% of the pixels near a half-integer, %d integers differ outside them"
          % (100 * near.mean(), (k != np.rint(r64["k"]))[~near].sum()))
    assert near.mean() <= 0.02
    assert np.array_equal(k[~near], np.rint(r64["k"])[~near])
    assert np.abs(host(got["phase"]) - (phi + TWO_PI * k)).max() <= np.spacing(np.float32(np.abs(host(got["phase"])).max()))


# ---- 4. two regions ---------------------------------------------------------------------------------------------------------
def test_two_regions_each_up_to_its_own_constant(pt):
    truth = ref.make_truth(*SHAPE, 25)
    w = np.ones(SHAPE, np.float32)
    w[:, 60:63] = 0
    phi = np.where(w > 0, ref.wrap(truth), np.random.default_rng(4).uniform(-np.pi, np.pi, SHAPE)).astype(np.float32)
    got = pt.unwrap_phase(dev(phi), weight=dev(w), congruent=False, tol=1e-6)
    r64 = ref.unwrap(phi, w, congruent=False, tol=1e-6)
    r32 = ref.unwrap(phi, w, congruent=False, tol=1e-6, dtype=np.float32)
    out = host(got["phase"]).astype(np.float64)
    assert np.array_equal(host(got["phase"])[:, 60:63], phi[:, 60:63])
    for cols in (slice(0, 60), slice(63, None)):
        spread = np.ptp(out[:, cols] - truth[:, cols])
        d32 = np.ptp(r32["phase"].astype(np.float64)[:, cols] - truth[:, cols])
        d64 = np.ptp(r64["phase"].astype(np.float64)[:, cols] - truth[:, cols])
        print("unwrap two regions, columns %s: spread %.2e rad (float32 restatement %.2e, float64 %.2e)" % (cols, spread, d32, d64))
        assert spread <= bound(d32, FLOOR, CAP), (spread, d32)


# ---- 5. vortex pair ---------------------------------------------------------------------------------------------------------
def test_vortex_pair_charges(pt):
    y, x = np.meshgrid(np.arange(float(SHAPE[0])), np.arange(float(SHAPE[1])), indexing="ij")
    phi = (np.arctan2(y - 20.5, x - 40.5) - np.arctan2(y - 45.5, x - 90.5)).astype(np.float32)
    ch = host(pt.phase_residues(dev(phi)))
    assert ch.dtype == np.int8 and ch.shape == (SHAPE[0] - 1, SHAPE[1] - 1)
    assert ch[20, 40] == 1 and ch[45, 90] == -1 and np.abs(ch).sum() == 2
    assert np.array_equal(ch, ref.residues(phi, dtype=np.float32)[0])
    assert pt.unwrap_phase(dev(phi), maxiter=0)["residues"] == 2
    w = np.ones(SHAPE, np.float32)
    w[43:48, 88:93] = 0
    ch = host(pt.phase_residues(dev(phi), dev(w)))
    assert ch[45, 90] == 0 and ch[20, 40] == 1 and np.abs(ch).sum() == 1
    assert np.array_equal(ch, ref.residues(phi, w, dtype=np.float32)[0])
    assert pt.unwrap_phase(dev(phi), weight=dev(w), maxiter=0)["residues"] == 1
    both = host(pt.phase_residues(dev(np.stack([phi, -phi])), dev(np.stack([w, np.ones_like(w)]))))   # angles apart
    assert np.array_equal(both[0], ch) and both[1][20, 40] == -1 and both[1][45, 90] == 1 and np.abs(both[1]).sum() == 2


# ---- 6. controls ------------------------------------------------------------------------------------------------------------
def test_maxiter_and_check_every(pt):
    truth, phi, _, _ = noisy()
    a = pt.unwrap_phase(dev(phi), maxiter=5, check_every=256)
    b = pt.unwrap_phase(dev(phi), maxiter=5, check_every=2)
    for g in (a, b):
        assert g["iterations"] == 5 and g["status"] == 3 and g["converged"] is False
    assert np.array_equal(host(a["phase"]), host(b["phase"])) and a["residual"] == b["residual"] and a["offset"] == b["offset"]
    r32 = ref.unwrap(phi, maxiter=5, dtype=np.float32)
    assert abs(a["residual"] - r32["residual"]) <= 1e-3 * r32["residual"]
    its = [pt.unwrap_phase(dev(phi), tol=tol)["iterations"] for tol in (1e-2, 1e-3, 1e-4, 1e-5)]
    assert its == sorted(its) and its[0] < its[-1]
    c = pt.unwrap_phase(dev(phi), check_every=7)                        # blocks that do not divide the count
    d = pt.unwrap_phase(dev(phi))
    assert c["iterations"] == d["iterations"] and np.array_equal(host(c["phase"]), host(d["phase"]))


def test_nothing_to_do(pt):
    truth, phi, _, _ = noisy()
    got = pt.unwrap_phase(dev(phi), weight=dev(np.zeros(SHAPE, np.float32)))
    assert np.array_equal(host(got["phase"]), phi) and got["iterations"] == 0 and got["converged"] and got["offset"] == 0.0
    assert np.isfinite(got["residual"]) and got["residues"] == 0
    flat = np.full((33, 70), 0.75, np.float32)
    got = pt.unwrap_phase(dev(flat))
    assert np.array_equal(host(got["phase"]), flat) and got["iterations"] == 0 and got["converged"]


def test_complex_input_repeats_and_out(pt):
    truth, phi, _, _ = noisy()
    psi = dev((0.7 * np.exp(1j * truth)).astype(np.complex64))
    a, b = pt.unwrap_phase(psi), pt.unwrap_phase(torch.angle(psi))
    assert np.array_equal(host(a["phase"]), host(b["phase"])) and a["iterations"] == b["iterations"]
    again = pt.unwrap_phase(psi)
    assert np.array_equal(host(a["phase"]), host(again["phase"])) and a["residual"] == again["residual"]
    into = torch.full(SHAPE, float("nan"), dtype=torch.float32, device="cuda")
    got = pt.unwrap_phase(psi, out=into)
    assert got["phase"] is into and np.array_equal(host(into), host(a["phase"]))
    one_integer(host(into), truth)
    with pytest.raises(ValueError, match="contiguous"):
        pt.unwrap_phase(psi, out=torch.zeros((SHAPE[1], SHAPE[0]), dtype=torch.float32, device="cuda").T)


# ---- 7. with the gauge ------------------------------------------------------------------------------------------------------
def test_fix_gauge_then_unwrap(pt):
    nz, n, nprb = 96, 160, 16
    truth = ref.make_truth(nz, n, 20.0)
    y, x = np.meshgrid(np.arange(nz, dtype=np.float64), np.arange(n, dtype=np.float64), indexing="ij")
    amp = 0.8 + 0.1 * np.cos(0.07 * x + 0.05 * y)
    psi = (amp * np.exp(1j * (truth + 0.31 * y - 0.17 * x))).astype(np.complex64)[None]     # the planted ramp
    py, px = np.meshgrid(np.arange(2.0, nz - nprb - 2, 6.0), np.arange(2.0, n - nprb - 2, 6.0), indexing="ij")
    scan = np.stack([py.ravel(), px.ravel()], -1).astype(np.float32)[None]
    g = np.exp(-((np.arange(nprb) - 7.5) ** 2) / 18.0)
    probe = (g[:, None] * g[None, :]).astype(np.complex64)[None, None]
    fa = pt.fix_gauge(dev(psi), dev(scan), dev(probe))
    got = pt.unwrap_phase(fa["psi"], weight=fa["lit"], tol=1e-6)
    lit = host(fa["lit"])[0]
    gauge = host(fa["gauge"])[0]
    assert lit.mean() > 0.5 and got["converged"][0] and got["residues"][0] == 0
    # what fix_gauge left: the planted phase minus the ramp and the offset that it fitted
    want = truth + 0.31 * y - 0.17 * x - (gauge[2] + gauge[0] * (y - gauge[4]) + gauge[1] * (x - gauge[5]))
    out = host(got["phase"])[0].astype(np.float64)
    k = (out - want)[lit] / TWO_PI
    r64 = ref.unwrap(host(torch.angle(fa["psi"]))[0], lit.astype(np.float32), tol=1e-6, congruent=False)
    r32 = ref.unwrap(host(torch.angle(fa["psi"]))[0], lit.astype(np.float32), tol=1e-6, congruent=False, dtype=np.float32)
    d32 = np.abs(centred(r32["phase"], lit) - centred(r64["phase"], lit))[lit].max()
    err = np.abs(k - np.rint(k)).max() * TWO_PI
    print("unwrap after fix_gauge: %d iterations, distance from the planted phase %.2e rad (bound %.2e), span %.1f rad"
          % (got["iterations"][0], err, bound(d32, FLOOR, CAP), np.ptp(out[lit])))
    assert np.ptp(np.rint(k)) == 0 and np.ptp(out[lit]) > TWO_PI
    assert err <= bound(d32, FLOOR, CAP), (err, d32)
