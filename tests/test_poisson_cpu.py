"""Poisson maximum-likelihood model of the CG reconstruction, host side: the NumPy reference of tests/cg_reference.py held
to calculus, its mask rules, the models it keeps as they are, and the C ABI's model key.  No GPU needed."""
import os
import sys
import warnings

import numpy as np
import pytest

from libtike.hipfft import synthetic as syn
from oracle import cg_oracle as cg
from oracle import ptycho_oracle as op

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cg_reference import ReferenceSolver, detector_mask, poisson_cost, poisson_residual  # noqa: E402


def problem(nmodes, ndet=16, seed=3, dose=20.0):
    """test_mask_cpu.py's problem with Poisson-sampled data (``dose`` photons at the brightest pixel)."""
    p = syn.make_problem(4, 4, 4, ndet, ndet, seed=seed)
    probe = syn.hermite_modes(ndet, nmodes) if nmodes > 1 else p["probe"][:, None].copy()
    rng = np.random.default_rng(seed + 100)
    probe = (probe * np.exp(2j * np.pi * rng.random(probe.shape[-2:]))).astype(np.complex64)
    ora = cg.OracleSolver(p["nscan"], ndet, ndet, 1, p["nz"], p["n"])
    inten = np.zeros((1, p["nscan"], ndet, ndet), np.float32)
    for k in range(nmodes):
        inten += np.abs(ora.fwd(p["psi"], p["scan"], probe[:, k])) ** 2
    data = rng.poisson(inten * (dose / inten.max())).astype(np.float32)
    return p, probe, data


def run(p, probe, data, model="poisson_ml", mask=None, piter=5, recover=True, precision="single"):
    ndet = data.shape[-1]
    slv = ReferenceSolver(p["nscan"], ndet, ndet, 1, p["nz"], p["n"], precision=precision)
    scan = p["scan"].copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = slv.run(data.copy(), np.ones_like(p["psi"]), scan, probe.copy().swapaxes(2, 3),
                      piter=piter, model=model, recover_prb=recover, mask=mask)
    return res, scan, slv.history


def test_the_residual_is_the_gradient():
    """d/dt f(|G(psi + t delta)|^2) at t = 0 is 2 Re <G*(G psi (1 - d / |G psi|^2)), delta>, with G = fwd(., probe) and
    G* = adj(., probe) (float64 oracle operators, probe scale 1): the residual that the object gradient back-projects."""
    ndet = 16
    p, probe, data = problem(1, ndet=ndet, dose=30.0)
    data = data.astype(np.float64)
    rng = np.random.default_rng(9)
    shape = p["psi"].shape
    psi = (p["psi"] * np.exp(0.3j * rng.standard_normal(shape))).astype(np.complex128)
    delta = rng.standard_normal(shape) + 1j * rng.standard_normal(shape)
    prb = probe[:, 0].astype(np.complex128)
    G = lambda x: op.fwd(x, p["scan"], prb, ndet, "double")  # noqa: E731
    Gs = lambda y: op.adj(y, p["scan"], prb, p["nz"], p["n"], "double")  # noqa: E731
    # premise: G* is the adjoint of G
    y = rng.standard_normal(data.shape) + 1j * rng.standard_normal(data.shape)
    lhs, rhs = np.vdot(G(delta), y), np.vdot(delta, Gs(y))
    assert abs(lhs - rhs) <= 1e-10 * abs(lhs)

    def f(x):
        return poisson_cost(np.abs(G(x)) ** 2, data)

    fp = G(psi)
    r = poisson_residual(fp, np.abs(fp) ** 2, data)
    assert np.abs(r).max() > 0.1 * np.abs(fp).max()      # far from the optimum: the check is not 0 = 0
    want = 2.0 * np.vdot(Gs(r), delta).real
    t = 1e-6
    got = (f(psi + t * delta) - f(psi - t * delta)) / (2.0 * t)
    assert abs(got - want) <= 1e-6 * abs(want), (got, want)
    # and the gaussian residual is not that gradient (the check tells the two models apart)
    rg = fp - np.sqrt(data) * fp / (np.abs(fp) + 1e-32)
    assert abs(2.0 * np.vdot(Gs(rg), delta).real - want) > 1e-3 * abs(want)


@pytest.mark.parametrize("nmodes", [1, 2])
def test_all_ones_mask_is_no_mask_bitwise(nmodes):
    p, probe, data = problem(nmodes)
    want, wscan, whist = run(p, probe, data)
    got, gscan, ghist = run(p, probe, data, mask=np.ones(data.shape[-2:], np.float32))
    assert np.array_equal(got["psi"], want["psi"])
    assert np.array_equal(got["probe"], want["probe"])
    assert np.array_equal(gscan, wscan)
    assert ghist == whist


@pytest.mark.parametrize("garbage", [np.nan, -1.0, 1e30])
def test_unmeasured_data_is_ignored(garbage):
    p, probe, data = problem(1)
    mask = detector_mask(data.shape[-1], beamstop=2, gap=1, dead=0.05, seed=4)
    assert 0 < (mask == 0).sum() < mask.size
    zero = np.where(mask != 0, data, 0).astype(np.float32)
    bad = np.where(mask != 0, data, garbage).astype(np.float32)
    want, wscan, whist = run(p, probe, zero, mask=mask)
    got, gscan, ghist = run(p, probe, bad, mask=mask)
    assert np.isfinite(got["psi"]).all() and np.isfinite(got["probe"]).all()
    assert np.array_equal(got["psi"], want["psi"])
    assert np.array_equal(got["probe"], want["probe"])
    assert np.array_equal(gscan, wscan)
    assert ghist == whist


def test_masked_terms_are_zero():
    """At an unmeasured pixel d and I are selected to 0, so its cost term 0 - 0 ln(1e-32) is exactly 0."""
    d = np.array([0.0, 3.0], np.float32)
    x = np.array([0.0, 2.0], np.float32)
    assert poisson_cost(x[:1], d[:1]) == 0.0
    assert poisson_cost(x, d) == poisson_cost(x[1:], d[1:])


def test_poisson_still_raises_and_poisson_ml_runs():
    p, probe, data = problem(1)
    with pytest.raises(UnboundLocalError):
        run(p, probe, data, model="poisson")
    with pytest.raises(UnboundLocalError):
        cg.OracleSolver(p["nscan"], 16, 16, 1, p["nz"], p["n"]).run(
            data.copy(), np.ones_like(p["psi"]), p["scan"].copy(), probe.copy(), piter=1, model="poisson")
    res, scan, hist = run(p, probe, data, piter=4)
    assert len(hist) == 4 and all(np.isfinite(h[3]) for h in hist)
    assert np.isfinite(res["psi"]).all() and np.isfinite(res["probe"]).all()
    # the logged cost is the Poisson one of the start-of-iteration intensity (after the probe rescale)
    ora = cg.OracleSolver(p["nscan"], 16, 16, 1, p["nz"], p["n"])
    inten = np.abs(ora.fwd(np.ones_like(p["psi"]), p["scan"], probe[:, 0].swapaxes(1, 2).copy())) ** 2
    ab = np.sum(np.sqrt(inten * data)) / np.sum(inten)
    want = float(poisson_cost(inten * ab ** 2, data))
    assert abs(hist[0][3] - want) <= 1e-5 * abs(want), (hist[0][3], want)
    # poisson_ml and gaussian take different steps from the same start
    assert [h[1:3] for h in hist] != [h[1:3] for h in run(p, probe, data, model="gaussian", piter=4)[2]]


def test_gaussian_reference_is_untouched():
    """With model="gaussian" the reference is the oracle itself, bit for bit: one and several modes, with and without
    probe recovery."""
    for nmodes, recover in [(2, True), (1, True), (3, True), (1, False), (3, False)]:
        p, probe, data = problem(nmodes)
        got, gscan, ghist = run(p, probe, data, model="gaussian", recover=recover)
        ora = cg.OracleSolver(p["nscan"], 16, 16, 1, p["nz"], p["n"])
        scan = p["scan"].copy()
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            want = ora.run(data.copy(), np.ones_like(p["psi"]), scan, probe.copy().swapaxes(2, 3), piter=5,
                           recover_prb=recover)
        assert np.array_equal(got["psi"], want["psi"]) and np.array_equal(got["probe"], want["probe"]), (nmodes, recover)
        assert np.array_equal(gscan, scan) and ghist == ora.history, (nmodes, recover)


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build_native()
    from libtike.hipfft import _native
    return _native


def test_model_key_without_gpu(nat):
    assert nat.GET_MODEL == 103
    assert (nat.MODEL_GAUSSIAN, nat.MODEL_POISSON_ML) == (0, 1)
    assert nat.get(None, nat.GET_MODEL) == -1
    assert nat.set_option(None, b"model", nat.MODEL_POISSON_ML) == 1
    assert b"null handle" in nat.last_error()


def test_run_documents_poisson_ml():
    import libtike.hipfft as pt
    doc = pt.CGPtychoSolver.run.__doc__
    assert '"poisson_ml"' in doc and "UnboundLocalError" in doc
