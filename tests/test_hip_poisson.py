"""Poisson maximum-likelihood model of the CG reconstruction on the GPU: ``CGPtychoSolver.run(..., model="poisson_ml")``
on every loop (native, host-driven fused, multi-mode, statement-by-statement torch), against the float64 NumPy reference
of tests/cg_reference.py, with and without the detector mask."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_harness as cg  # noqa: E402
from cg_harness import (assert_ranks_match, check_run_batch_partitions, intensity, reference, same_run,  # noqa: E402
                        solver, two_rank_run)
from cg_reference import detector_mask  # noqa: E402
from hip_common import pt  # noqa: E402, F401
import recon_metrics as rm  # noqa: E402
from libtike.hipfft import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu

#: Poisson-sampled data unless a test says otherwise: 20 photons expected at the brightest pixel
problem = functools.partial(cg.problem, dose=20.0)
gpu_run = functools.partial(cg.gpu_run, model="poisson_ml")


def track(pt, p, start, data, recover, path, **kw):
    """cg_harness.track on the Poisson model; the positions follow the reference to 1e-2 pixels."""
    return cg.track(pt, p, start, data, recover, path, model="poisson_ml", scan_tol=1e-2, **kw)


# (name, ndet, nmodes, recover, solver path, dose): the native single-mode loop at 256^2 with and without probe
# recovery, the host-driven fused loop, the multi-mode loop with 2 and 4 modes, the torch loop with fused=False and on
# a size without a Stockham plan (Bluestein operators)
TRACK = [("native256_prb", 256, 1, True, "default", 20.0), ("native256", 256, 1, False, "default", 20.0),
         ("fused64", 64, 1, True, "fused", 20.0), ("modes2_128", 128, 2, True, "default", 1000.0),
         ("modes4_512", 512, 4, True, "default", 1000.0), ("torch64", 64, 1, True, "torch", 20.0),
         ("torch100", 100, 1, True, "torch", 20.0)]


@pytest.mark.parametrize("name,ndet,nmodes,recover,path,dose", TRACK, ids=[c[0] for c in TRACK])
def test_poisson_cg_tracks_the_float64_reference(pt, name, ndet, nmodes, recover, path, dose):
    small = ndet == 512
    p, probe, data = problem(ndet, nmodes, dose=dose, ny=4 if small else 6, step=24 if small else 6)
    start = probe.swapaxes(2, 3).copy() if recover else probe.copy()
    # Bluestein operators (ndet 100): ~1e-6 of the largest farplane value is absolute error, which ln and d / I amplify at
    # dim pixels
    track(pt, p, start, data, recover, path, cost_rtol=5e-4 if ndet == 100 else 1e-5, tol=2e-3 if ndet == 100 else 5e-4)


@pytest.mark.parametrize("path", ["default", "fused", "modes", "torch"])
def test_gradient_vanishes_at_the_truth(pt, path):
    """With d = |G psi_true|^2 and the true object and probe, a / b = 1 and the Poisson residual fp (1 - d / |fp|^2) is ~0:
    one iteration with probe recovery stays at the truth."""
    ndet = 64
    p, probe, data = problem(ndet, 2 if path == "modes" else 1, dose=None)
    truth = p["psi"].astype(np.complex64)
    with solver(pt, p, ndet, "default" if path == "modes" else path) as slv:
        psi, prb = gpu_run(slv, p, probe, data, piter=1, recover=True, psi=truth)[:2]
    assert np.abs(psi - truth).max() < 1e-4 * np.abs(truth).max(), np.abs(psi - truth).max()
    assert np.abs(prb - probe).max() < 1e-4 * np.abs(probe).max(), np.abs(prb - probe).max()
    # and the same start with gaussian-consistent but Poisson-sampled data moves (the check is not vacuous)
    with solver(pt, p, ndet, "default" if path == "modes" else path) as slv:
        noisy = np.random.default_rng(1).poisson(data * (20.0 / data.max())).astype(np.float32) * (data.max() / 20.0)
        psi2 = gpu_run(slv, p, probe, noisy.astype(np.float32), piter=1, recover=False, psi=truth)[0]
    assert np.abs(psi2 - truth).max() > 1e-3 * np.abs(truth).max()


def test_deterministic_adjoint_with_dark_pixels(pt):
    """Counts where the model intensity is ~0 (1e-8 .. 1e-5 of its maximum): the residual d fp / I there is ~1e3 times
    the others, so the fixed point of the deterministic adjoint is sized by these pixels.  It agrees with the float-atomic
    adjoint and with the float64 reference, and nothing is NaN or Inf."""
    ndet = 64
    p = syn.make_problem(6, 6, 6, ndet, ndet, seed=13)
    probe = p["probe"][:, None].copy()          # smooth probe, no phase screen: its far field falls off to ~0
    inten = intensity(p, probe)
    rel = inten / inten.max()
    dark = (rel > 1e-8) & (rel < 1e-5)
    assert dark.sum() > 100
    data = np.random.default_rng(3).poisson(inten * (50.0 / inten.max())).astype(np.float32)
    data[dark] = 2.0
    truth = p["psi"].astype(np.complex64)
    runs = {}
    for det in (True, False):
        with solver(pt, p, ndet, "default") as slv:
            slv.reproducible = det
            runs[det] = gpu_run(slv, p, probe, data, piter=2, recover=True, psi=truth)
    want = reference(p, probe, data, 2, "double", psi=truth, model="poisson_ml")
    for got in runs.values():
        assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
        assert [h[1:3] for h in got[3]] == [h[1:3] for h in want[3]], (got[3], want[3])
        for k in (0, 1):
            d = np.abs(got[k] - want[k]).max() / np.abs(want[k]).max()
            assert d < 1e-3, (k, d)
    for k in (0, 1):
        d = np.abs(runs[True][k] - runs[False][k]).max() / np.abs(runs[False][k]).max()
        assert d < 1e-4, (k, d)


PATHS = [("native64", 64, 1, "default"), ("native256", 256, 1, "default"), ("fused64", 64, 1, "fused"),
         ("modes64", 64, 3, "default"), ("torch64", 64, 1, "torch"), ("torch100", 100, 1, "torch")]


@pytest.mark.parametrize("name,ndet,nmodes,path", PATHS, ids=[q[0] for q in PATHS])
def test_all_ones_mask_is_no_mask_bitwise(pt, name, ndet, nmodes, path):
    p, probe, data = problem(ndet, nmodes)
    start = probe.swapaxes(2, 3).copy()
    with solver(pt, p, ndet, path) as slv:
        want = gpu_run(slv, p, start, data)
    with solver(pt, p, ndet, path) as slv:
        got = gpu_run(slv, p, start, data, mask=np.ones((ndet, ndet), bool))
    same_run(got, want)


@pytest.mark.parametrize("garbage", [np.nan, -1.0, 1e30])
@pytest.mark.parametrize("name,ndet,nmodes,path", PATHS, ids=[q[0] for q in PATHS])
def test_unmeasured_data_is_ignored_bitwise(pt, name, ndet, nmodes, path, garbage):
    import torch
    p, probe, data = problem(ndet, nmodes)
    mask = detector_mask(ndet)
    start = probe.swapaxes(2, 3).copy()
    zero = np.where(mask != 0, data, 0).astype(np.float32)
    bad = np.where(mask != 0, data, garbage).astype(np.float32)
    with solver(pt, p, ndet, path) as slv:
        want = gpu_run(slv, p, start, zero, mask=mask)
    with solver(pt, p, ndet, path) as slv:
        got = gpu_run(slv, p, start, bad, mask=torch.as_tensor(mask, device="cuda").float())
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    same_run(got, want)


@pytest.mark.parametrize("ndet,nmodes,path", [(64, 1, "default"), (64, 2, "default"), (100, 1, "torch")])
def test_masked_poisson_tracks_the_masked_reference(pt, ndet, nmodes, path):
    p, probe, data = problem(ndet, nmodes)
    track(pt, p, probe.swapaxes(2, 3).copy(), data, True, path, mask=detector_mask(ndet, seed=ndet), piter=4,
          cost_rtol=5e-4 if ndet == 100 else 1e-5, tol=2e-3 if ndet == 100 else 5e-4)


def test_model_option_values(pt):
    from libtike.hipfft import _native as nat
    p, probe, data = problem(32)
    with solver(pt, p, 32, "default") as slv:
        h = slv._h
        assert nat.get(h, nat.GET_MODEL) == nat.MODEL_GAUSSIAN
        assert nat.set_option(h, b"model", 1) == 0 and nat.get(h, nat.GET_MODEL) == 1
        assert nat.set_option(h, b"model", 2) == 1          # PTYCHO_ERR_ARG, the value stays
        assert b"model" in nat.last_error()
        assert nat.set_option(h, b"model", -1) == 1
        assert nat.get(h, nat.GET_MODEL) == 1
        assert nat.set_option(h, b"model", 0) == 0 and nat.get(h, nat.GET_MODEL) == 0


@pytest.mark.parametrize("path", ["default", "fused", "modes", "torch"])
def test_no_state_leaks_between_runs(pt, path):
    from libtike.hipfft import _native as nat
    ndet = 64
    p, probe, data = problem(ndet, 2 if path == "modes" else 1)
    start = probe.swapaxes(2, 3).copy()
    sp = "default" if path == "modes" else path
    with solver(pt, p, ndet, sp) as fresh:
        want = gpu_run(fresh, p, start, data, model="gaussian")
    with solver(pt, p, ndet, sp) as slv:
        pml = gpu_run(slv, p, start, data)
        assert nat.get(slv._h, nat.GET_MODEL) == nat.MODEL_GAUSSIAN
        with pytest.raises(UnboundLocalError):      # model="poisson" stays broken like the reference's
            gpu_run(slv, p, start, data, model="poisson")
        got = gpu_run(slv, p, start, data, model="gaussian")
    same_run(got, want)
    assert pml[3] != want[3]


def test_bitwise_reproducible_at_4096_positions(pt):
    """bench.py's CG geometry (4096 positions x 256^2, smooth probe): two poisson_ml runs give the same bits (the fused
    loops use the deterministic adjoints)."""
    import torch
    p = syn.make_problem(64, 64, 8, 256, 256, seed=1234, nz=768, n=768)
    dev = torch.device("cuda", 0)
    prb = torch.as_tensor(p["probe"][:, None].copy(), device=dev)
    scan0 = torch.as_tensor(p["scan"], device=dev)
    runs = []
    with pt.CGPtychoSolver(p["nscan"], 256, 256, 1, p["nz"], p["n"]) as slv:
        slv.verbose, slv.log_every = False, 1
        inten = torch.abs(slv.fwd(torch.as_tensor(p["psi"], device=dev), scan0, prb[:, 0])) ** 2
        torch.manual_seed(5)
        data = torch.poisson(inten * (20.0 / inten.max())).contiguous()
        del inten
        for _ in range(2):
            scan = scan0.clone()
            n0 = len(slv.history)
            res = slv.run(data, torch.ones((1, p["nz"], p["n"]), dtype=torch.complex64, device=dev), scan, prb.clone(),
                          piter=3, recover_prb=True, model="poisson_ml")
            runs.append((res["psi"].cpu().numpy(), res["probe"].cpu().numpy(), scan.cpu().numpy(), list(slv.history[n0:])))
    same_run(runs[0], runs[1])
    assert all(np.isfinite(h[3]) for h in runs[0][3])


def test_run_batch_partitions(pt):
    check_run_batch_partitions(pt, 64, 1, problem_kw={"dose": 20.0}, model="poisson_ml")


def test_two_rank_poisson_cg_matches_single_process(pt):
    """The all-reduced costs of both ranks are the Poisson sums: steps and logged costs are the single process's.  One
    iteration: the second one's object search accepts a step decided by rounding (UNRESOLVED_STEP), and two ranks sum
    in another order than one process."""
    ranks = two_rank_run({"ndet": 32, "seed": 31, "dose": 20.0}, {"piter": 1, "model": "poisson_ml"}, salt=1500)
    p, probe, data = problem(32, seed=31)
    with solver(pt, p, 32, "default") as slv:
        want = gpu_run(slv, p, probe, data, piter=1)
    assert_ranks_match(ranks, want)


@pytest.mark.xfail(strict=True, reason="measured: poisson_ml object error 0.834 against 0.424 for gaussian (DESIGN.md 6)")
def test_low_dose_reconstruction(pt):
    """Data Poisson-sampled at ~4 photons at the brightest pixel (256^2 detector, 100 positions).  poisson_ml and gaussian
    run the same 24 iterations from the same start; the object error (tests/recon_metrics.py) of poisson_ml should not be
    above the gaussian one.  Measured on an MI355X: poisson_ml 0.834, gaussian 0.424 -- the Poisson loop of the reference
    (gaussian probe rescale a / b, steps of ~1e-8 from the second iteration on) does not win here.  Kept as a strict
    expected failure: it turns into a failure of the suite the day poisson_ml wins."""
    ndet, piter = 256, 24
    p, probe, data = problem(ndet, ny=10, step=16, seed=21, dose=4.0)
    errs = {}
    with pt.CGPtychoSolver(p["nscan"], ndet, ndet, 1, p["nz"], p["n"]) as slv:
        slv.verbose = False
        for model in ("gaussian", "poisson_ml"):
            res = slv.run_batch(data, np.ones_like(p["psi"]), p["scan"].copy(), probe.copy(), piter=piter, model=model)
            errs[model] = rm.report(res["psi"], probe, p["psi"], probe, p["scan"])["obj_err"]
    print("object error:", errs)
    assert errs["poisson_ml"] <= errs["gaussian"], errs
