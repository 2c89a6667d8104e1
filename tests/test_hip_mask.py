"""Measured-pixel mask of the CG reconstruction on the GPU: ``CGPtychoSolver.run(..., mask=)`` on every loop (native,
fused, multi-mode, statement-by-statement torch), against the NumPy reference of tests/cg_reference.py."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cg_harness import (assert_ranks_match, check_run_batch_partitions, gpu_run, problem, same_run, solver,  # noqa: E402
                        two_rank_run)
from cg_reference import ReferenceSolver, detector_mask, random_mask  # noqa: E402
from hip_common import dev, pt  # noqa: E402, F401
import recon_metrics as rm  # noqa: E402

pytestmark = pytest.mark.gpu


# (name, ndet, nmodes, solver path): native single mode, the fused single-mode loop, the multi-mode loop, the torch loop
# on a power of two, the torch loop on a size without a Stockham plan (Bluestein operators)
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


CASES = [(32, 1, False), (32, 1, True), (32, 2, True), (32, 2, False), (64, 1, True), (64, 2, True), (64, 1, False),
         (112, 1, True), (100, 1, True)]


@pytest.mark.parametrize("ndet,nmodes,recover", CASES)
def test_masked_cg_tracks_the_masked_reference(pt, ndet, nmodes, recover):
    """The standard of test_hip_cg.py::test_cg_tracks_the_oracle, with the detector mask."""
    p, probe, data = problem(ndet, nmodes)
    mask = detector_mask(ndet, seed=ndet)
    start = probe.swapaxes(2, 3).copy() if recover else probe.copy()
    piter = 5
    ora = ReferenceSolver(p["nscan"], ndet, ndet, 1, p["nz"], p["n"])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        want = ora.run(data.copy(), np.ones_like(p["psi"]), p["scan"].copy(), start.copy(), piter=piter,
                       recover_prb=recover, mask=mask)
    with pt.CGPtychoSolver(p["nscan"], ndet, ndet, 1, p["nz"], p["n"]) as slv:
        slv.verbose, slv.log_every = False, 1
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            got = slv.run_batch(data.copy(), np.ones_like(p["psi"]), p["scan"].copy(), start.copy(), piter=piter,
                                recover_prb=recover, mask=mask)
        hist = list(slv.history)
    assert len(hist) == piter
    for (i, gpsi, gprb, cost), (io, gpsi_o, gprb_o, cost_o) in zip(hist, ora.history):
        assert i == io
        assert abs(cost - cost_o) <= 1e-4 * abs(cost_o), (i, cost, cost_o)
        assert gpsi == gpsi_o and gprb == gprb_o, (i, gpsi, gpsi_o, gprb, gprb_o)
    d = np.abs(got["psi"] - want["psi"]).max() / np.abs(want["psi"]).max()
    assert d < 2e-4, d
    dp = np.abs(got["probe"] - want["probe"]).max() / np.abs(want["probe"]).max()
    assert dp < 2e-4, dp


@pytest.mark.parametrize("path", ["default", "torch"])
def test_gradient_vanishes_at_the_truth(pt, path):
    """At the true object and probe with -1 in the unmeasured pixels, one masked iteration stays at the truth; the same
    call without the mask does not (sqrt(-1) = NaN, or the fit of the -1s moves the object)."""
    ndet = 64
    p, probe, data = problem(ndet)
    mask = random_mask(ndet)
    bad = np.where(mask != 0, data, -1.0).astype(np.float32)
    truth = p["psi"].astype(np.complex64)
    with solver(pt, p, ndet, path) as slv:
        psi = gpu_run(slv, p, probe, bad, mask=mask, piter=1, recover=False, psi=truth)[0]
    assert np.abs(psi - truth).max() < 1e-4 * np.abs(truth).max(), np.abs(psi - truth).max()
    with solver(pt, p, ndet, path) as slv:
        psi = gpu_run(slv, p, probe, bad, piter=1, recover=False, psi=truth)[0]
    assert not np.isfinite(psi).all() or np.abs(psi - truth).max() > 1e-3 * np.abs(truth).max()


@pytest.mark.parametrize("path", ["default", "fused", "torch"])
def test_no_state_leaks_between_runs(pt, path):
    from libtike.hipfft import _native as nat
    ndet = 64
    p, probe, data = problem(ndet)
    start = probe.swapaxes(2, 3).copy()
    mask = detector_mask(ndet)
    with solver(pt, p, ndet, path) as fresh:
        want = gpu_run(fresh, p, start, data)
    with solver(pt, p, ndet, path) as slv:
        masked = gpu_run(slv, p, start, data, mask=mask)
        assert nat.get(slv._h, nat.GET_MASK) == 0
        with pytest.raises(UnboundLocalError):      # model="poisson" is broken like the reference's; the mask is cleared
            gpu_run(slv, p, start, data, mask=mask, model="poisson")
        assert nat.get(slv._h, nat.GET_MASK) == 0
        got = gpu_run(slv, p, start, data)
    same_run(got, want)
    assert masked[3] != want[3]


def test_run_batch_partitions_with_a_mask(pt):
    mask = detector_mask(64)
    check_run_batch_partitions(pt, 64, 1, mask=mask, single_kw={"mask": dev(mask != 0)})


def test_bad_masks_are_rejected(pt):
    import torch
    from libtike.hipfft import _native as nat
    ndet = 32
    p, probe, data = problem(ndet)
    with solver(pt, p, ndet, "default") as slv:
        with pytest.raises(ValueError):
            gpu_run(slv, p, probe, data, mask=np.ones((ndet, ndet + 1)), piter=1)
        with pytest.raises(ValueError):
            gpu_run(slv, p, probe, data, mask=np.zeros((ndet, ndet)), piter=1)
        # the C ABI: a device mask with no measured pixel, then a good one, then clear
        z = torch.zeros((ndet, ndet), dtype=torch.uint8, device="cuda")
        assert nat.set_mask(slv._h, ctypes.c_void_p(z.data_ptr()), None) == 1
        assert b"no measured pixel" in nat.last_error()
        assert nat.get(slv._h, nat.GET_MASK) == 0
        z[3, 5] = 7
        assert nat.set_mask(slv._h, ctypes.c_void_p(z.data_ptr()), None) == 0
        assert nat.get(slv._h, nat.GET_MASK) == 1
        assert nat.set_mask(slv._h, None, None) == 0
        assert nat.get(slv._h, nat.GET_MASK) == 0
        slv.free()
        assert nat.set_mask(slv._h, None, None) == 3


def test_masked_reconstruction_of_a_detector_with_dead_regions(pt):
    """256^2 detector with a beamstop, module gaps and 2 % dead pixels that read 0.  The masked run's object error
    (tests/recon_metrics.py) is below half of the same run without the mask, and within 1.5x of a run on complete
    data."""
    ndet, piter = 256, 24
    p, probe, full = problem(ndet, ny=10, step=16, seed=21)
    mask = detector_mask(ndet, seed=3)
    dead = np.where(mask != 0, full, 0).astype(np.float32)
    errs = {}
    with pt.CGPtychoSolver(p["nscan"], ndet, ndet, 1, p["nz"], p["n"]) as slv:
        slv.verbose = False
        for key, d, m in (("complete", full, None), ("masked", dead, mask), ("unmasked", dead, None)):
            res = slv.run_batch(d, np.ones_like(p["psi"]), p["scan"].copy(), probe.copy(), piter=piter, mask=m)
            errs[key] = rm.report(res["psi"], probe, p["psi"], probe, p["scan"])["obj_err"]
    print("object error:", errs)
    assert errs["masked"] < 0.5 * errs["unmasked"], errs
    assert errs["masked"] < 1.5 * errs["complete"], errs


def test_two_rank_masked_cg_matches_single_process(pt):
    ranks = two_rank_run({"ndet": 32, "seed": 31}, {"piter": 5, "mask": detector_mask(32)}, salt=1000)
    p, probe, data = problem(32, seed=31)
    with solver(pt, p, 32, "default") as slv:
        want = gpu_run(slv, p, probe, data, mask=detector_mask(32), piter=5)
    assert_ranks_match(ranks, want)
