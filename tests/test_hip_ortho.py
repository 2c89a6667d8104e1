"""Orthogonal probe modes on the GPU: ``libtike.hipfft.orthogonalize_modes`` (C ABI ``ptycho_orthogonalize_modes``)
against the float64 NumPy reference of tests/ortho_modes.py, and ``CGPtychoSolver.run(..., ortho_prb=True)`` on the fused
multi-mode loop and the torch loop against the reference loop of tests/cg_reference.py."""
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import cg_harness as cg  # noqa: E402
import ortho_modes as om  # noqa: E402
from cg_harness import assert_ranks_match, check_run_batch_partitions, gpu_run, same_run, solver, two_rank_run  # noqa: E402
from cg_reference import detector_mask  # noqa: E402
from hip_common import dev, pt  # noqa: E402, F401
import recon_metrics as rm  # noqa: E402
from libtike.hipfft import synthetic as syn  # noqa: E402

pytestmark = pytest.mark.gpu


def max_rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()   # not hip_common.rel_max: the difference in the arrays' own precision


# ---- the helper ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nprb", [64, 128, 256])
@pytest.mark.parametrize("nmodes", [2, 3, 4, 8, 12])
def test_helper_matches_reference(pt, nmodes, nprb):
    probe = om.mixed_probe(nmodes, nprb=nprb, ptheta=2, seed=nmodes * 1000 + nprb)
    d, g0 = om.mixed_probe(nmodes, nprb, 2, seed=1), om.mixed_probe(nmodes, nprb, 2, seed=2)
    want, (wd, wg0), wpow, _ = om.orthogonalize(probe, d, g0)
    runs = []
    for _ in range(2):
        x, y, z = dev(probe), dev(d), dev(g0)
        powers = pt.orthogonalize_modes(x, y, z)
        runs.append([t.cpu().numpy() for t in (x, y, z, powers)])
    for a, b in zip(*runs):
        assert a.tobytes() == b.tobytes()                   # bitwise reproducible
    got, gd, gg0, gpow = runs[0]
    assert gpow.dtype == np.float64 and gpow.shape == (2, nmodes)
    assert max_rel(gpow, wpow) < 1e-9, (gpow, wpow)
    for t in range(2):
        assert max_rel(got[t], want[t]) < 1e-5
        assert max_rel(gd[t], wd[t]) < 1e-5 and max_rel(gg0[t], wg0[t]) < 1e-5
    g = om.gram(got)
    for t in range(2):
        assert np.abs(g[t] - np.diag(np.diag(g[t]))).max() <= 1e-5 * np.diag(g[t]).real.max()


def test_helper_one_mode_and_non_contiguous(pt):
    import torch
    probe = om.mixed_probe(1, nprb=64, ptheta=3, seed=5)
    x = dev(probe)
    powers = pt.orthogonalize_modes(x)
    assert x.cpu().numpy().tobytes() == probe.tobytes()
    assert max_rel(powers.cpu().numpy(), om.gram(probe)[:, :, 0].real) < 1e-9
    # a transposed view is rotated through a contiguous copy and written back
    probe = om.mixed_probe(3, nprb=64, ptheta=1, seed=6)
    base = dev(probe.swapaxes(2, 3))
    view = base.transpose(2, 3)
    assert not view.is_contiguous()
    pt.orthogonalize_modes(view)
    assert max_rel(view.cpu().numpy(), om.orthogonalize(probe)[0]) < 1e-5
    with pytest.raises(ValueError):
        pt.orthogonalize_modes(torch.zeros((1, 17, 8, 8), dtype=torch.complex64, device="cuda"))


def test_summed_intensity_is_unchanged(pt):
    p = syn.make_problem(6, 6, 10, 64, 64, seed=3)
    probe = om.mixed_probe(4, nprb=64, ptheta=1, seed=7)
    with pt.CGPtychoSolver(p["nscan"], 64, 64, 1, p["nz"], p["n"]) as slv:
        psi, scan = dev(p["psi"]), dev(p["scan"])

        def inten(modes):
            return sum((abs(slv.fwd(psi, scan, modes[:, k].contiguous())) ** 2).cpu().numpy() for k in range(4))
        x = dev(probe)
        before = inten(x)
        pt.orthogonalize_modes(x)
        after = inten(x)
    assert max_rel(after, before) < 1e-5


# ---- the CG loop ------------------------------------------------------------------------------------------------------------
#: non-orthogonal smooth modes (ortho_modes.mode_stack) under a phase screen
problem = functools.partial(cg.problem, modes="mixed")


def assert_orthogonal(probe):
    g = om.gram(probe)
    for t in range(g.shape[0]):
        d = np.diag(g[t]).real
        assert np.abs(g[t] - np.diag(np.diag(g[t]))).max() <= 1e-5 * d.max(), g[t]
        assert np.all(np.diff(d) <= 0), d


def assert_modes(got):
    """The probe of a ``gpu_run`` is orthogonal, and ``mode_powers`` are its modes' powers."""
    assert_orthogonal(got[1])
    powers = got[4]["mode_powers"].cpu().numpy()
    assert max_rel(powers[0], np.diag(om.gram(got[1])[0]).real) < 1e-5


def track(pt, p, start, data, path="default", **kw):
    """cg_harness.track with ortho_prb=True, and the modes stay orthogonal."""
    return cg.track(pt, p, start, data, True, path, ortho_prb=True, extra=assert_modes, **kw)


# (name, ndet, nmodes, path): the fused multi-mode loop at 128^2 and 256^2, the torch loop beyond 8 modes
TRACK = [("modes2_128", 128, 2, "default"), ("modes3_128", 128, 3, "default"), ("modes4_128", 128, 4, "default"),
         ("modes2_256", 256, 2, "default"), ("modes3_256", 256, 3, "default"), ("modes4_256", 256, 4, "default"),
         ("modes10_64", 64, 10, "torch")]


@pytest.mark.parametrize("name,ndet,nmodes,path", TRACK, ids=[t[0] for t in TRACK])
def test_ortho_cg_tracks_the_reference(pt, name, ndet, nmodes, path):
    p, start, data = problem(ndet, nmodes)
    track(pt, p, start, data, path=path)


def test_ortho_with_mask(pt):
    p, start, data = problem(128, 3)
    track(pt, p, start, data, mask=detector_mask(128))


def test_ortho_with_poisson_ml(pt):
    p, start, data = problem(128, 3, dose=1000.0)
    track(pt, p, start, data, model="poisson_ml")


def test_ortho_on_the_torch_loop(pt):
    p, start, data = problem(64, 3)
    track(pt, p, start, data, path="torch")


def test_run_batch_partitions(pt):
    got = check_run_batch_partitions(pt, 64, 3, problem_kw={"modes": "mixed"}, swap=False, log_every=1, ortho_prb=True)
    assert_orthogonal(got["probe"])


# ---- no effect when off ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nmodes,path", [(2, "default"), (10, "torch"), (3, "torch")])
def test_off_is_the_plain_loop_and_leaves_no_state(pt, nmodes, path):
    p, start, data = problem(64, nmodes)
    with solver(pt, p, 64, path) as slv:
        plain = gpu_run(slv, p, start, data, 3)
    with solver(pt, p, 64, path) as slv:
        off = gpu_run(slv, p, start, data, 3, ortho_prb=False)
        on = gpu_run(slv, p, start, data, 3, ortho_prb=True)
        after = gpu_run(slv, p, start, data, 3)
    same_run(off, plain)
    same_run(after, plain)
    assert "mode_powers" not in plain[4] and "mode_powers" in on[4]
    assert on[1].tobytes() != plain[1].tobytes()
    assert_orthogonal(on[1])


def test_single_mode_and_no_probe_recovery_are_untouched(pt):
    import torch
    p, start, data = problem(64, 1)
    with solver(pt, p, 64) as slv:
        a = gpu_run(slv, p, start, data, 3)
        b = gpu_run(slv, p, start, data, 3, ortho_prb=True)
    same_run(a, b)
    p, start, data = problem(64, 3)
    outs = []
    for kw in ({}, {"ortho_prb": True}):
        with solver(pt, p, 64) as slv:
            res = slv.run(dev(data), dev(np.ones_like(p["psi"])), dev(p["scan"].copy()), dev(start.copy()), piter=3,
                          recover_prb=False, **kw)
            torch.cuda.synchronize()
            outs.append((res["psi"].cpu().numpy().tobytes(), res["probe"].cpu().numpy().tobytes(), sorted(res)))
    assert outs[0] == outs[1]


def test_more_than_16_modes_raise(pt):
    p, start, data = problem(32, 1)
    start17 = np.repeat(start, 17, axis=1)
    with solver(pt, p, 32) as slv:
        with pytest.raises(ValueError):
            gpu_run(slv, p, start17, data, 1, ortho_prb=True)


# ---- two ranks ----------------------------------------------------------------------------------------------------------------
def test_two_rank_ortho_matches_single_process(pt):
    ranks = two_rank_run({"ndet": 32, "nmodes": 3, "seed": 31, "modes": "mixed"}, {"piter": 1, "ortho_prb": True}, salt=1700)
    p, probe, data = problem(32, 3, seed=31)
    with solver(pt, p, 32) as slv:
        want = gpu_run(slv, p, probe, data, 1, ortho_prb=True)
    assert ranks[0][1].tobytes() == ranks[1][1].tobytes()       # every rank computes the same V
    assert_ranks_match(ranks, want)
    assert_orthogonal(ranks[0][1])


# ---- the reference's 3-mode demo ----------------------------------------------------------------------------------------
def demo(pt, model, ortho, piter=128):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import recon_calib as rc
    psi0, prb_true, prb_init, scan = rc.scenario(model, "modes", 1100)
    nscan = scan.shape[1]
    with pt.CGPtychoSolver(nscan, rc.NPRB, rc.NDET, 1, rc.NZ, rc.N) as slv:
        slv.verbose, slv.log_every = False, 1
        data = np.zeros([1, nscan, rc.NDET, rc.NDET], dtype="float32")
        for k in range(prb_true.shape[1]):
            data += np.abs(slv.fwd_ptycho_batch(psi0, scan, prb_true[:, k:k + 1])) ** 2
        psi = np.ones([1, rc.NZ, rc.N], dtype="complex64")
        res = slv.run_batch(data, psi, scan, prb_init.copy(), piter=piter, model="gaussian", recover_prb=True,
                            ortho_prb=ortho)
        costs = [h[3] for h in slv.history]
    # per-mode errors mean nothing after mixing: the incoherent illumination sum_k |P_k|^2 against the truth's, and the
    # object at the translation read off that illumination
    illum = np.sum(np.abs(res["probe"][0]) ** 2, axis=0)
    illum_true = np.sum(np.abs(prb_true[0]) ** 2, axis=0)
    ill_err, _, shift, _ = rm.aligned_error(illum.astype(np.complex128), illum_true.astype(np.complex128))
    mask = rm.lit_mask(scan[0], prb_true[0], rc.NZ, rc.N)
    obj_err, _ = rm.scaled_error(rm.fourier_shift(res["psi"][0], *shift), psi0[0], mask)
    return {"obj_err": obj_err, "illum_err": ill_err, "cost_ratio": costs[-1] / costs[0], "probe": res["probe"]}


# Measured on an MI355X (profiles/r05/ortho.txt), 128 iterations, 1100 positions:
#   ortho_prb=True : object 0.0178, illumination 0.0069, cost ratio 8.80e-4
#   ortho_prb=False: object 0.0187, illumination 0.0069, cost ratio 8.94e-4
# The thresholds leave a factor 2 over the ortho_prb=True figures (CG on this problem is not bitwise stable across
# implementations, the quality of the result is).
DEMO_THRESHOLDS = {"obj_err": 0.036, "illum_err": 0.014, "cost_ratio": 0.0018}


def test_demo_reconstruction_with_ortho(pt, model):
    on = demo(pt, model, True)
    off = demo(pt, model, False)
    print("ortho_prb=True : object %.4f, illumination %.4f, cost ratio %.2e" % (on["obj_err"], on["illum_err"], on["cost_ratio"]))
    print("ortho_prb=False: object %.4f, illumination %.4f, cost ratio %.2e" % (off["obj_err"], off["illum_err"], off["cost_ratio"]))
    assert_orthogonal(on["probe"])
    for key, limit in DEMO_THRESHOLDS.items():
        assert on[key] < limit, (key, on[key], off[key])
