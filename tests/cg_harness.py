"""CG scenarios of the GPU tests (``test_hip_cg.py``, ``test_hip_mask.py``, ``test_hip_poisson.py``,
``test_hip_ortho.py``, ``test_hip_distributed.py``): the seeded problem, the solver on each of its loops, one run on the
GPU and one on the NumPy reference of ``cg_reference.py``, and the comparisons between them.  ``torch`` is imported
inside the functions that need it: the problem builders and the comparisons run without a GPU
(``test_harness_cpu.py``)."""
import os
import warnings

import numpy as np

import ortho_modes as om
from cg_cases import phase_screen
from cg_reference import ReferenceSolver
from hip_common import rel_max
from libtike.hipfft import synthetic as syn


# ---- inputs -------------------------------------------------------------------------------------------------------------
def intensity(p, probe):
    """Noiseless detector intensities of the problem ``p`` under all modes of ``probe``, float32."""
    ndet = probe.shape[-1]
    ora = ReferenceSolver(p["nscan"], ndet, ndet, 1, p["nz"], p["n"])
    inten = np.zeros((1, p["nscan"], ndet, ndet), np.float32)
    for k in range(probe.shape[1]):
        inten += np.abs(ora.fwd(p["psi"], p["scan"], probe[:, k])) ** 2
    return inten


def problem(ndet, nmodes=1, seed=7, ny=6, step=6, dose=None, modes="hermite", screen=None):
    """``(p, probe, data)``: ``ny`` x ``ny`` positions, probe mode(s) under a phase screen (``cg_cases.phase_screen``,
    seeded ``seed + 100`` unless ``screen`` says otherwise) and data consistent with them.

    ``modes="hermite"``: the Gaussian probe of ``synthetic.make_problem``, from two modes on ``synthetic.hermite_modes``;
    ``"mixed"``: the non-orthogonal smooth modes of ``ortho_modes.mode_stack``.  ``dose=None``: the noiseless
    intensities; else Poisson-sampled counts (seeded ``seed + 200``) with ``dose`` photons expected at the brightest
    pixel."""
    p = syn.make_problem(ny, ny, step, ndet, ndet, seed=seed)
    if modes == "mixed":
        probe = om.mode_stack(ndet, nmodes, seed=seed)
    else:
        probe = syn.hermite_modes(ndet, nmodes) if nmodes > 1 else p["probe"][:, None].copy()
    probe = phase_screen(probe, seed + 100 if screen is None else screen)
    inten = intensity(p, probe)
    if dose is None:
        return p, probe, inten
    rng = np.random.default_rng(seed + 200)
    return p, probe, rng.poisson(inten * (dose / inten.max())).astype(np.float32)


# ---- runs ----------------------------------------------------------------------------------------------------------------
def solver(pt, p, ndet, path="default"):
    """``default``: the loop the solver picks; ``fused``: the host-driven fused loop; ``torch``: statement by statement."""
    slv = pt.CGPtychoSolver(p["nscan"], ndet, ndet, 1, p["nz"], p["n"])
    slv.verbose, slv.log_every = False, 1
    if path == "fused":
        slv.native = False
    elif path == "torch":
        slv.fused = False
        slv.set_deterministic(True)   # the torch loop's adjoints use float atomics unless told otherwise
    return slv


def gpu_run(slv, p, probe, data, piter=4, recover=True, psi=None, **kw):
    """``(psi, probe, scan, history, res)`` of one ``slv.run`` from the flat object (or ``psi``); ``kw`` goes to ``run``."""
    import torch
    dev = torch.device("cuda", 0)
    scan = torch.as_tensor(p["scan"].copy(), device=dev)
    psi0 = np.ones_like(p["psi"]) if psi is None else psi
    n0 = len(slv.history)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = slv.run(torch.as_tensor(data, device=dev), torch.as_tensor(psi0.copy(), device=dev), scan,
                      torch.as_tensor(probe.copy(), device=dev), piter=piter, recover_prb=recover, **kw)
    torch.cuda.synchronize()
    return res["psi"].cpu().numpy(), res["probe"].cpu().numpy(), scan.cpu().numpy(), list(slv.history[n0:]), res


def reference(p, start, data, piter, precision, recover=True, psi=None, **kw):
    """``(psi, probe, scan, history)`` of ``ReferenceSolver.run`` in ``precision``; ``kw`` goes to ``run``."""
    ndet = data.shape[-1]
    ora = ReferenceSolver(p["nscan"], ndet, ndet, 1, p["nz"], p["n"], precision=precision)
    scan = p["scan"].copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = ora.run(data.copy(), np.ones_like(p["psi"]) if psi is None else psi.copy(), scan, start.copy(),
                      piter=piter, recover_prb=recover, **kw)
    return res["psi"], res["probe"], scan, ora.history


# ---- comparisons ------------------------------------------------------------------------------------------------------
#: an accepted step below this is decided at the float32 resolution of the cost: the second iteration's object search of
#: every Poisson case (after the probe rescale) accepts 1e-10 .. 2e-5, where f(trial) - f(p1) is a few float32 ulps of the
#: summed cost, and the float32 reference, the GPU loops (float32 partial sums per thread) and a two-rank run each accept
#: a different power of two there.  Measured: GPU 3.0e-8 / 1.5e-8 where the float64 reference accepts 1.5e-5 / 1.9e-6
#: (2 and 4 modes); the float32 reference agreed with float64 there by its summation order.
UNRESOLVED_STEP = 1e-4


def horizon(single, double):
    """Iterations that both references decide alike and on resolved line searches."""
    for i, (a, b) in enumerate(zip(single, double)):
        if a[1:3] != b[1:3] or 0.0 < b[1] < UNRESOLVED_STEP or 0.0 < b[2] < UNRESOLVED_STEP:
            return i
    return len(double)


def assert_follows(got, want, dsum, cost_rtol, tol, scan_tol=None):
    """``got`` and ``want`` are ``(psi, probe, scan, history, ...)``.  Every iteration of ``got`` has the index and the
    two accepted steps of ``want``; its logged cost, a sum of terms of both signs, is within ``cost_rtol * (|cost| +
    dsum)`` with ``dsum`` the sum of the measured data; object and probe are within ``tol`` of the largest element, the
    positions within ``scan_tol`` pixels where one is given."""
    for (i, gpsi, gprb, cost), (io, gpsi_o, gprb_o, cost_o) in zip(got[3], want[3]):
        assert i == io
        assert gpsi == gpsi_o and gprb == gprb_o, (got[3], want[3])
        assert abs(cost - cost_o) <= cost_rtol * (abs(cost_o) + dsum), (i, cost, cost_o, dsum)
    for k in (0, 1):
        d = rel_max(got[k], want[k])
        assert d < tol, (k, d)
    if scan_tol is not None:
        assert np.abs(got[2] - want[2]).max() < scan_tol


def track(pt, p, start, data, recover=True, path="default", piter=5, cost_rtol=1e-5, tol=5e-4, scan_tol=None,
          extra=None, **kw):
    """Steps, logged costs, object, probe (and positions) follow the float64 reference up to -- not beyond -- the
    iteration at which the float32 and float64 references themselves take different line-search decisions (or one of
    them is decided by rounding, UNRESOLVED_STEP).  ``kw`` (``model``, ``mask``, ``ortho_prb``) goes to the reference's
    and the solver's ``run`` alike; ``extra(got)`` checks what only one feature asserts."""
    single = reference(p, start, data, piter, "single", recover, **kw)[3]
    double = reference(p, start, data, piter, "double", recover, **kw)
    split = horizon(single, double[3])
    assert split >= 1, (single, double[3])      # the case must say something
    if split < piter:
        double = reference(p, start, data, split, "double", recover, **kw)
    with solver(pt, p, data.shape[-1], path) as slv:
        got = gpu_run(slv, p, start, data, piter=split, recover=recover, **kw)
    assert len(got[3]) == split
    mask = kw.get("mask")
    dsum = float(np.where(mask != 0, data, 0).sum()) if mask is not None else float(data.sum())
    assert_follows(got, double, dsum, cost_rtol, tol, scan_tol)
    if extra is not None:
        extra(got)
    return split


def same_run(a, b):
    """Two ``gpu_run`` results have the same bits: object, probe and positions (shape and bytes), and the history."""
    for x, y in zip(a[:3], b[:3]):
        assert x.shape == y.shape and x.tobytes() == y.tobytes()
    assert a[3] == b[3]


def check_run_batch_partitions(pt, ndet, nmodes, problem_kw=None, swap=True, single_kw=None, log_every=32, **run_kw):
    """``run_batch`` over two independent angles gives the bits of ``run`` on each angle alone.  ``run_kw`` goes to
    both; ``single_kw`` replaces entries of it for the single runs (the same option in another form).  ``swap``: start
    from the transposed probes.  ``log_every``: how often the host reads the logged cost back (the solver's default).
    Returns the ``run_batch`` result."""
    import torch
    problem_kw = problem_kw or {}
    p, probe, data = problem(ndet, nmodes, **problem_kw)
    q, probe2, data2 = problem(ndet, nmodes, **dict(problem_kw, seed=9))
    assert p["nz"] == q["nz"] and p["n"] == q["n"]
    start = np.concatenate([probe, probe2])
    if swap:
        start = start.swapaxes(2, 3).copy()
    D = np.concatenate([data, data2])
    S = np.concatenate([p["scan"], q["scan"]])
    psi = np.ones((2, p["nz"], p["n"]), np.complex64)
    with solver(pt, p, ndet) as slv:
        slv.log_every = log_every
        got = slv.run_batch(D, psi, S.copy(), start.copy(), piter=4, recover_prb=True, **run_kw)
    dev = torch.device("cuda", 0)
    for k in range(2):
        with solver(pt, p, ndet) as slv:
            slv.log_every = log_every
            res = slv.run(torch.as_tensor(D[k:k + 1].copy(), device=dev), torch.as_tensor(psi[k:k + 1].copy(), device=dev),
                          torch.as_tensor(S[k:k + 1].copy(), device=dev), torch.as_tensor(start[k:k + 1].copy(), device=dev),
                          piter=4, recover_prb=True, **dict(run_kw, **(single_kw or {})))
        torch.cuda.synchronize()
        assert res["psi"].cpu().numpy().tobytes() == got["psi"][k:k + 1].tobytes()
        assert res["probe"].cpu().numpy().tobytes() == got["probe"][k:k + 1].tobytes()
    return got


# ---- two ranks -----------------------------------------------------------------------------------------------------------
def _rank_main(rank, world, port, out, problem_args, run_kwargs):
    """One ``gloo`` rank on its half of the positions (module level: ``mp.spawn`` pickles it by name)."""
    import torch
    import torch.distributed as dist
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        import libtike.hipfft as pt
        from libtike.hipfft.distributed import shard_slice
        p, probe, data = problem(**problem_args)
        ndet = data.shape[-1]
        sl = shard_slice(p["nscan"], rank, world)
        dev = torch.device("cuda", 0)
        with pt.CGPtychoSolver(sl.stop - sl.start, ndet, ndet, 1, p["nz"], p["n"], group=dist.group.WORLD) as slv:
            slv.verbose, slv.log_every = False, 1
            assert slv.fused
            res = slv.run(torch.as_tensor(data[:, sl].copy(), device=dev),
                          torch.ones((1, p["nz"], p["n"]), dtype=torch.complex64, device=dev),
                          torch.as_tensor(p["scan"][:, sl].copy(), device=dev),
                          torch.as_tensor(probe.copy(), device=dev), recover_prb=True, **run_kwargs)
            out[rank] = (res["psi"].cpu().numpy(), res["probe"].cpu().numpy(), list(slv.history))
    finally:
        dist.destroy_process_group()


def two_rank_run(problem_args, run_kwargs, salt):
    """``problem(**problem_args)`` solved by two ``gloo`` ranks that share the one GPU, each on half of the positions
    with ``run(..., recover_prb=True, **run_kwargs)``.  Returns ``[(psi, probe, history)]`` by rank.  ``salt`` keeps the
    rendezvous ports of the tests of one session apart."""
    import torch.multiprocessing as mp
    mgr = mp.Manager()
    out = mgr.dict()
    port = 29700 + ((os.getpid() + salt) % 2000)
    mp.spawn(_rank_main, args=(2, port, out, problem_args, run_kwargs), nprocs=2, join=True)
    return [out[r] for r in (0, 1)]


def assert_ranks_match(ranks, want):
    """Both ranks end within 2e-4 of the object and probe of ``want``, the single process's ``gpu_run``, with its steps
    and, to 2e-4, its logged costs; the two replicas of the object agree bitwise."""
    for psi, prb, h in ranks:
        assert np.abs(psi - want[0]).max() < 2e-4 * np.abs(want[0]).max()
        assert np.abs(prb - want[1]).max() < 2e-4 * np.abs(want[1]).max()
        for a, b in zip(h, want[3]):
            assert a[:3] == b[:3] and abs(a[3] - b[3]) <= 2e-4 * abs(b[3]), (a, b)
    np.testing.assert_array_equal(ranks[0][0], ranks[1][0])
