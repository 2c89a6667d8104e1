"""The N > 1 path on the GPU kernels: two ``gloo`` ranks share the one GPU of the test box
(RCCL refuses two ranks on one device), each owns half of the scan positions and runs the
FUSED CG loop (``ptycho_cg_*`` kernels, position correction and probe recovery on) with
``CGPtychoSolver(group=...)``; both must end with the object / probe / cost trajectory of a
single-process run over all positions.  The production backend (nccl = RCCL, one rank per
GPU) differs only in the transport of the same all-reduces."""
import pytest

from cg_harness import assert_ranks_match, gpu_run, problem, solver, two_rank_run
from hip_common import pt  # noqa: F401

pytestmark = pytest.mark.gpu

#: 6 x 6 positions on a 32^2 detector, the probe under the phase screen of seed 4
PROBLEM = {"ndet": 32, "seed": 31, "screen": 4}


def test_two_rank_fused_cg_matches_single_process(pt):
    ranks = two_rank_run(PROBLEM, {"piter": 5}, salt=0)
    p, probe, data = problem(**PROBLEM)
    with solver(pt, p, 32) as slv:
        want = gpu_run(slv, p, probe, data, piter=5)
    assert_ranks_match(ranks, want)
