"""Long-horizon reconstructions: the reference's two demo scripts at their own length (128 iterations, probe recovery) on
its own fixtures, checked against the TRUTH the data were simulated from -- north_star's "reconstructed object within
stated float tolerance".

* ``/root/reference/tests/test.py:18-64``       one mode, 1000 positions (the script's own ``nscan``; the fixture holds
  5706, also run), probe started from the transposed true probe;
* ``/root/reference/tests/test_modes.py:18-60`` three incoherent modes, ``coords[:5500:5]`` = 1100 positions, probes
  started from the true ones normalised to max 1.

The reference stores no reconstruction (its scripts write TIFFs for a human to look at), and 128 oracle iterations take
the CPU restatement most of an hour (``tools/recon_calib.py --backend oracle``: the thresholds below were set from such a
run and from the GPU runs recorded in ``profiles/r04/reconstruction.txt``), so the checks are on the physics: the data
cost must fall to a small fraction of its start value, and the recovered object / probe must approach the truth inside
the lit region after the one complex factor a ptychographic solution leaves open (``tests/recon_metrics.py``).  The
6-iteration trajectory comparisons with the oracle stay in ``tests/test_hip_reference_scenarios.py``.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import recon_metrics as rm  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import recon_calib as rc  # noqa: E402  (scenario(): the two scripts' inputs from the fixtures)
from hip_common import pt  # noqa: E402, F401

pytestmark = pytest.mark.gpu


def reconstruct(pt, model, which, nscan, piter):
    psi0, prb_true, prb_init, scan = rc.scenario(model, which, nscan)
    nscan = scan.shape[1]
    with pt.CGPtychoSolver(nscan, rc.NPRB, rc.NDET, 1, rc.NZ, rc.N) as slv:
        slv.verbose, slv.log_every = False, 1
        data = np.zeros([1, nscan, rc.NDET, rc.NDET], dtype="float32")
        for k in range(prb_true.shape[1]):
            data += np.abs(slv.fwd_ptycho_batch(psi0, scan, prb_true[:, k:k + 1])) ** 2
        psi = np.ones([1, rc.NZ, rc.N], dtype="complex64")
        res = slv.run_batch(data, psi, scan, prb_init.copy(), piter=piter, model="gaussian", recover_prb=True)
        hist = list(slv.history)
    start = rm.report(psi, prb_init, psi0, prb_true, scan)
    end = rm.report(res["psi"], res["probe"], psi0, prb_true, scan)
    return start, end, hist


# (cost_last / cost_first <, object error <, |true|^2-weighted object phase rms [rad] <, worst probe-mode error <)
# Observed on MI355X (profiles/r04/reconstruction.txt), metric of tests/recon_metrics.py (best complex factor, common
# sub-pixel translation, lit region):
#   single, 1000 positions: 0.0035, 0.066, 0.046, 0.152   (start: object 0.298, probe 0.491 -- the transposed true probe)
#   single, 5706 positions: see the file                   (same start)
#   3 modes, 1100 positions: 0.0009, 0.019, 0.015, 0.061  (start: object 0.321; the probes start at the truth up to scale)
# The NumPy oracle's own 128 iterations of the first scenario (tools/recon_calib.py --backend oracle, 45 minutes) are in
# the same file.  The thresholds leave a factor 1.5-2 for other boxes / summation orders: CG on this problem is not
# bitwise stable across implementations, the quality of the result is.
THRESHOLDS = {
    "single-1000": (0.01, 0.12, 0.08, 0.25),
    "single-5706": (0.01, 0.12, 0.08, 0.25),
    "modes-1100": (0.005, 0.04, 0.03, 0.12),
}


@pytest.mark.parametrize("which,nscan", [("single", 1000), ("single", 5706), ("modes", 1100)])
def test_demo_reconstruction_recovers_object_and_probe(pt, model, which, nscan):
    """128 iterations with probe recovery, as the reference's scripts run them (tests/test.py:27, tests/test_modes.py:27)."""
    start, end, hist = reconstruct(pt, model, which, nscan, 128)
    cost_max, obj_max, phase_max, prb_max = THRESHOLDS["%s-%d" % (which, nscan)]
    costs = [h[3] for h in hist]
    assert len(costs) == 128 and all(np.isfinite(costs))
    assert costs[-1] < cost_max * costs[0], (costs[0], costs[-1])
    assert end["obj_err"] < obj_max and end["obj_err"] < 0.4 * start["obj_err"], (start, end)
    assert end["obj_phase_rms"] < phase_max, (start, end)
    assert max(end["prb_err"]) < prb_max, (start, end)
    if which == "single":   # the probe starts far away (transposed): it has to move towards the truth
        assert end["prb_err"][0] < 0.5 * start["prb_err"][0], (start, end)
    assert end["lit_fraction"] > 0.15
