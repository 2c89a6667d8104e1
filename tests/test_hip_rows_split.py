"""The split row pass of ndet 256 (``k_rows_split<256, -1 / +1>``, csrc/k_rows.hpp) against the float64 oracle and against
the un-split path (``set_split(False)``: ``k_rows<256>`` and the un-split column kernels, independent code for the same
numbers).  Needs an MI355X: ``pytest -m gpu``.

The pass exists at ndet 256 only, so every case is 256 x 256.  What the cases are there for:

(a) the inverse pass reads its source tile through ``tile_index`` (the sorted order): positions given in descending row
    order, one of them skipped;
(b) a probe narrower than the detector: the forward pass requests whole rows and masks the columns outside the strips
    afterwards, the inverse pass writes the strips' columns only;
(c) more positions than the forward grid has workgroups for, so that a workgroup walks several items: requests of the
    next item go out while LDS still holds the previous one.

Tolerances are the operators': against the oracle ``check_op`` of tests/hip_common.py (FACTOR x the float32 oracle's own
error), against the un-split path on the device the caps ``REL_MAX`` / ``REL_L2`` of that rule.
"""
import numpy as np
import pytest

from libtike.hipfft import synthetic as syn
from gatherwin_cases import SPLIT_FWD_C, strip_range
from operator_cases import oracles as oracles_at
from hip_common import REL_L2, REL_MAX, check_op, dev, host, pt, rel_errors  # noqa: F401

pytestmark = pytest.mark.gpu

NDET = 256
FWD_WG_PER_CU = 32          # launch_rows_split<256, -1>: workgroups per CU in the grid (csrc/host_ops.hpp)


def check(name, got, want):
    """device against device (the un-split path)"""
    e = rel_errors(got, np.asarray(want, dtype=np.complex128))
    print("%s: rel max %.3e  rel l2 %.3e" % (name, e[0], e[1]))
    assert e[0] < REL_MAX and e[1] < REL_L2, (name, e)


def random_farplane(shape, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def phase_probe(nprb, seed):
    rng = np.random.default_rng(seed)
    return (syn.gaussian_probe(nprb) * np.exp(2j * np.pi * rng.random((1, nprb, nprb)))).astype(np.complex64)


def oracles(psi, scan, prb, y, precision):
    return oracles_at(psi, scan, prb, y, NDET, precision)


def three_operators(slv, psi, scan, prb, y):
    return host(slv.fwd(psi, scan, prb)), host(slv.adj(y, scan, prb)), host(slv.adj_probe(y, scan, psi))


def test_order_and_skips(pt):
    """(a) 7 positions, nprb 256, rows descending (the sorted order is the reverse of the given one), position 3 skipped."""
    nprb, nz, n = 256, 256 + 80, 256 + 24
    rng = np.random.default_rng(21)
    scan = np.empty((1, 7, 2), np.float32)
    scan[0, :, 0] = 70.0 - 11.0 * np.arange(7) + rng.random(7)
    scan[0, :, 1] = 2.0 + 3.0 * (np.arange(7) % 3) + rng.random(7)      # two column buckets, rows descending in both
    scan[0, 3] = [-1.5, 4.25]                                            # skipped
    assert np.all(np.diff(np.delete(scan[0, :, 0], 3)) < 0)
    psi_h, prb_h = syn.random_object(nz, n, rng), phase_probe(nprb, 22)
    y_h = random_farplane((1, 7, NDET, NDET), 23)
    want, want32 = oracles(psi_h, scan, prb_h, y_h, "double"), oracles(psi_h, scan, prb_h, y_h, "single")
    with pt.PtychoCuFFT(7, nprb, NDET, 1, nz, n) as slv:
        psi, sc, prb, y = dev(psi_h), dev(scan), dev(prb_h), dev(y_h)
        got = three_operators(slv, psi, sc, prb, y)
        slv.set_split(False)
        ref = three_operators(slv, psi, sc, prb, y)
    assert np.all(got[0][0, 3] == 0)          # skipped position: exact zeros in every row
    for name, g, w, s, r in zip(("fwd", "adj", "adj_probe"), got, want, want32, ref):
        check_op(g, w, s, "rows_split %s against the oracle" % name)
        check(name + " against the un-split path", g, r)


def test_column_limits_inside_the_row(pt):
    """(b) nprb 128 (pad 64): the forward pass's columns [xa, xb) and the inverse pass's [wa, wb) are not the full row.
    The farplane buffer is filled with a finite sentinel before fwd: the padding columns, which the column pass never
    writes and the row pass now requests, must not reach the result."""
    nprb = 128
    strip0, nstrips = strip_range(NDET, nprb, SPLIT_FWD_C)
    assert strip0 > 0 and (strip0 + nstrips) * SPLIT_FWD_C < NDET
    p = syn.make_problem(3, 4, 13, nprb, NDET, seed=31)
    p["probe"] = phase_probe(nprb, 32)
    p["scan"][0, 5] = [-2.5, 3.0]                                         # skipped
    ns, nz, n = p["nscan"], p["nz"], p["n"]
    y_h = random_farplane((1, ns, NDET, NDET), 33)
    want, want32 = oracles(p["psi"], p["scan"], p["probe"], y_h, "double"), oracles(p["psi"], p["scan"], p["probe"], y_h, "single")
    import torch
    with pt.PtychoCuFFT(ns, nprb, NDET, 1, nz, n) as slv:
        psi, sc, prb, y = dev(p["psi"]), dev(p["scan"]), dev(p["probe"]), dev(y_h)
        outs = []
        for sentinel in (0.0, 3.0e30, -7.0):
            g = torch.full((1, ns, NDET, NDET), complex(sentinel, -sentinel), dtype=torch.complex64, device="cuda")
            outs.append(host(slv.fwd(psi, sc, prb, out=g)))
        got = (outs[0], host(slv.adj(y, sc, prb)), host(slv.adj_probe(y, sc, psi)))
        slv.set_split(False)
        ref = three_operators(slv, psi, sc, prb, y)
    for o in outs[1:]:
        np.testing.assert_array_equal(o, outs[0])                         # the result does not depend on the sentinel
    assert np.all(outs[1][0, 5] == 0)
    for name, g, w, s, r in zip(("fwd", "adj", "adj_probe"), got, want, want32, ref):
        check_op(g, w, s, "rows_split %s against the oracle" % name)
        check(name + " against the un-split path", g, r)


def test_several_items_per_workgroup(pt):
    """(c) more than 32 n_cu / 16 positions: the forward grid (32 workgroups per CU, 16 items per position) takes at least
    two items per workgroup.  Every position against the un-split path, a seeded sample of 32 against the oracle; the
    adjoints get a farplane that is zero outside the sample, so the oracle needs those 32 positions only while the pass
    still walks all of them."""
    import torch
    n_cu = torch.cuda.get_device_properties(0).multi_processor_count
    nprb = 256
    nx = 26
    ny = (FWD_WG_PER_CU * n_cu // 16) // nx + 1
    ns = ny * nx
    assert ns * 16 > FWD_WG_PER_CU * n_cu             # 520 positions on 256 CUs
    p = syn.make_problem(ny, nx, 5, nprb, NDET, seed=41)
    p["probe"] = phase_probe(nprb, 42)
    nz, n = p["nz"], p["n"]
    rng = np.random.default_rng(43)
    p["scan"][0] = p["scan"][0, rng.permutation(ns)]   # scan order is not the sorted order
    sample = np.sort(rng.choice(ns, size=32, replace=False))
    sub = np.ascontiguousarray(p["scan"][:, sample])
    y_s = random_farplane((1, 32, NDET, NDET), 44)
    want, want32 = oracles(p["psi"], sub, p["probe"], y_s, "double"), oracles(p["psi"], sub, p["probe"], y_s, "single")
    with pt.PtychoCuFFT(ns, nprb, NDET, 1, nz, n) as slv:
        psi, sc, prb = dev(p["psi"]), dev(p["scan"]), dev(p["probe"])
        y = torch.zeros((1, ns, NDET, NDET), dtype=torch.complex64, device="cuda")
        y[0, dev(sample)] = dev(y_s[0])
        yfull = dev(random_farplane((1, ns, NDET, NDET), 45))
        g = slv.fwd(psi, sc, prb)
        a, b = host(slv.adj(y, sc, prb)), host(slv.adj_probe(y, sc, psi))
        af, bf = host(slv.adj(yfull, sc, prb)), host(slv.adj_probe(yfull, sc, psi))
        slv.set_split(False)
        gr = slv.fwd(psi, sc, prb)
        afr, bfr = host(slv.adj(yfull, sc, prb)), host(slv.adj_probe(yfull, sc, psi))
        # every position of the forward result against the un-split path, on the device
        d = (g.to(torch.complex128) - gr.to(torch.complex128)).abs()
        per_pos = (d.amax(dim=(2, 3)) / gr.abs().amax(dim=(2, 3)).to(torch.float64))[0]
        l2 = torch.sqrt((d ** 2).sum() / (gr.abs().to(torch.float64) ** 2).sum()).item()
        print("fwd against the un-split path: worst position rel max %.3e  rel l2 %.3e" % (per_pos.max().item(), l2))
        assert per_pos.max().item() < REL_MAX and l2 < REL_L2, (int(per_pos.argmax()), per_pos.max().item(), l2)
        gs = host(g[:, dev(sample)])
    for name, g, w, s in zip(("fwd sample", "adj", "adj_probe"), (gs, a, b), want, want32):
        check_op(g, w, s, "rows_split several items %s against the oracle" % name)
    check("adj against the un-split path", af, afr)
    check("adj_probe against the un-split path", bf, bfr)
