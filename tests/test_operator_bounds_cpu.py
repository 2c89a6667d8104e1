"""The operators' tolerance rule (``op_bounds`` of tests/hip_common.py) is never decided by its cap: on the inputs of the
GPU tests (tests/operator_cases.py, same seeds) the float32 oracle's own error against the float64 oracle, times ``FACTOR``,
stays below a quarter of ``REL_MAX`` and half of ``REL_L2``.  A condition on the inputs, not a tolerance on any kernel: an
input that makes the float32 restatement itself that inaccurate is the wrong input for the test.  No GPU, no torch."""
import numpy as np
import pytest

import operator_cases as oc
from hip_common import FACTOR, OP_FLOOR, REL_L2, REL_MAX, op_bounds, rel_errors


def check_e32(what, want64, want32, may_be_exact=False):
    assert want32.dtype == np.complex64 and want64.dtype == np.complex128, (what, want32.dtype, want64.dtype)
    e32 = rel_errors(want32, want64)
    bmax, bl2 = op_bounds(want64, want32)
    print("%s: float32 oracle max %.3g l2 %.3g -> bound max %.3g l2 %.3g" % (what, e32[0], e32[1], bmax, bl2))
    if not may_be_exact:
        assert e32[0] > 0 and e32[1] > 0, (what, e32)        # the restatement is a float32 evaluation, not the reference again
    assert FACTOR * e32[0] < REL_MAX / 4 and FACTOR * e32[1] < REL_L2 / 2, (what, e32)
    assert OP_FLOOR <= bmax < REL_MAX and OP_FLOOR <= bl2 < REL_L2, (what, bmax, bl2)
    return e32


@pytest.mark.parametrize("ndet,nprb,ny,nx,step,ntheta", [c for c in oc.CASES if c[0] <= 512])
def test_case_bounds_come_from_the_float32_oracle(ndet, nprb, ny, nx, step, ntheta):
    p, y = oc.case_inputs(ndet, nprb, ny, nx, step, ntheta)
    w64 = oc.oracles(p["psi"], p["scan"], p["probe"], y, ndet, "double")
    w32 = oc.oracles(p["psi"], p["scan"], p["probe"], y, ndet, "single")
    for name, a, b in zip(("fwd", "adj", "adj_probe"), w64, w32):
        check_e32("%d/%d %s" % (ndet, nprb, name), a, b)


@pytest.mark.parametrize("case", oc.EDGE_CASES)
def test_edge_case_bounds_come_from_the_float32_oracle(case):
    c = oc.edge_case(case)
    w64 = oc.oracles(c["psi"], c["scan"], c["prb"], c["y"], c["ndet"], "double")
    w32 = oc.oracles(c["psi"], c["scan"], c["prb"], c["y"], c["ndet"], "single")
    for name, a, b in zip(("fwd", "adj", "adj_probe"), w64, w32):
        if case == "all_skipped":
            assert not a.any() and not b.any()
            assert op_bounds(a, b) == (OP_FLOOR, OP_FLOOR)
        else:
            check_e32("%s %s" % (case, name), a, b)


def test_fft2_bounds_come_from_the_complex64_transform():
    for ndet, nb, tile, x in oc.fft2_inputs():
        (wf, wb), (sf, sb) = oc.fft2_oracles(x)
        check_e32("fft2 %d x %d forward" % (nb, ndet), wf, sf)
        check_e32("fft2 %d x %d inverse" % (nb, ndet), wb, sb)


@pytest.mark.parametrize("ndet", oc.FFT2_ANY_SIZES)
def test_fft2_any_size_bounds_come_from_the_complex64_transform(ndet):
    (wf, wb), (sf, sb) = oc.fft2_oracles(oc.fft2_any_size_input(ndet))
    check_e32("fft2 %d forward" % ndet, wf, sf)
    check_e32("fft2 %d inverse" % ndet, wb, sb)


@pytest.mark.parametrize("ndet,nprb", oc.WEIGHT_EDGES)
def test_weight_edge_positions_are_what_they_claim(ndet, nprb):
    """float32 keeps the intended integer parts and fractions, the last position ends on the last object row and column,
    and the float32 oracle on these inputs is an honest restatement too."""
    from oracle import ptycho_oracle as op
    c = oc.weight_edge_inputs(ndet, nprb)
    ip, fr, valid = op.split_positions(c["scan"], "double")
    assert valid.all()
    np.testing.assert_array_equal(ip, c["want_int"])
    np.testing.assert_array_equal(fr, c["want_frac"])                  # every intended fraction is exact in float32
    assert np.float32(1) - np.float32(oc.NEARLY_ONE) == np.float32(2.0 ** -24) and np.float32(oc.NEARLY_ONE) < 1
    assert ip[0, 7, 0] + nprb == c["nz"] - 1 and ip[0, 7, 1] + nprb == c["n"] - 1
    w64 = oc.oracles(c["psi"], c["scan"], c["prb"], c["y"], ndet, "double")
    w32 = oc.oracles(c["psi"], c["scan"], c["prb"], c["y"], ndet, "single")
    for name, a, b in zip(("fwd", "adj", "adj_probe"), w64, w32):
        check_e32("weights %d/%d %s" % (ndet, nprb, name), a, b)


@pytest.mark.parametrize("N", oc.STOCKHAM)
def test_impulse_references(N):
    """the closed form of the impulse tests is the float64 transform of the tiles"""
    x, wf, wb = oc.impulse_tiles(N)
    (nf, nb), _ = oc.fft2_oracles(x)
    assert np.abs(nf - wf).max() < 1e-12 and np.abs(nb - wb).max() < 1e-12


@pytest.mark.parametrize("ndet", oc.CANCEL_SIZES)
def test_cancellation_reference(ndet):
    c = oc.cancel_inputs(ndet)
    want = oc.oracles(c["psi"], c["scan"], c["prb"], np.zeros((1, 4, ndet, ndet), np.complex64), ndet, "double")[0]
    dc = np.zeros_like(want)
    dc[..., 0, 0] = ndet
    assert np.abs(want - dc).max() < 1e-9 * ndet
