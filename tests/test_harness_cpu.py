"""The helpers that decide pass or fail for the GPU tests (``tests/hip_common.py``, ``tests/cg_harness.py``), on inputs
they must reject.  No GPU."""
import numpy as np
import pytest

from cg_harness import UNRESOLVED_STEP, assert_follows, horizon, same_run
from hip_common import FACTOR, bound, rel_errors, rel_max, same_bits


# ---- same_bits -------------------------------------------------------------------------------------------------------------
def test_same_bits_sees_one_bit_and_the_sign_of_zero():
    a = np.array([1.0, 2.0, 0.0], np.float32)
    assert same_bits(a, a.copy())
    b = a.copy()
    b.view(np.uint32)[1] ^= 1                                # the last mantissa bit of 2.0
    assert not same_bits(a, b)
    assert np.array_equal(a, np.array([1.0, 2.0, -0.0], np.float32))
    assert not same_bits(a, np.array([1.0, 2.0, -0.0], np.float32))


def test_same_bits_takes_equal_nan_payloads_as_equal():
    a = np.array([np.nan, 1.0])
    assert not np.array_equal(a, a.copy()) and same_bits(a, a.copy())
    b = a.copy()
    b.view(np.uint64)[0] ^= 1                                # another payload
    assert np.isnan(b[0]) and not same_bits(a, b)


def test_same_bits_rejects_another_shape_or_dtype():
    a = np.arange(8, dtype=np.float32).reshape(2, 4)
    assert same_bits(a, a.T.copy().T)                        # the layout in memory does not matter
    assert not same_bits(a, a.reshape(4, 2))
    assert not same_bits(a, a.view(np.int32))
    assert not same_bits(a, a.view(np.float64))              # the same 32 bytes


# ---- same_run --------------------------------------------------------------------------------------------------------------
def a_run():
    rng = np.random.default_rng(0)
    psi = (rng.random((1, 6, 8)) + 1j * rng.random((1, 6, 8))).astype(np.complex64)
    probe = (rng.random((1, 2, 4, 4)) + 1j).astype(np.complex64)
    scan = rng.random((1, 5, 2)).astype(np.float32)
    return psi, probe, scan, [(0, 0.5, 0.25, 100.0), (1, 0.25, 0.125, 60.0)], None


def but(run, k, value):
    return run[:k] + (value,) + run[k + 1:]


def test_same_run_rejects_a_shape_a_bit_and_a_history():
    run = a_run()
    same_run(run, a_run())
    with pytest.raises(AssertionError):
        same_run(run, but(run, 0, run[0].reshape(1, 8, 6)))  # the same bytes
    moved = run[2].copy()
    moved[0, 3, 1] = np.nextafter(moved[0, 3, 1], np.float32(2))
    with pytest.raises(AssertionError):
        same_run(run, but(run, 2, moved))
    with pytest.raises(AssertionError):
        same_run(run, but(run, 3, [run[3][0], (1, 0.25, 0.125, np.nextafter(60.0, 61.0))]))
    with pytest.raises(AssertionError):
        same_run(run, but(run, 3, run[3][:1]))


# ---- the error norms and the tolerance rule -----------------------------------------------------------------------------------
def test_rel_errors_of_a_known_pair():
    want = np.array([3.0, 4.0j, 0.0, -10.0])
    got = np.array([3.0, 4.0j, 0.0, -10.0]) + np.array([0.0, 0.5, 0.0, 1.0j])
    e_max, e_l2 = rel_errors(got, want)
    assert e_max == 1.0 / 10.0
    assert e_l2 == pytest.approx(np.sqrt(1.25 / 125.0), rel=1e-15)
    assert rel_max(got, want) == e_max
    assert rel_errors(got.astype(np.complex64), want)[0] == e_max      # the difference is taken in complex128


def test_bound_has_three_regimes():
    floor, cap = 1e-6, 1e-4
    assert FACTOR == 4
    assert bound(0.0, floor, cap) == floor and bound(floor / FACTOR, floor, cap) == floor
    assert bound(5e-6, floor, cap) == FACTOR * 5e-6
    assert bound(cap / FACTOR, floor, cap) == cap and bound(1.0, floor, cap) == cap


# ---- horizon -----------------------------------------------------------------------------------------------------------------
def history(steps):
    return [(i, gpsi, gprb, 100.0 / (i + 1)) for i, (gpsi, gprb) in enumerate(steps)]


def test_horizon_ends_where_the_references_part_or_a_step_is_unresolved():
    resolved = [(0.5, 0.25), (0.25, 0.125), (0.125, 0.5), (0.5, 0.5)]
    double = history(resolved)
    assert horizon(history(resolved), double) == 4                                   # never
    parted = list(resolved)
    parted[2] = (0.125, 0.25)                                                        # another probe step at iteration 2
    assert horizon(history(parted), double) == 2
    small = UNRESOLVED_STEP / 2
    for k, step in ((1, (small, 0.125)), (3, (0.5, small))):                          # object step, probe step
        steps = list(resolved)
        steps[k] = step
        assert horizon(history(steps), history(steps)) == k
    steps = list(resolved)
    steps[1] = (0.0, UNRESOLVED_STEP)                  # a failed search (0) and a step at the threshold are resolved
    assert horizon(history(steps), history(steps)) == 4
    # the logged cost plays no part
    assert horizon([h[:3] + (h[3] * 2,) for h in double], double) == 4


# ---- assert_follows ----------------------------------------------------------------------------------------------------------
def test_assert_follows_passes_on_equal_input_and_at_its_bounds():
    run = a_run()
    assert_follows(run, a_run(), dsum=50.0, cost_rtol=1e-5, tol=5e-4, scan_tol=1e-2)
    # a cost just inside cost_rtol * (|cost| + dsum) = 1e-5 * (60 + 50)
    near = but(run, 3, [run[3][0], (1, 0.25, 0.125, 60.0 + 1.09e-3)])
    assert_follows(near, run, dsum=50.0, cost_rtol=1e-5, tol=5e-4)


def test_assert_follows_rejects_steps_costs_arrays_and_indices():
    run = a_run()
    kw = dict(dsum=50.0, cost_rtol=1e-5, tol=5e-4)
    with pytest.raises(AssertionError):                      # another probe step
        assert_follows(but(run, 3, [run[3][0], (1, 0.25, 0.25, 60.0)]), run, **kw)
    with pytest.raises(AssertionError):                      # a cost just outside 1e-5 * (60 + 50) = 1.1e-3
        assert_follows(but(run, 3, [run[3][0], (1, 0.25, 0.125, 60.0 + 1.11e-3)]), run, **kw)
    with pytest.raises(AssertionError):                      # without dsum the same cost is outside: the bound uses it
        assert_follows(but(run, 3, [run[3][0], (1, 0.25, 0.125, 60.0 + 1.09e-3)]), run, dsum=0.0, cost_rtol=1e-5, tol=5e-4)
    with pytest.raises(AssertionError):                      # a wrong iteration index
        assert_follows(but(run, 3, [run[3][0], (2, 0.25, 0.125, 60.0)]), run, **kw)
    for k in (0, 1):                                         # one element of the object, of the probe, just above tol
        off = run[k].copy()
        off.flat[3] += np.complex64(5.5e-4 * np.abs(run[k]).max())
        with pytest.raises(AssertionError):
            assert_follows(but(run, k, off), run, **kw)
        off = run[k].copy()
        off.flat[3] += np.complex64(4.5e-4 * np.abs(run[k]).max())
        assert_follows(but(run, k, off), run, **kw)          # and just below it
    moved = run[2].copy()
    moved[0, 2, 0] += 0.02
    assert_follows(but(run, 2, moved), run, **kw)            # positions are compared only where scan_tol is given
    with pytest.raises(AssertionError):
        assert_follows(but(run, 2, moved), run, scan_tol=1e-2, **kw)
