"""What every GPU test file (``tests/test_hip_*.py``) needs: the ``pt`` fixture, host <-> device copies, the two error
norms, the bitwise comparison of arrays, and the project's tolerance rule.  No top-level ``torch`` import, so that the
CPU tests can import it.

``conftest.py`` does not provide ``pt``: a test file takes it with ``from hip_common import pt  # noqa: F401`` (pytest
collects the fixtures it finds in the test module's namespace).

The tolerance rule: the device may be ``FACTOR`` times the error that the float32 restatement of the same arithmetic
has against the float64 reference, between a floor and a cap.  The factor is the project's; every floor and cap is tied
to one kernel's measured error and stays in that kernel's test file.  The operators (fwd / adj / adj_probe / fft2)
follow it through ``op_bounds`` / ``check_op``: the restatement is ``oracle.ptycho_oracle`` with ``"single"``, the floor
is ``OP_FLOOR`` and the caps are ``REL_MAX`` / ``REL_L2``; tests/test_operator_bounds_cpu.py shows that no tested case is
decided by a cap."""
import numpy as np
import pytest

FACTOR = 4         # the device against the float32 restatement's own error
# Caps of the operators' bounds (once the bounds themselves): no operator-against-oracle assertion may be looser than these,
# whatever the float32 restatement's error.  Device-against-device comparisons still use them directly.
REL_MAX = 2e-5     # cap, elementwise: relative to the largest element of the reference
REL_L2 = 3e-6      # cap, relative L2
OP_FLOOR = 2.0 ** -22   # FACTOR float32 roundings (2^-24 each): matters only where the restatement is almost exact


@pytest.fixture(scope="module")
def pt():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import libtike.hipfft as pt
    return pt


def dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x), device="cuda")


def host(t):
    return t.detach().cpu().numpy()


def crand(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def rel_errors(got, want):
    """``(rel_max, rel_l2)`` of ``got`` against ``want``: the largest elementwise error relative to the largest element
    of ``want``, and the relative L2 error; the difference is taken in complex128."""
    d = np.abs(got.astype(np.complex128) - want)
    return d.max() / np.abs(want).max(), np.sqrt((d ** 2).sum() / (np.abs(want) ** 2).sum())


def rel_max(got, want):
    return rel_errors(got, want)[0]


def same_bits(a, b):
    """Equal shape, equal dtype, equal bytes: 0.0 and -0.0 differ, NaNs of one payload are equal."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def bound(e32, floor, cap):
    """The tolerance rule for a float32 restatement's error ``e32``."""
    return min(cap, max(FACTOR * e32, floor))


def op_bounds(want64, want32):
    """``(bound_max, bound_l2)`` of an operator output: the rule on the errors that the float32 oracle ``want32`` has
    against the float64 oracle ``want64``.  A reference that is zero everywhere (every position skipped) has no relative
    error: the bounds are the floor, and ``check_op`` asks for exact zeros."""
    e32 = rel_errors(want32, want64) if np.any(want64) else (0.0, 0.0)
    return bound(e32[0], OP_FLOOR, REL_MAX), bound(e32[1], OP_FLOOR, REL_L2)


def check_op(got, want64, want32, what):
    """A device result against the float64 oracle, held to ``op_bounds`` (strictly below, as the fixed bounds were);
    prints one line whatever the outcome.  Returns ``(device errors, e32, bounds)``."""
    bmax, bl2 = op_bounds(want64, want32)
    assert got.shape == want64.shape == want32.shape, (what, got.shape, want64.shape, want32.shape)
    if not np.any(want64):
        e32 = (0.0, 0.0)
        e = (float(np.abs(got).max()),) * 2        # absolute: must be exactly zero
        ok = not np.any(got)
    else:
        e32 = rel_errors(want32, want64)
        e = rel_errors(got, want64)
        ok = bool(e[0] < bmax and e[1] < bl2)
    print("check_op %s: device max %.3g l2 %.3g | float32 oracle max %.3g l2 %.3g | bound max %.3g l2 %.3g%s"
          % (what, e[0], e[1], e32[0], e32[1], bmax, bl2, "" if ok else "  <-- FAILS"))
    assert ok, (what, "device", e, "float32 oracle", e32, "bound", (bmax, bl2))
    return e, e32, (bmax, bl2)
