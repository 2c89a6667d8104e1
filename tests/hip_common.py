"""What every GPU test file (``tests/test_hip_*.py``) needs: the ``pt`` fixture, host <-> device copies, the two error
norms, the bitwise comparison of arrays, and the project's tolerance rule.  No top-level ``torch`` import, so that the
CPU tests can import it.

``conftest.py`` does not provide ``pt``: a test file takes it with ``from hip_common import pt  # noqa: F401`` (pytest
collects the fixtures it finds in the test module's namespace).

The tolerance rule: the device may be ``FACTOR`` times the error that the float32 restatement of the same arithmetic
has against the float64 reference, between a floor and a cap.  The factor is the project's; every floor and cap is tied
to one kernel's measured error and stays in that kernel's test file."""
import numpy as np
import pytest

FACTOR = 4         # the device against the float32 restatement's own error
REL_MAX = 2e-5     # operators: elementwise, relative to the largest element of the reference
REL_L2 = 3e-6      # operators: relative L2


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
