"""Object adjoint with the overlap-add window in registers (``k_cols_adjreg``, ndet = 256 and 512) against the CPU oracle.

The shapes are the smallest at which the launcher still gives runs of 16 sorted positions (positions x strips / CUs >=
16: 256 positions at 256, 128 at 512); the scans are built so that the window's slots wrap, several row groups retire
per position, every column offset inside a bucket occurs and runs re-anchor.  The tolerance is ``check_op`` of
``tests/hip_common.py`` (FACTOR x the float32 oracle's own error); the deterministic option must also be bitwise
reproducible.  ``pytest -m gpu``.
"""
import functools

import numpy as np
import pytest

from oracle import ptycho_oracle as op
from hip_common import check_op, host, pt  # noqa: F401

pytestmark = pytest.mark.gpu

GAPS = (0, 1, 23, 24, 25, 47, 48, 287, 288, 289, 600)   # around RPG = 24, 2 RPG and the window height 288


def dev(x):
    import torch
    return torch.as_tensor(np.array(x), device="cuda")   # a copy: the shared case arrays are read-only


def scan_of(name):
    """(ndet, nprb, ntheta, nz, n, scan[ntheta, nscan, 2])"""
    rng = np.random.default_rng({"step32": 1, "step8": 2, "gaps": 3, "angles": 4, "n512": 5}[name])
    if name == "step32":     # ONE 4-px column bucket, a run of 16 travels 512 rows > 288: slots wrap, > 1 group per position
        rows = 32.0 * np.arange(256) + rng.integers(0, 4, 256) + rng.random(256)
        cols = 8.0 + 3.99 * rng.random(256)
        return 256, 256, 1, int(rows.max()) + 300, 288, np.stack([rows, cols], -1)[None]
    if name == "step8":      # a group retires every third position; columns cross bucket boundaries
        rows = 8.0 * np.arange(256) + rng.random(256)
        cols = 4.0 + 12.0 * rng.random(256)
        return 256, 256, 1, int(rows.max()) + 300, 288, np.stack([rows, cols], -1)[None]
    if name == "gaps":
        p = np.array([1.0] * 7 + [0.25] * 4)
        gaps = rng.choice(GAPS, size=256, p=p / p.sum())
        gaps[:11] = GAPS                                   # every gap at least once
        rows = np.cumsum(gaps).astype(np.float64)
        frac = rng.random(256)
        frac[::5] = 0.0                                    # fractional part exactly 0
        rows += frac
        cols = 8.0 + np.where(np.arange(256) % 7 == 0, 0.0, 3.99 * rng.random(256))
        nz, n = int(rows.max()) + 120, 288                 # the last positions hang over the bottom edge
        cols[40:48] = n - 130.0 + rng.random(8)            # taps fall off the right edge
        rows[[5, 77, 200]] = -1.5                          # skipped (kernels.cu:39)
        cols[[130]] = -2.25
        return 256, 256, 1, nz, n, np.stack([rows, cols], -1)[None]
    if name == "angles":     # nprb < ndet; 152 positions per angle: the angle changes inside a run of 16
        rows = np.tile(12.0 * np.arange(152), (2, 1)) + rng.random((2, 152))
        cols = 6.0 + 7.0 * rng.random((2, 152))
        return 256, 200, 2, int(rows.max()) + 230, 240, np.stack([rows, cols], -1)
    if name == "n512":
        rows = 40.0 * np.arange(128) + rng.random(128)
        cols = 4.0 + 7.0 * rng.random(128)
        return 512, 512, 1, int(rows.max()) + 560, 540, np.stack([rows, cols], -1)[None]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """The problem and its oracle adjoint (float64, and the float32 restatement that sets the bound), computed once and
    shared (read-only) by the tests that use it."""
    ndet, nprb, ntheta, nz, n, scan = scan_of(name)
    rng = np.random.default_rng(99)
    scan = scan.astype(np.float32)
    nscan = scan.shape[1]
    yy, xx = np.mgrid[:nprb, :nprb] - (nprb - 1) / 2
    amp = np.exp(-(yy ** 2 + xx ** 2) / (2 * (nprb / 3.0) ** 2))
    probe = (amp * np.exp(2j * np.pi * rng.random((ntheta, nprb, nprb)))).astype(np.complex64)
    y = (rng.standard_normal((ntheta, nscan, ndet, ndet)) + 1j * rng.standard_normal((ntheta, nscan, ndet, ndet))).astype(np.complex64)
    want, want32 = op.adj(y, scan, probe, nz, n, "double"), op.adj(y, scan, probe, nz, n, "single")
    for a in (scan, probe, y, want, want32):
        a.setflags(write=False)
    return dict(ndet=ndet, nprb=nprb, ntheta=ntheta, nz=nz, n=n, nscan=nscan, scan=scan, probe=probe, y=y, want=want,
                want32=want32)


def check_adj(pt, name, split=True):
    c = case(name)
    with pt.PtychoCuFFT(c["nscan"], c["nprb"], c["ndet"], c["ntheta"], c["nz"], c["n"]) as slv:
        slv.set_split(split)
        y, scan, prb = dev(c["y"]), dev(c["scan"]), dev(c["probe"])
        tag = "adjreg %s %s " % (name, "split" if split else "unsplit")
        check_op(host(slv.adj(y, scan, prb)), c["want"], c["want32"], tag + "float atomics")
        slv.set_deterministic(True)
        a1 = host(slv.adj(y, scan, prb))
        a2 = host(slv.adj(y, scan, prb))
        check_op(a1, c["want"], c["want32"], tag + "deterministic")
        assert np.array_equal(a1.view(np.uint32), a2.view(np.uint32)), "deterministic option: two runs differ"


@pytest.mark.parametrize("split", [True, False])
def test_rows_step_32_one_bucket(pt, split):
    check_adj(pt, "step32", split)


def test_rows_step_8_columns_cross_buckets(pt):
    check_adj(pt, "step8")


def test_row_gaps_around_group_and_window_height(pt):
    c = case("gaps")
    assert (c["scan"][0, :, 0] < 0).sum() == 3 and (c["scan"][0, :, 0] + c["nprb"] + 1 > c["nz"]).any()
    check_adj(pt, "gaps")


def test_small_probe_two_angles(pt):
    check_adj(pt, "angles")


def test_ndet_512(pt):
    check_adj(pt, "n512")


def test_adjoint_identity(pt):
    """<fwd x, y> = <x, adj y> to 1e-5 (the bound of tests/test_hip_operators.py), sums in float64, on the first case."""
    import torch
    c = case("step32")
    rng = np.random.default_rng(7)
    x = (rng.standard_normal((1, c["nz"], c["n"])) + 1j * rng.standard_normal((1, c["nz"], c["n"]))).astype(np.complex64)
    with pt.PtychoCuFFT(c["nscan"], c["nprb"], c["ndet"], 1, c["nz"], c["n"]) as slv:
        psi, y, scan, prb = dev(x), dev(c["y"]), dev(c["scan"]), dev(c["probe"])
        lhs = complex(torch.sum(slv.fwd(psi, scan, prb).to(torch.complex128) * y.conj().to(torch.complex128)))
        rhs = complex(torch.sum(psi.to(torch.complex128) * slv.adj(y, scan, prb).conj().to(torch.complex128)))
    print("identity residual", abs(lhs - rhs) / abs(lhs))
    assert abs(lhs - rhs) / abs(lhs) < 1e-5
