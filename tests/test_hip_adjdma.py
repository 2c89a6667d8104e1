"""Split adjoints at ndet = 256 after the inter-step twiddle moved into the row pass and the object adjoint's tiles stream
through an LDS ring filled by LDS-DMA (``k_rows_split<256, +1>``, ``k_cols_adjreg<256, split>``, the split probe adjoint
of ``k_cols_gatherwin``), against the CPU oracle in double through ``check_op`` of ``tests/hip_common.py`` (FACTOR x the
float32 oracle's own error).

The edges are those of the ring: a skipped position requests nothing and waits for nothing (first, last and two
consecutive middle positions of a run); runs of one and of three positions; a launch that starts at ``k_begin`` != 0
(``set_chunk``); a first strip that starts inside the padding (nprb < ndet); two inputs in succession on one handle.  256
positions at 256^2 give runs of 16 (14 with the 14 strips of nprb = 200); a handful of positions give runs of one.  The
deterministic option must be bitwise reproducible on every case.  ``pytest -m gpu``.
"""
import functools

import numpy as np
import pytest

from oracle import ptycho_oracle as op
from hip_common import REL_MAX, check_op, host, pt, rel_max  # noqa: F401

pytestmark = pytest.mark.gpu


def dev(x):
    import torch
    return torch.as_tensor(np.array(x), device="cuda")   # a copy: the shared case arrays are read-only


def scan_of(name):
    """(nprb, nz, n, scan[ntheta, nscan, 2])"""
    rng = np.random.default_rng({"skips": 11, "three": 12, "one": 13, "slide": 14, "small_probe": 15}[name])
    if name == "skips":
        # one position per angle: the sorted order is the angle order, so a skipped position (negative coordinate,
        # kernels.cu:39) sits INSIDE its run of 16 (with several positions per angle they are sorted behind the valid ones)
        rows = 3.0 + 9.0 * rng.random(256)
        cols = 2.0 + 9.0 * rng.random(256)
        rows[[0, 7, 8, 15]] = -1.5              # run 0: first, two consecutive middle, last
        cols[[16, 40, 41, 42, 63]] = -0.25      # run 1: first; run 2: three in a row; run 3: last
        rows[64:80] = -3.0                      # run 4: nothing but skipped positions
        return 256, 272, 272, np.stack([rows, cols], -1)[:, None]
    if name == "three":
        return 256, 300, 288, np.array([[[20.25, 9.5], [3.0, 8.75], [11.5, 10.0]]])
    if name == "one":
        return 256, 300, 288, np.array([[[5.5, 7.25]]])
    if name == "slide":      # one angle, the window slides by 8 rows per position; columns cross bucket boundaries
        rows = 8.0 * np.arange(256) + rng.random(256)
        cols = 4.0 + 12.0 * rng.random(256)
        return 256, int(rows.max()) + 300, 288, np.stack([rows, cols], -1)[None]
    if name == "small_probe":   # nprb = 200: pad = 28, the first strip (columns 16 .. 31) starts inside the padding
        rows = 10.0 * np.arange(256) + rng.random(256)
        cols = 6.0 + 7.0 * rng.random(256)
        return 200, int(rows.max()) + 230, 240, np.stack([rows, cols], -1)[None]
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def case(name):
    """The problem and its oracle adjoint (float64, and the float32 restatement that sets the bound), computed once and
    shared (read-only) by the tests that use it."""
    nprb, nz, n, scan = scan_of(name)
    rng = np.random.default_rng(99)
    scan = scan.astype(np.float32)
    ntheta, nscan = scan.shape[:2]
    yy, xx = np.mgrid[:nprb, :nprb] - (nprb - 1) / 2
    amp = np.exp(-(yy ** 2 + xx ** 2) / (2 * (nprb / 3.0) ** 2))
    # one probe for all angles of "skips" (256 angles): broadcast, 256 random phase screens would only cost memory
    phase = np.exp(2j * np.pi * rng.random((1 if ntheta > 8 else ntheta, nprb, nprb)))
    probe = np.ascontiguousarray(np.broadcast_to((amp * phase).astype(np.complex64), (ntheta, nprb, nprb)))
    y = (rng.standard_normal((ntheta, nscan, 256, 256)) + 1j * rng.standard_normal((ntheta, nscan, 256, 256))).astype(np.complex64)
    want, want32 = op.adj(y, scan, probe, nz, n, "double"), op.adj(y, scan, probe, nz, n, "single")
    for a in (scan, probe, y, want, want32):
        a.setflags(write=False)
    return dict(nprb=nprb, ntheta=ntheta, nz=nz, n=n, nscan=nscan, scan=scan, probe=probe, y=y, want=(want, want32))


@functools.lru_cache(maxsize=None)
def second_input(name):
    """Another farplane for the problem of ``case(name)`` and its oracle adjoints ``(float64, float32)``."""
    c = case(name)
    rng = np.random.default_rng(1234)
    y = (rng.standard_normal(c["y"].shape) + 1j * rng.standard_normal(c["y"].shape)).astype(np.complex64)
    want = tuple(op.adj(y, c["scan"], c["probe"], c["nz"], c["n"], precision) for precision in ("double", "single"))
    for a in (y,) + want:
        a.setflags(write=False)
    return y, want


@functools.lru_cache(maxsize=None)
def probe_case(name):
    """An object for the problem of ``case(name)`` and the oracle probe adjoints ``(float64, float32)`` of its farplane."""
    c = case(name)
    rng = np.random.default_rng(77)
    psi = (rng.standard_normal((c["ntheta"], c["nz"], c["n"])) + 1j * rng.standard_normal((c["ntheta"], c["nz"], c["n"]))).astype(np.complex64)
    want = tuple(op.adj_probe(c["y"], c["scan"], psi, c["nprb"], precision) for precision in ("double", "single"))
    for a in (psi,) + want:
        a.setflags(write=False)
    return psi, want


def solver(pt, c):
    return pt.PtychoCuFFT(c["nscan"], c["nprb"], 256, c["ntheta"], c["nz"], c["n"])


def check_adj(slv, c, y, want, tag):
    """Float atomics against the oracle ``want = (float64, float32)``, then the deterministic option: against the oracle
    and bitwise twice."""
    yd, scan, prb = dev(y), dev(c["scan"]), dev(c["probe"])
    slv.set_deterministic(False)
    got = host(slv.adj(yd, scan, prb))
    check_op(got, want[0], want[1], "adjdma %s float atomics" % tag)
    slv.set_deterministic(True)
    a1 = host(slv.adj(yd, scan, prb))
    a2 = host(slv.adj(yd, scan, prb))
    check_op(a1, want[0], want[1], "adjdma %s deterministic" % tag)
    assert np.array_equal(a1.view(np.uint32), a2.view(np.uint32)), (tag, "deterministic option: two runs differ")
    return a1


@pytest.mark.parametrize("split", [True, False])
def test_skipped_first_last_and_two_middle_positions_of_a_run(pt, split):
    c = case("skips")
    rows, cols = c["scan"][:16, 0, 0], c["scan"][:16, 0, 1]
    assert list(np.flatnonzero((rows < 0) | (cols < 0))) == [0, 7, 8, 15]
    with solver(pt, c) as slv:
        slv.set_split(split)
        check_adj(slv, c, c["y"], c["want"], "skips split=%s" % split)


@pytest.mark.parametrize("name", ["three", "one"])
def test_runs_of_three_and_of_one_position(pt, name):
    c = case(name)
    with solver(pt, c) as slv:
        check_adj(slv, c, c["y"], c["want"], name)


def test_chunk_smaller_than_nscan(pt):
    """40 positions per launch pair: the column launches start at k_begin = 40, 80, ... and read scratch tile k - k_begin."""
    c = case("slide")
    with solver(pt, c) as slv:
        slv.set_chunk(40)
        check_adj(slv, c, c["y"], c["want"], "slide chunk 40")


def test_two_inputs_in_succession_on_one_handle(pt):
    c = case("slide")
    y2, want2 = second_input("slide")
    with solver(pt, c) as slv:
        check_adj(slv, c, c["y"], c["want"], "slide first input")
        check_adj(slv, c, y2, want2, "slide second input")
        check_adj(slv, c, c["y"], c["want"], "slide first input again")


def test_small_probe_split_and_unsplit(pt):
    """nprb < ndet: adj and adj_probe, split and un-split, each against the oracle and the two against each other.
    Both are float32 evaluations within REL_MAX (the cap of the rule) of the exact result, so they differ by less than
    2 REL_MAX."""
    c = case("small_probe")
    psi, want_prb = probe_case("small_probe")
    obj, prb = {}, {}
    with solver(pt, c) as slv:
        for split in (True, False):
            slv.set_split(split)
            obj[split] = check_adj(slv, c, c["y"], c["want"], "small_probe split=%s" % split)
            yd, scan, psid = dev(c["y"]), dev(c["scan"]), dev(psi)
            slv.set_deterministic(False)
            check_op(host(slv.adj_probe(yd, scan, psid)), want_prb[0], want_prb[1],
                     "adjdma small_probe adj_probe split=%s float atomics" % split)
            slv.set_deterministic(True)
            p1 = host(slv.adj_probe(yd, scan, psid))
            p2 = host(slv.adj_probe(yd, scan, psid))
            check_op(p1, want_prb[0], want_prb[1], "adjdma small_probe adj_probe split=%s deterministic" % split)
            assert np.array_equal(p1.view(np.uint32), p2.view(np.uint32)), "adj_probe, deterministic option: two runs differ"
            prb[split] = p1
    e_obj = rel_max(obj[True], obj[False].astype(np.complex128))
    e_prb = rel_max(prb[True], prb[False].astype(np.complex128))
    print("small_probe split against un-split: adj", e_obj, "adj_probe", e_prb)
    assert e_obj < 2 * REL_MAX and e_prb < 2 * REL_MAX, (e_obj, e_prb)
