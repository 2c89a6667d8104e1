"""The geometries and inputs of the operator tests (tests/test_hip_operators.py), without torch and without the native
library, so that tests/test_operator_bounds_cpu.py can evaluate the float32 oracle on exactly the inputs the GPU tests use.

``libtike.hipfft.synthetic`` is plain NumPy, but importing it as a module of its package runs ``libtike/hipfft/__init__.py``,
which loads torch and ``libptychohip.so``.  It is therefore loaded here from its file, under a private name: the same
generators, no package import.  Expected values never come from here: ``oracles`` only calls ``oracle.ptycho_oracle``.
"""
import importlib.util
import os

import numpy as np

from oracle import ptycho_oracle as op

from hip_common import crand

_SYN = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                    "libtike-cufft_amd", "libtike", "hipfft", "synthetic.py")
_spec = importlib.util.spec_from_file_location("_operator_cases_synthetic", _SYN)
syn = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(syn)


def problem(ndet, nprb, ny, nx, step, ntheta=1, seed=11, hard=True):
    p = syn.make_problem(ny, nx, step, nprb, ndet, ntheta=ntheta, seed=seed)
    rng = np.random.default_rng(seed + 1)
    p["probe"] = (p["probe"] * np.exp(2j * np.pi * rng.random(p["probe"].shape))).astype(np.complex64)
    if hard and p["nscan"] >= 4:
        p["scan"][0, 1] = [-1.5, 2.25]                       # skipped (kernels.cu:39)
        p["scan"][0, 2] = [-0.25, 1.5]                       # trunc -> -0.0, not skipped
        p["scan"][-1, 3] = [p["nz"] - nprb / 2, 3.75]        # hangs over the bottom edge
        p["scan"][0, 0] = [2.0, 5.0]                         # exactly integer
    return p


def oracles(psi, scan, prb, y, ndet, precision):
    """``[fwd, adj, adj_probe]`` of the oracle in ``precision`` ("double": the reference; "single": its float32 restatement)."""
    nz, n, nprb = psi.shape[1], psi.shape[2], prb.shape[-1]
    return [op.fwd(psi, scan, prb, ndet, precision), op.adj(y, scan, prb, nz, n, precision),
            op.adj_probe(y, scan, psi, nprb, precision)]


def fft2_oracles(x):
    """``(forward, inverse)`` unnormalised transforms of the tiles ``x``: ``np.fft`` in complex128, and the complex64
    transform the oracle uses (pocketfft keeps complex64)."""
    x64 = x.astype(np.complex128)
    nn = x.shape[-1] * x.shape[-2]
    return (np.fft.fft2(x64), np.fft.ifft2(x64) * nn), (op.fft2_unnorm(x), op.ifft2_unnorm(x))


CASES = [
    # ndet, nprb, ny, nx, step, ntheta
    (16, 16, 3, 3, 5, 1),
    (16, 12, 3, 3, 5, 2),
    (32, 32, 3, 4, 6, 1),
    (32, 21, 2, 3, 6, 1),
    (64, 64, 4, 4, 9, 2),
    (64, 40, 3, 3, 9, 1),
    (128, 128, 4, 5, 11, 1),
    (128, 100, 3, 3, 11, 1),
    # sizes with an odd prime factor and a Stockham plan of their own (radix 3 / 5 / 7 first, fft_core.hpp)
    (48, 48, 3, 4, 7, 1),
    (48, 30, 3, 3, 7, 2),
    (80, 80, 3, 3, 9, 1),
    (80, 55, 2, 3, 9, 1),
    (96, 96, 3, 4, 9, 2),
    (96, 70, 3, 3, 9, 1),
    (112, 112, 3, 4, 11, 1),
    (112, 75, 3, 3, 11, 2),
    (192, 192, 2, 3, 13, 1),
    (192, 130, 2, 2, 13, 2),
    (256, 256, 3, 4, 13, 1),
    (256, 128, 2, 3, 13, 2),
    (512, 512, 2, 2, 17, 1),
    (512, 300, 2, 2, 17, 1),
    (1024, 1024, 1, 2, 17, 1),
    (2048, 2048, 1, 2, 19, 1),
    (2048, 1500, 1, 2, 19, 1),
]


def case_inputs(ndet, nprb, ny, nx, step, ntheta):
    """``(p, y)`` of test_fwd_adj_adjprobe_match_oracle: the problem and the random farplane of the adjoints."""
    p = problem(ndet, nprb, ny, nx, step, ntheta)
    rng = np.random.default_rng(2)
    return p, crand(rng, (ntheta, p["nscan"], ndet, ndet))


EDGE_CASES = ["one_position", "all_skipped", "one_pixel_probe", "flush_against_edges", "far_outside"]


def edge_case(case):
    """``dict(ndet, nprb, nz, n, nscan, scan, psi, prb, y)`` of test_edge_cases."""
    rng = np.random.default_rng(3)
    ndet, nprb, nz, n, nscan = 16, 16, 40, 44, 3
    scan = np.array([[[3.25, 4.5], [10.0, 20.75], [17.5, 1.125]]], np.float32)
    if case == "one_position":
        nscan, scan = 1, scan[:, :1]
    elif case == "all_skipped":
        scan = -scan - 1.0
    elif case == "one_pixel_probe":
        nprb = 1
    elif case == "flush_against_edges":      # trunc(pos) + nprb + 1 == size exactly, and pos = 0
        scan = np.array([[[nz - nprb - 1.0, n - nprb - 1.0], [0.0, 0.0], [nz - nprb - 0.5, 0.25]]], np.float32)
    elif case == "far_outside":              # beyond the object: every tap reads zero / is dropped
        scan = np.array([[[1000.0, 3.0], [3.0, 5000.5], [2.0, 2.0]]], np.float32)
    else:
        raise KeyError(case)
    psi = crand(rng, (1, nz, n))
    prb = crand(rng, (1, nprb, nprb))
    y = crand(rng, (1, nscan, ndet, ndet))
    return dict(ndet=ndet, nprb=nprb, nz=nz, n=n, nscan=nscan, scan=scan, psi=psi, prb=prb, y=y)


# ---- fft2 ------------------------------------------------------------------------------------------------------------
STOCKHAM = (16, 32, 48, 64, 80, 96, 112, 128, 192, 256, 512, 1024, 2048)      # sizes with a plan of their own (fft_core.hpp)
FFT2_CASES = [(n, 3, True) for n in STOCKHAM] + [(n, 3, False) for n in STOCKHAM if n <= 128] + \
             [(64, 1100, True), (16, 37, True), (112, 600, True)]             # ndet, tiles, option tile
FFT2_ANY_SIZES = [12, 30, 48, 80, 96, 100, 112, 192, 200, 1000]               # 48 ... 192: own plans; the others: Bluestein


def fft2_inputs():
    """``(ndet, nb, tile, x)`` of test_fft2_matches_numpy, in its order: one generator feeds every case."""
    rng = np.random.default_rng(0)
    for ndet, nb, tile in FFT2_CASES:
        yield ndet, nb, tile, crand(rng, (nb, ndet, ndet))


def fft2_any_size_input(ndet):
    rng = np.random.default_rng(ndet)
    return crand(rng, (3 if ndet < 500 else 2, ndet, ndet))


# ---- the new geometries --------------------------------------------------------------------------------------------------
UNALIGNED = [(16, 16, 1), (64, 64, 1), (64, 27, 2), (112, 75, 1), (128, 128, 1), (256, 256, 1)]      # ndet, nprb, ntheta


def unaligned_inputs(ndet, nprb, ntheta):
    """3 x 4 positions for the calls on a far plane that is 8 but not 16 bytes aligned."""
    p = problem(ndet, nprb, 3, 4, 5, ntheta, seed=21)
    rng = np.random.default_rng(22)
    return p, crand(rng, (ntheta, 12, ndet, ndet))


def impulses(N):
    return [(0, 0), (0, 1), (1, 0), (N - 1, N - 1), (N // 2, 1), (3, N - 5)]      # (row, column)


def impulse_tiles(N):
    """Six tiles with a single 1.0 each, and their exact transforms ``exp(-/+ 2 pi i (r ky + c kx) / N)`` in complex128
    (the phase reduced modulo N in integers, so the argument of exp is exact to one rounding)."""
    x = np.zeros((6, N, N), np.complex64)
    k = np.arange(N)
    fwd = np.empty((6, N, N), np.complex128)
    for i, (r, c) in enumerate(impulses(N)):
        x[i, r, c] = 1.0
        fwd[i] = np.exp(-2j * np.pi * ((r * k[:, None] + c * k[None, :]) % N) / N)
    return x, fwd, np.conj(fwd)


CANCEL_SIZES = [64, 112, 256, 100]


def cancel_inputs(ndet):
    """psi = 1, probe = 1, nprb = ndet, 2 x 2 integer positions: the far plane is ndet in bin (0, 0), zero elsewhere."""
    nz = n = ndet + 8
    scan = np.array([[[0.0, 0.0], [0.0, 7.0], [6.0, 1.0], [7.0, 7.0]]], np.float32)
    return dict(ndet=ndet, nprb=ndet, nz=nz, n=n, nscan=4, scan=scan, psi=np.ones((1, nz, n), np.complex64),
                prb=np.ones((1, ndet, ndet), np.complex64))


WEIGHT_EDGES = [(32, 21), (256, 128)]         # ndet, nprb
TINY, NEARLY_ONE = 2.0 ** -20, 1.0 - 2.0 ** -24


def weight_edge_inputs(ndet, nprb):
    """8 positions whose bilinear fractions sit at the edges of float32: 2^-20 (weight of the second tap far below one
    ulp of the first tap's product), 1 - 2^-24 (the largest float32 below 1; the first tap's weight is 2^-24), 0.5 and
    exactly 0, paired over rows and columns; the last position puts the second tap of the last probe row and column on the
    last object row and column.  ``1 - 2^-24`` plus an integer >= 1 rounds up in float32, so those fractions sit at
    integer part 0; ``want_int`` are the intended integer parts, to be checked against ``split_positions``."""
    nz, n = nprb + 12, nprb + 14
    frac = [(TINY, NEARLY_ONE), (NEARLY_ONE, TINY), (0.5, TINY), (TINY, 0.5), (NEARLY_ONE, NEARLY_ONE), (0.0, NEARLY_ONE),
            (TINY, 0.0)]
    ints = [(5, 0), (0, 9), (3, 4), (7, 2), (0, 0), (11, 0), (2, 13)]
    scan = np.zeros((1, 8, 2), np.float32)
    for k, ((fy, fx), (iy, ix)) in enumerate(zip(frac, ints)):
        scan[0, k] = [np.float32(iy) + np.float32(fy), np.float32(ix) + np.float32(fx)]
    scan[0, 7] = [nz - nprb - 1 + 0.5, n - nprb - 1 + TINY]          # rows sy .. sy + nprb end on nz - 1, columns on n - 1
    want_int = np.array(ints + [(nz - nprb - 1, n - nprb - 1)], np.int64)[None]
    want_frac = np.array(frac + [(0.5, TINY)], np.float64)[None]
    rng = np.random.default_rng(31)
    psi, prb, y = crand(rng, (1, nz, n)), crand(rng, (1, nprb, nprb)), crand(rng, (1, 8, ndet, ndet))
    return dict(ndet=ndet, nprb=nprb, nz=nz, n=n, nscan=8, scan=scan, psi=psi, prb=prb, y=y, want_int=want_int, want_frac=want_frac)
