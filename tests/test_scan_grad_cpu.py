"""The scan-position gradient without a GPU: the formula of ``ptycho_adj_scan`` against central differences of the float64
oracle and against autograd of the oracle restated in torch, the index logic of csrc/k_scangrad.hpp walked on the host,
the C ABI's argument checks and the header's text."""
import os
import re

import numpy as np
import pytest

import host_build
import scan_grad_ref as sg
from oracle import ptycho_oracle as op

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def small_problem(seed=3, ptheta=2, nscan=9, nz=29, n=35, nprb=12, ndet=16):
    rng = np.random.default_rng(seed)
    psi = sg.crand(rng, (ptheta, nz, n))
    probe = sg.crand(rng, (ptheta, nprb, nprb))
    g = sg.crand(rng, (ptheta, nscan, ndet, ndet))
    # fractions that are multiples of 1 / 64, never 0: with h = 2^-8 both points of a central difference stay in the cell
    whole = rng.integers(0, [nz - nprb - 1, n - nprb - 1], (ptheta, nscan, 2))
    frac = rng.integers(1, 64, (ptheta, nscan, 2)) / 64.0
    scan = (whole + frac).astype(np.float32)
    scan[0, 0] = (-19.0 / 64.0, 4.5)                    # valid, negative fraction: trunc = -0
    scan[0, 1] = (nz - 5 + 0.25, n - 7 + 0.75)          # overhangs the bottom and right edges
    scan[1, 0] = (2.5, -1.5)                            # skipped
    return psi, scan, probe, g, ndet


def test_formula_matches_central_differences_of_the_oracle():
    """``fwd`` is linear in the fraction inside a cell, so the central difference of ``Re <g, fwd>`` is its derivative up
    to rounding: the two agree to 1e-9 of the largest gradient (the difference quotient divides float64 noise of a sum of
    ndet^2 terms by 2 h = 2^-7)."""
    psi, scan, probe, g, ndet = small_problem()
    want = sg.adj_scan_ref(g, scan, psi, probe, "double")
    h = 2.0 ** -8
    got = np.zeros_like(want)
    g128 = g.astype(np.complex128)
    for k in range(2):
        step = np.zeros(2, dtype=np.float32)
        step[k] = h
        plus = op.fwd(psi, scan + step, probe, ndet, "double")
        minus = op.fwd(psi, scan - step, probe, ndet, "double")
        assert np.array_equal(np.trunc(scan + step), np.trunc(scan)) and np.array_equal(np.trunc(scan - step), np.trunc(scan))
        got[..., k] = (np.conj(g128) * (plus - minus)).real.sum(axis=(-2, -1)) / (2 * h)
    assert np.all(want[1, 0] == 0) and np.all(got[1, 0] == 0)          # the skipped position
    assert np.abs(want[0, 0]).min() > 0 and np.abs(want[0, 1]).min() > 0
    err = np.abs(got - want).max() / np.abs(want).max()
    print("central difference against the formula: %.3g" % err)
    assert err < 1e-9, err


def test_formula_at_an_integer_coordinate_is_the_derivative_of_the_truncated_cell():
    """At an exact integer the formula is the one-sided derivative towards larger coordinates (the cell trunc selects)."""
    psi, scan, probe, g, ndet = small_problem(seed=4)
    scan[:, :, 0] = np.trunc(scan[:, :, 0])
    scan[0, 0, 0] = 0.0
    scan[1, 0] = (2.0, -1.5)
    want = sg.adj_scan_ref(g, scan, psi, probe, "double")[..., 0]
    h = np.float32(2.0 ** -8)
    step = np.array([h, 0], dtype=np.float32)
    d = op.fwd(psi, scan + step, probe, ndet, "double") - op.fwd(psi, scan, probe, ndet, "double")
    got = (np.conj(g.astype(np.complex128)) * d).real.sum(axis=(-2, -1)) / h
    assert np.abs(got - want).max() < 1e-9 * np.abs(want).max()


@pytest.mark.parametrize("precision,tol", [("double", 1e-12), ("single", 2e-5)])
def test_formula_matches_autograd_of_the_restated_fwd(precision, tol):
    """``Re <g, fwd_torch>`` differentiated by torch: ``scan.grad`` is the formula, ``psi.grad`` the oracle's ``adj`` and
    ``probe.grad`` its ``adj_probe``; and ``fwd_torch`` is the oracle's ``fwd``."""
    import torch
    psi, scan, probe, g, ndet = small_problem(seed=5)
    gt = torch.tensor(g.astype(np.complex128 if precision == "double" else np.complex64))
    value = []

    def loss_of(farplane):
        value.append(farplane.detach().numpy())
        return (torch.conj(gt) * farplane).real.sum()
    gpsi, gscan, gprobe = sg.torch_grads(loss_of, psi, scan, probe, ndet, precision)
    rel = lambda a, b: np.abs(a - b).max() / np.abs(b).max()
    assert rel(value[0], op.fwd(psi, scan, probe, ndet, "double")) < tol
    assert rel(gscan, sg.adj_scan_ref(g, scan, psi, probe, "double")) < tol
    assert rel(gpsi, op.adj(g, scan, probe, psi.shape[1], psi.shape[2], "double")) < tol
    assert rel(gprobe, op.adj_probe(g, scan, psi, probe.shape[-1], "double")) < tol
    assert np.all(gscan[1, 0] == 0)


def test_float32_formula_is_close_to_the_float64_formula():
    """The float32 restatement (the source of the GPU test's bounds) differs from float64 by float32 rounding only."""
    psi, scan, probe, g, ndet = small_problem(seed=6)
    w64 = sg.adj_scan_ref(g, scan, psi, probe, "double")
    w32 = sg.adj_scan_ref(g, scan, psi, probe, "single")
    assert w32.dtype == np.float32 and w64.dtype == np.float64
    e = np.abs(w32 - w64).max() / np.abs(w64).max()
    assert 0 < e < 1e-5, e


def test_every_gpu_case_holds_the_five_kinds_of_position():
    for ndet, nprb, nscan, ptheta in sg.GRAD_CASES:
        c = sg.grad_case(ndet, nprb, nscan, ptheta)
        flat = c["scan"].reshape(-1, 2)
        ip, fr, valid = op.split_positions(flat[None], "single")
        s = c["special"]
        assert np.all(fr[0, s["integer"]] == 0) and valid[0, s["integer"]]
        assert valid[0, s["negative_fraction"]] and fr[0, s["negative_fraction"], 0] < 0
        assert not valid[0, s["skipped"]]
        oy, ox = ip[0, s["overhang"]]
        assert 0 <= oy < c["nz"] < oy + nprb and 0 <= ox < c["n"] < ox + nprb and valid[0, s["overhang"]]
        assert ip[0, s["outside"], 0] >= c["nz"] and ip[0, s["outside"], 1] >= c["n"] and valid[0, s["outside"]]
        want = sg.adj_scan_ref(c["farplane"], c["scan"], c["psi"], c["probe"], "double").reshape(-1, 2) if ndet <= 64 else None
        if want is not None:
            assert np.all(want[s["skipped"]] == 0) and np.all(want[s["outside"]] == 0)
            assert np.all(want[s["overhang"]] != 0) and np.all(want[s["negative_fraction"]] != 0)


def test_scangrad_index_logic_on_host(tmp_path):
    """csrc/k_scangrad.hpp walked thread by thread (sg_walk): for nprb in 1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257,
    512, 1024 every probe pixel is visited exactly once, and the carried taps and their in-object flags equal the plain
    statement ``psi[sy + i + a][sx + j + b]`` for patches inside the object, flush with and overhanging the bottom edge,
    the right edge and their corner, and wholly outside (positions are never negative: those are skipped)."""
    run = host_build.build("host_scangrad", tmp_path)
    out = run(check=False)
    assert out.returncode == 0, out.stdout
    last = out.stdout.splitlines()[-1]
    assert last.startswith("host_scangrad: 0 errors, "), out.stdout
    shapes, visits = (int(x) for x in re.findall(r"(\d+) (?:shapes|visits)", last))
    assert shapes >= 14 * 16 and visits > 0
    # one position by hand: 17^2 pixels once each; rows 20 .. 25 and column 30 of a 26 x 31 object are inside
    one = run("walk", 17, 20, 30, 26, 31).stdout.split()
    inside = sum(1 for i in range(17) for j in range(17) for a in (0, 1) for b in (0, 1) if 20 + i + a < 26 and 30 + j + b < 31)
    assert [int(v) for v in one] == [0, 17 * 17, 4 * 17 * 17 - inside]


def test_c_abi_argument_checks_need_no_gpu():
    import __graft_entry__ as ge
    ge.build_native()
    from libtike.hipfft import _native as nat
    assert "ptycho_adj_scan" in nat.SYMBOLS
    assert nat.adj_scan(None, None, None, None, None, None, None, 0, None) == 1      # null handle comes first
    assert b"null handle" in nat.last_error()
    assert nat.adj_scan(None, None, None, None, None, None, None, 4, None) == 1


def test_header_documents_adj_scan():
    text = open(os.path.join(ROOT, "include", "ptycho_hip.h")).read()
    m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*int ptycho_adj_scan\(ptycho_handle h, float\* out, const void\* g, const void\* f, "
                  r"const void\* scan,\s*const void\* prb, void\* work,\s*size_t work_tiles, void\* stream\);", text, flags=re.S)
    assert m, "ptycho_adj_scan is not declared with a comment in front of it"
    doc = m.group(1)
    for word in ("work_tiles", "PTYCHO_ERR_ARG", "float32 [ptheta][nscan][2]", "ptycho_fft2", "exactly 0.0", "same bits"):
        assert word in doc, word


def test_operator_class_has_the_new_methods():
    import __graft_entry__ as ge
    ge.build_native()
    import libtike.hipfft as pt
    from libtike.hipfft import ptycho as P
    for cls in (pt.PtychoCuFFT, pt.CGPtychoSolver, P.PtychoHIP):
        assert callable(getattr(cls, "adj_scan")) and callable(getattr(cls, "fwd_autograd"))
    assert "adj_scan" not in P.__all__ and "FwdFunction" not in P.__all__


def test_refinement_reaches_the_goal_with_the_float64_restatement():
    """End to end on the CPU: Adam on ``scan`` alone (``REFINE_LR``, ``REFINE_STEPS``) through ``fwd_torch`` in float64
    must bring the rms position error to at most 0.4 of its start, which leaves the GPU test's 0.5 a margin for float32.
    Measured: 0.3682 -> 0.0037 px (ratio 0.010), loss 3.069 -> 2.2e-4."""
    import torch
    s = sg.refine_scenario()
    psi, probe = torch.tensor(s["psi"].astype(np.complex128)), torch.tensor(s["probe"].astype(np.complex128))
    scan = torch.tensor(s["scan_start"], dtype=torch.float64)
    e0 = sg.rms_error(s["scan_start"], s["scan_true"])
    losses = sg.refine(lambda x: sg.fwd_torch(psi, x, probe, s["ndet"]), scan, torch.tensor(np.sqrt(s["data"])))
    e1 = sg.rms_error(scan.numpy(), s["scan_true"])
    print("refine (float64 restatement): rms %.4f -> %.4f px (ratio %.3f), loss %.4g -> %.4g" % (e0, e1, e1 / e0, losses[0], losses[-1]))
    assert e1 <= 0.4 * e0, (e0, e1)
