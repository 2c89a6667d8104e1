"""Parity of the HIP operators (through the C ABI, via ``libtike.hipfft``) with the
CPU oracle.  Everything here needs a real MI355X: ``pytest -m gpu``.

Tolerance: the rule of tests/hip_common.py.  Every operator output is compared with the oracle in float64 through
``check_op``: the device may have ``FACTOR`` = 4 times the error (largest element relative to the largest element of the
reference, and relative L2) that the oracle's float32 restatement of the same arithmetic (``"single"``; for ``fft2`` the
complex64 transform the oracle uses) has on the same inputs, not less than 2^-22 and never more than the former fixed
bounds ``REL_MAX`` / ``REL_L2``.  tests/test_operator_bounds_cpu.py shows on the CPU that no case here is decided by those
caps.  ``check_op`` prints the device error, the float32 oracle's and the bound of every comparison; the per-size maxima
of one full run are the table "Operator errors against the float32 oracle" in NOTEBOOK.md.  The impulse and cancellation
tests hold single elements to the same factor.  The adjoint identity is held to 1e-5 (BASELINE.json), accumulated in
float64.  The geometries and inputs live in tests/operator_cases.py, which the CPU test shares.
"""
import numpy as np
import pytest

from oracle import ptycho_oracle as op
from libtike.hipfft import synthetic as syn
import operator_cases as oc
from operator_cases import CASES, problem
from hip_common import FACTOR, OP_FLOOR, check_op, crand, dev, host, pt, rel_errors, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu
NAMES = ("fwd", "adj", "adj_probe")


def vdot(a, b):
    return np.vdot(b.astype(np.complex128), a.astype(np.complex128))


def unaligned(shape, fill=None):
    """A contiguous complex64 device tensor whose first byte is 8 but not 16 bytes aligned (``fill``: a host array)."""
    import torch
    numel = int(np.prod(shape))
    t = torch.empty(numel + 1, dtype=torch.complex64, device="cuda")[1:].view(*shape)
    assert t.data_ptr() % 16 == 8 and t.is_contiguous()
    if fill is not None:
        t.copy_(torch.as_tensor(np.ascontiguousarray(fill)))
    return t


def launches(slv):
    return {k: n for k, (_, n) in slv.profile_read().items()}


@pytest.mark.parametrize("ndet,nprb,ny,nx,step,ntheta", CASES)
def test_fwd_adj_adjprobe_match_oracle(pt, ndet, nprb, ny, nx, step, ntheta):
    p, y = oc.case_inputs(ndet, nprb, ny, nx, step, ntheta)
    w64 = oc.oracles(p["psi"], p["scan"], p["probe"], y, ndet, "double")
    w32 = oc.oracles(p["psi"], p["scan"], p["probe"], y, ndet, "single")
    with pt.PtychoCuFFT(p["nscan"], nprb, ndet, ntheta, p["nz"], p["n"]) as slv:
        assert (slv.ptheta, slv.nz, slv.n, slv.nscan, slv.ndet, slv.nprb) == \
            (ntheta, p["nz"], p["n"], p["nscan"], ndet, nprb)
        psi, scan, prb = dev(p["psi"]), dev(p["scan"]), dev(p["probe"])
        # ndet <= 128 has two paths: one launch with the tile in LDS (default) and the two-pass kernels
        for tile in ((True, False) if ndet <= 128 else (True,)):
            slv.set_tile(tile)
            tag = "oracle %d/%d tile=%d " % (ndet, nprb, tile)
            g = host(slv.fwd(psi, scan, prb))
            check_op(g, w64[0], w32[0], tag + "fwd")
            if p["nscan"] >= 4:
                assert np.all(g[0, 1] == 0)    # skipped position -> exact zeros
            check_op(host(slv.adj(dev(y), scan, prb)), w64[1], w32[1], tag + "adj")
            check_op(host(slv.adj_probe(dev(y), scan, psi)), w64[2], w32[2], tag + "adj_probe")


@pytest.mark.parametrize("ndet,nprb,ny,nx", [(16, 16, 151, 65), (32, 27, 67, 39), (64, 64, 41, 19), (128, 100, 17, 9),
                                               (48, 40, 50, 21), (80, 80, 24, 11), (96, 96, 20, 9), (112, 90, 19, 9)])
def test_tile_kernels_equal_the_two_pass_kernels(pt, ndet, nprb, ny, nx):
    """ndet <= 128, more positions than one trip of the persistent workgroups holds, a count that does not fill the last
    workgroup, two angles (the probe adjoint's accumulators are flushed at the angle change), padded probes, skipped and
    overhanging positions: the one-launch kernels (k_tile.hpp) against the two-pass kernels, and each of the two against
    the oracle."""
    p = problem(ndet, nprb, ny, nx, 3, ntheta=2)
    rng = np.random.default_rng(5)
    ns = p["nscan"]
    y = (rng.standard_normal((2, ns, ndet, ndet)) + 1j * rng.standard_normal((2, ns, ndet, ndet))).astype(np.complex64)
    with pt.PtychoCuFFT(ns, nprb, ndet, 2, p["nz"], p["n"]) as slv:
        psi, scan, prb, yd = dev(p["psi"]), dev(p["scan"]), dev(p["probe"]), dev(y)
        slv.set_tile(False)
        ref = [host(slv.fwd(psi, scan, prb)), host(slv.adj(yd, scan, prb)), host(slv.adj_probe(yd, scan, psi))]
        slv.set_tile(True)
        slv.profile(True)
        got = [host(slv.fwd(psi, scan, prb)), host(slv.adj(yd, scan, prb)), host(slv.adj_probe(yd, scan, psi))]
        ran = slv.profile_read()
        slv.profile(False)
    assert "k_fwd_tile" in ran and "k_adjprb_tile" in ran, ran      # the paths under test did run
    for name, a, b in zip(NAMES, got, ref):
        e = rel_errors(a, b.astype(np.complex128))
        assert e[0] < 2e-5 and e[1] < 2e-6, (name, e)
    w64 = oc.oracles(p["psi"], p["scan"], p["probe"], y, ndet, "double")
    w32 = oc.oracles(p["psi"], p["scan"], p["probe"], y, ndet, "single")
    for name, a, b, w, s in zip(NAMES, got, ref, w64, w32):
        check_op(a, w, s, "many positions %d/%d tile %s" % (ndet, nprb, name))
        check_op(b, w, s, "many positions %d/%d two-pass %s" % (ndet, nprb, name))
    assert np.all(got[0][0, 1] == 0)        # skipped position -> exact zeros


def test_chunking_does_not_change_results(pt):
    p = problem(64, 48, 5, 5, 7, 2)
    with pt.PtychoCuFFT(p["nscan"], 48, 64, 2, p["nz"], p["n"]) as slv:
        psi, scan, prb = dev(p["psi"]), dev(p["scan"]), dev(p["probe"])
        g0 = host(slv.fwd(psi, scan, prb))
        a0 = host(slv.adj(dev(g0), scan, prb))
        slv.set_chunk(7)                   # ragged chunks crossing the angle boundary
        g1 = host(slv.fwd(psi, scan, prb))
        a1 = host(slv.adj(dev(g0), scan, prb))
        b1 = host(slv.adj_probe(dev(g0), scan, psi))
        slv.set_chunk(0)
        b0 = host(slv.adj_probe(dev(g0), scan, psi))
    np.testing.assert_array_equal(g0, g1)
    assert rel_errors(a1, a0.astype(np.complex128))[0] < 1e-5      # atomics: order differs
    assert rel_errors(b1, b0.astype(np.complex128))[0] < 1e-5
    w64 = oc.oracles(p["psi"], p["scan"], p["probe"], g0, 64, "double")
    w32 = oc.oracles(p["psi"], p["scan"], p["probe"], g0, 64, "single")
    for what, got, k in (("fwd", g0, 0), ("adj", a0, 1), ("adj chunk 7", a1, 1), ("adj_probe", b0, 2), ("adj_probe chunk 7", b1, 2)):
        check_op(got, w64[k], w32[k], "chunking 64/48 " + what)


@pytest.mark.parametrize("ndet,nprb,ntheta", [(64, 64, 2), (128, 100, 1), (256, 256, 1)])
def test_object_adjoint_any_scan_order(pt, ndet, nprb, ntheta):
    """The LDS overlap-add window must not depend on the scan being a sorted raster:
    random positions in random order (with skipped and overhanging ones), window on/off."""
    rng = np.random.default_rng(9)
    nscan, nz, n = 150, ndet + 90, ndet + 130
    scan = np.empty((ntheta, nscan, 2), np.float32)
    scan[..., 0] = rng.random((ntheta, nscan)) * (nz - nprb - 1)
    scan[..., 1] = rng.random((ntheta, nscan)) * (n - nprb - 1)
    scan[0, 5] = [-3.5, 4.0]
    scan[-1, 7] = [nz - nprb / 3, n - nprb / 2]
    scan[0, 9:12] = scan[0, 8]                      # repeated position
    prb = (rng.standard_normal((ntheta, nprb, nprb)) + 1j * rng.standard_normal((ntheta, nprb, nprb))).astype(np.complex64)
    y = (rng.standard_normal((ntheta, nscan, ndet, ndet)) + 1j * rng.standard_normal((ntheta, nscan, ndet, ndet))).astype(np.complex64)
    psi = (rng.standard_normal((ntheta, nz, n)) + 1j * rng.standard_normal((ntheta, nz, n))).astype(np.complex64)
    w64 = oc.oracles(psi, scan, prb, y, ndet, "double")
    w32 = oc.oracles(psi, scan, prb, y, ndet, "single")
    with pt.PtychoCuFFT(nscan, nprb, ndet, ntheta, nz, n) as slv:
        res = []
        settings = ((0, True), (37, True), (0, False))
        for chunk, window in settings:
            slv.set_chunk(chunk)
            slv.set_window(window)
            res.append((host(slv.fwd(dev(psi), dev(scan), dev(prb))),
                        host(slv.adj(dev(y), dev(scan), dev(prb))),
                        host(slv.adj_probe(dev(y), dev(scan), dev(psi)))))
    for (chunk, window), got in zip(settings, res):
        for name, gg, w, s in zip(NAMES, got, w64, w32):
            check_op(gg, w, s, "scan order %d/%d chunk=%d window=%d %s" % (ndet, nprb, chunk, window, name))
        assert np.all(got[0][0, 5] == 0)


@pytest.mark.parametrize("case", oc.EDGE_CASES)
def test_edge_cases(pt, case):
    c = oc.edge_case(case)
    ndet, nprb, nz, n, nscan, scan, psi, prb, y = (c[k] for k in ("ndet", "nprb", "nz", "n", "nscan", "scan", "psi", "prb", "y"))
    with pt.PtychoCuFFT(nscan, nprb, ndet, 1, nz, n) as slv:
        g = host(slv.fwd(dev(psi), dev(scan), dev(prb)))
        a = host(slv.adj(dev(y), dev(scan), dev(prb)))
        b = host(slv.adj_probe(dev(y), dev(scan), dev(psi)))
    w64, w32 = oc.oracles(psi, scan, prb, y, ndet, "double"), oc.oracles(psi, scan, prb, y, ndet, "single")
    for name, got, w, s in zip(NAMES, (g, a, b), w64, w32):
        check_op(got, w, s, "edge case %s %s" % (case, name))       # a reference of zeros asks for exact zeros
    if case == "all_skipped":
        assert not g.any() and not a.any() and not b.any()


def test_optional_paths_give_the_same_results(pt):
    """ndet = 256 has two forward and two adjoint paths -- split two-pass (default) and unsplit two-pass; they must
    agree.  (The single-launch forward of the experiments build: tests/test_hip_experiments.py.)"""
    p = syn.make_problem(48, 48, 4, 256, 256, seed=2, nz=512, n=512)          # 2304 positions
    rng = np.random.default_rng(1)
    y = (rng.standard_normal((1, 2304, 256, 256)) + 1j * rng.standard_normal((1, 2304, 256, 256))).astype(np.complex64)
    with pt.PtychoCuFFT(2304, 256, 256, 1, 512, 512) as slv:
        psi, scan, prb, yd = dev(p["psi"]), dev(p["scan"]), dev(p["probe"]), dev(y)
        ref = [host(slv.fwd(psi, scan, prb)), host(slv.adj(yd, scan, prb)), host(slv.adj_probe(yd, scan, psi))]
        slv.set_split(False)               # unsplit column / row kernels
        uns = [host(slv.fwd(psi, scan, prb)), host(slv.adj(yd, scan, prb)), host(slv.adj_probe(yd, scan, psi))]
        slv.set_split(True)
        for a, b in zip(uns, ref):
            assert np.abs(a - b).max() <= 1e-5 * np.abs(b).max()
        slv.release_scratch()              # the adjoint's intermediate is given back and allocated again on demand
        again = host(slv.adj(yd, scan, prb))
        assert np.abs(again - ref[1]).max() <= 1e-5 * np.abs(ref[1]).max()


def test_optional_paths_match_the_oracle(pt):
    """The comparison above at a size the CPU oracle does in seconds (6 x 7 positions of 256^2 on a 400 x 400 object): split,
    unsplit and the adjoint after release_scratch, each against the oracle."""
    p = syn.make_problem(6, 7, 20, 256, 256, seed=2, nz=400, n=400)
    y = crand(np.random.default_rng(1), (1, 42, 256, 256))
    w64 = oc.oracles(p["psi"], p["scan"], p["probe"], y, 256, "double")
    w32 = oc.oracles(p["psi"], p["scan"], p["probe"], y, 256, "single")
    with pt.PtychoCuFFT(42, 256, 256, 1, 400, 400) as slv:
        psi, scan, prb, yd = dev(p["psi"]), dev(p["scan"]), dev(p["probe"]), dev(y)
        for split in (True, False):
            slv.set_split(split)
            got = [host(slv.fwd(psi, scan, prb)), host(slv.adj(yd, scan, prb)), host(slv.adj_probe(yd, scan, psi))]
            for name, g, w, s in zip(NAMES, got, w64, w32):
                check_op(g, w, s, "optional paths 256/256 split=%d %s" % (split, name))
        slv.set_split(True)
        slv.release_scratch()
        check_op(host(slv.adj(yd, scan, prb)), w64[1], w32[1], "optional paths 256/256 adj after release_scratch")


@pytest.mark.parametrize("ndet", [100, 112])
def test_deterministic_adjoints_at_a_size_that_is_not_a_power_of_two(pt, ndet):
    """Option deterministic on the Bluestein path (ndet 100) and on a mixed-radix plan (112 = 7 x 4 x 4): both adjoints
    equal the float-atomic ones to rounding and are bitwise equal between two calls."""
    import torch
    p = syn.make_problem(12, 12, 6, ndet, ndet, seed=8)
    rng = np.random.default_rng(2)
    y = (rng.standard_normal((1, 144, ndet, ndet)) + 1j * rng.standard_normal((1, 144, ndet, ndet))).astype(np.complex64)
    with pt.PtychoCuFFT(144, ndet, ndet, 1, p["nz"], p["n"]) as slv:
        psi, scan, prb, yd = dev(p["psi"]), dev(p["scan"]), dev(p["probe"]), dev(y)
        ref = [host(slv.adj(yd, scan, prb)), host(slv.adj_probe(yd, scan, psi))]
        slv.set_deterministic(True)
        a1 = [host(slv.adj(yd, scan, prb)), host(slv.adj_probe(yd, scan, psi))]
        a2 = [host(slv.adj(yd, scan, prb)), host(slv.adj_probe(yd, scan, psi))]
    for r, x1, x2 in zip(ref, a1, a2):
        assert np.array_equal(x1, x2)
        assert np.abs(x1 - r).max() <= 2e-6 * np.abs(r).max()


def test_fft2_matches_numpy(pt):
    # ndet <= 128: one launch with the tile in LDS (default) and the two-pass kernels; 1100 tiles of 64^2 are more than one
    # trip of the persistent workgroups (oc.FFT2_CASES)
    for ndet, nb, tile, x in oc.fft2_inputs():
        with pt.PtychoCuFFT(1, ndet, ndet, 1, ndet + 2, ndet + 2) as slv:
            slv.set_tile(tile)
            f = host(slv.fft2(dev(x)))
            b = host(slv.fft2(dev(x), inverse=True))
            xd = dev(x)
            inplace = host(slv.fft2(xd, out=xd))
        (wf, wb), (sf, sb) = oc.fft2_oracles(x)
        check_op(f, wf, sf, "fft2 %d x %d tile=%d forward" % (nb, ndet, tile))
        check_op(b, wb, sb, "fft2 %d x %d tile=%d inverse" % (nb, ndet, tile))
        np.testing.assert_array_equal(inplace, f)


def test_reference_adjoint_script(pt, model):
    """/root/reference/tests/test_adjoint.py:15-59 through the *_batch API."""
    n, nz, nscan, nprb, ndet = 600, 276, 100, 128, 128
    prb0 = np.zeros([1, 1, nprb, nprb], dtype="complex64")
    prb0[0] = model["prbamp"] * np.exp(1j * model["prbang"])
    scan = np.ones([1, nscan, 2], dtype="float32")
    temp = np.moveaxis(model["coords"], 0, 1)[:nscan]
    scan[0, :, 0] = temp[:, 1]
    scan[0, :, 1] = temp[:, 0]
    psi0 = np.ones([1, nz, n], dtype="complex64")
    psi0[0] = model["initpsiamp"] * np.exp(1j * model["initpsiang"])
    with pt.PtychoCuFFT(nscan, nprb, ndet, 1, nz, n) as slv:
        t1 = slv.fwd_ptycho_batch(psi0, scan, prb0)
        t2 = slv.adj_ptycho_batch(t1, scan, prb0)
        t3 = slv.adj_ptycho_batch_prb(t1, scan, psi0)
    a = np.sum(psi0 * np.conj(t2))
    b = np.sum(t1 * np.conj(t1))
    c = np.sum(prb0 * np.conj(t3))
    assert ((a - b) / a < 1e-3) & ((a - c) / a < 1e-3)       # the reference's PASSED line
    a, b, c = vdot(psi0, t2), vdot(t1, t1), vdot(prb0[:, 0], t3)
    assert abs(a - b) / abs(a) < 1e-5 and abs(a - c) / abs(a) < 1e-5
    check_op(t1, op.fwd(psi0, scan, prb0[:, 0], ndet, "double"), op.fwd(psi0, scan, prb0[:, 0], ndet, "single"),
             "reference adjoint script 128/128 fwd")


@pytest.mark.parametrize("nprb", [256, 128])
def test_adjoint_identity_full_size(pt, nprb):
    """BASELINE.json config 2 geometry: 4096 x (256 x 256), <Ax,y> = <x,A*y> with
    an independent random y, both adjoints, relative residual < 1e-5."""
    import torch
    p = syn.make_problem(64, 64, 8, nprb, 256, seed=1234, nz=768, n=768)
    with pt.PtychoCuFFT(4096, nprb, 256, 1, 768, 768) as slv:
        psi, scan, prb = dev(p["psi"]), dev(p["scan"]), dev(p["probe"])
        gen = torch.Generator(device="cuda").manual_seed(5)
        y = torch.view_as_complex(torch.randn((1, 4096, 256, 256, 2), generator=gen,
                                              device="cuda", dtype=torch.float32))
        Ax = slv.fwd(psi, scan, prb)
        lhs = torch.sum(Ax.to(torch.complex128) * y.conj().to(torch.complex128))
        Aty = slv.adj(y, scan, prb)
        rhs1 = torch.sum(psi.to(torch.complex128) * Aty.conj().to(torch.complex128))
        Bty = slv.adj_probe(y, scan, psi)
        rhs2 = torch.sum(prb.to(torch.complex128) * Bty.conj().to(torch.complex128))
        # Parseval: ||Ax||^2 = ||prb * patch||^2 -- checked on a sample of positions
        sel = np.arange(0, 4096, 512)
        q = p["probe"][:, None] * op.patches(p["psi"], p["scan"][:, sel], nprb, "double")
        got = (torch.abs(Ax[0, sel].to(torch.complex128)) ** 2).sum(dim=(1, 2)).cpu().numpy()
        want = (np.abs(q[0]) ** 2).sum(axis=(1, 2))
        lhs, rhs1, rhs2 = complex(lhs), complex(rhs1), complex(rhs2)
    assert abs(lhs - rhs1) / abs(lhs) < 1e-5
    assert abs(lhs - rhs2) / abs(lhs) < 1e-5
    np.testing.assert_allclose(got, want, rtol=1e-5)


def test_error_behaviour(pt):
    import torch
    from libtike.hipfft import _native as nat
    with pytest.raises(nat.PtychoHipError):
        pt.PtychoCuFFT(4, 16, 1100, 1, 1200, 1200)    # ndet neither <= 1024 nor a power of two
    with pytest.raises(nat.PtychoHipError):
        pt.PtychoCuFFT(4, 32, 16, 1, 64, 64)          # nprb > ndet
    slv = pt.PtychoCuFFT(4, 16, 16, 1, 64, 64)
    psi = torch.ones((1, 64, 64), dtype=torch.complex64, device="cuda")
    scan = torch.ones((1, 4, 2), dtype=torch.float32, device="cuda")
    prb = torch.ones((1, 16, 16), dtype=torch.complex64, device="cuda")
    with pytest.raises(AssertionError):
        slv.fwd(psi.to(torch.complex128), scan, prb)  # dtype assert, ptycho.py:82-84
    with pytest.raises(ValueError):
        slv.fwd(psi[:, :32], scan, prb)               # wrong shape never reaches the kernel
    slv.fwd(psi, scan, prb)
    slv.free()
    slv.free()                                        # idempotent, ptychofft.cu:49-57
    with pytest.raises(nat.PtychoHipError):
        slv.fwd(psi, scan, prb)
    with pytest.raises(NotImplementedError):
        pt.PtychoCuFFT(4, 16, 16, 1, 64, 64).run(None, None, None, None)
    # options that a path does not cover fail loudly instead of being ignored
    with pt.PtychoCuFFT(4, 30, 30, 1, 64, 64) as gen:               # Bluestein path without its window: no fixed-point object adjoint
        gen.set_deterministic(True)
        gen.set_window(False)
        g = gen.fwd(psi, scan, torch.ones((1, 30, 30), dtype=torch.complex64, device="cuda"))
        with pytest.raises(nat.PtychoHipError):
            gen.adj(g, scan, torch.ones((1, 30, 30), dtype=torch.complex64, device="cuda"))


# ---- detector sizes that are not a power of two (cuFFT takes any size, ptychofft.cu:13-20) ----------------
@pytest.mark.parametrize("ndet", oc.FFT2_ANY_SIZES)   # 48, 80, 96, 112, 192: own plans; the others: Bluestein
def test_fft2_any_size_matches_numpy(pt, ndet):
    x = oc.fft2_any_size_input(ndet)
    nb = x.shape[0]
    with pt.PtychoCuFFT(nb, ndet, ndet, 1, ndet + 2, ndet + 2) as slv:
        got = host(slv.fft2(dev(x)))
        back = host(slv.fft2(dev(x), inverse=True))
    (want, wantb), (s, sb) = oc.fft2_oracles(x)                           # inverse unnormalised, like cufftExecC2C INVERSE
    check_op(got, want, s, "fft2 any size %d forward" % ndet)
    check_op(back, wantb, sb, "fft2 any size %d inverse" % ndet)
    assert np.abs(got - want).max() <= 2e-6 * np.abs(want).max()          # this test's own bound from before the rule: stays
    assert np.abs(back - wantb).max() <= 2e-6 * np.abs(wantb).max()


@pytest.mark.parametrize("ndet,nprb,ntheta", [(112, 112, 1), (96, 64, 2), (100, 64, 2), (30, 17, 1), (200, 140, 1)])
def test_operators_any_detector_size_match_oracle(pt, ndet, nprb, ntheta):
    """/root/reference/tests/test_fsc.py:115-120 crops the detector and the probe from 128 to 112:
    fwd / adj / adj_probe at such sizes against the oracle, and the adjoint identity."""
    p = syn.make_problem(4, 5, 7, nprb, ndet, ntheta=ntheta, seed=ndet)
    rng = np.random.default_rng(1)
    scan = p["scan"].copy()
    scan[0, 0] = (-0.5, 1.0) if ndet in (96, 100) else scan[0, 0]   # -0.0 integer part: NOT skipped, negative fraction (kernels.cu:39)
    prb = (p["probe"] * np.exp(2j * np.pi * rng.random((nprb, nprb)))).astype(np.complex64)
    y = (rng.standard_normal((ntheta, p["nscan"], ndet, ndet)) + 1j * rng.standard_normal((ntheta, p["nscan"], ndet, ndet))).astype(np.complex64)
    with pt.PtychoCuFFT(p["nscan"], nprb, ndet, ntheta, p["nz"], p["n"]) as slv:
        g = host(slv.fwd(dev(p["psi"]), dev(scan), dev(prb)))
        a = host(slv.adj(dev(y), dev(scan), dev(prb)))
        b = host(slv.adj_probe(dev(y), dev(scan), dev(p["psi"])))
    w64, w32 = oc.oracles(p["psi"], scan, prb, y, ndet, "double"), oc.oracles(p["psi"], scan, prb, y, ndet, "single")
    for name, got, w, s in zip(NAMES, (g, a, b), w64, w32):
        check_op(got, w, s, "any detector size %d/%d %s" % (ndet, nprb, name))
    lhs = np.vdot(y.astype(np.complex128), g.astype(np.complex128))
    r1 = np.vdot(a.astype(np.complex128), p["psi"].astype(np.complex128))
    r2 = np.vdot(b.astype(np.complex128), prb.astype(np.complex128))
    assert abs(lhs - r1) < 1e-5 * abs(lhs) and abs(lhs - r2) < 1e-5 * abs(lhs)


@pytest.mark.parametrize("ndet,nprb", [(256, 256), (128, 96), (512, 512)])
def test_deterministic_adjoints_are_bitwise_reproducible(pt, ndet, nprb):
    """Option "deterministic": the object / probe adjoints accumulate in 64-bit fixed point with integer
    atomics, so repeated calls give identical bits (the reference's float atomicAdd, kernels.cu:73-80,92-93,
    and the default path here do not), and the result agrees with the default path to float32 rounding."""
    p = syn.make_problem(12, 12, 9, nprb, ndet, seed=4)
    rng = np.random.default_rng(2)
    y = (rng.standard_normal((1, 144, ndet, ndet)) + 1j * rng.standard_normal((1, 144, ndet, ndet))).astype(np.complex64)
    with pt.PtychoCuFFT(144, nprb, ndet, 1, p["nz"], p["n"]) as slv:
        psi, scan, prb, yd = dev(p["psi"]), dev(p["scan"]), dev(p["probe"]), dev(y)
        ref_a, ref_b = host(slv.adj(yd, scan, prb)), host(slv.adj_probe(yd, scan, psi))
        slv.set_deterministic(True)
        runs = [(host(slv.adj(yd, scan, prb)), host(slv.adj_probe(yd, scan, psi))) for _ in range(3)]
        slv.set_deterministic(False)
    for a, b in runs[1:]:
        np.testing.assert_array_equal(a, runs[0][0])
        np.testing.assert_array_equal(b, runs[0][1])
    assert np.abs(runs[0][0] - ref_a).max() <= 2e-6 * np.abs(ref_a).max()
    assert np.abs(runs[0][1] - ref_b).max() <= 2e-6 * np.abs(ref_b).max()


# Launches per kernel id of one fwd / adj / adj_probe call each (in-library profiler), by detector size and options: the
# record of which path the host dispatch takes.  None: the call is not part of the row.  One angle, 4 x 5 positions,
# nprb = ndet, a scan tensor of its own per call, all three alive (so every call that sorts the positions does sort them).
# Option "unaligned" is the test's, not the library's: the far plane of all three calls is 8 but not 16 bytes aligned, so
# do_fwd / do_adj (csrc/host_ops.hpp) leave the tile kernels out and row_path (csrc/col_path.hpp) gives ROWS_PLAIN; the
# expected ids of those two rows are read from that code.
SORT, TILE_F, TILE_P = "sort_positions", "k_fwd_tile", "k_adjprb_tile"
CF, CO, CP, RF, RI = "k_cols<FWD>", "k_cols<ADJ_OBJ>", "k_cols<ADJ_PRB>", "k_rows<fwd>", "k_rows<inv>"
LEDGER = [
    # ndet, options, fwd, adj, adj_probe
    (64, {}, {TILE_F: 1}, {SORT: 1, RI: 1, CO: 1}, {TILE_P: 1}),
    (64, {"tile": 0}, {SORT: 1, CF: 1, RF: 1}, {SORT: 1, RI: 1, CO: 1}, {SORT: 1, RI: 1, CP: 1}),
    (64, {"tile": 0, "window": 0}, {CF: 1, RF: 1}, {SORT: 1, RI: 1, CO: 1}, None),
    (64, {"unaligned": 1}, {SORT: 1, CF: 1, RF: 1}, {SORT: 1, RI: 1, CO: 1}, {SORT: 1, RI: 1, CP: 1}),
    (64, {"unaligned": 1, "window": 0}, {CF: 1, RF: 1}, {SORT: 1, RI: 1, CO: 1}, {SORT: 1, RI: 1, CP: 1}),
    (256, {}, None, {SORT: 1, RI: 1, CO: 1}, None),
    (256, {"chunk": 7}, None, {SORT: 1, RI: 3, CO: 3}, None),
    (100, {}, {CF: 1, RF: 2}, {SORT: 1, RI: 2, CO: 1}, {RI: 2, CP: 1}),   # Bluestein lines: a row and a column launch
]


def test_launch_ledger_of_the_operators(pt):
    import torch
    bad = []
    for ndet, options, want_fwd, want_adj, want_prb in LEDGER:
        p = syn.make_problem(4, 5, 5, ndet, ndet, seed=3)
        assert p["nscan"] == 20 and p["nz"] < ndet + 100 and p["n"] < ndet + 100
        with pt.PtychoCuFFT(20, ndet, ndet, 1, p["nz"], p["n"]) as slv:
            if "tile" in options:
                slv.set_tile(options["tile"])
            if "window" in options:
                slv.set_window(options["window"])
            if "chunk" in options:
                slv.set_chunk(options["chunk"])
            psi, prb = dev(p["psi"]), dev(p["probe"])
            scans = [dev(p["scan"]) for _ in range(3)]
            if options.get("unaligned"):
                y, out = unaligned((1, 20, ndet, ndet)).fill_(1), unaligned((1, 20, ndet, ndet))
                assert y.data_ptr() % 16 == 8 and out.data_ptr() % 16 == 8
            else:
                y, out = torch.ones((1, 20, ndet, ndet), dtype=torch.complex64, device="cuda"), None
                assert y.data_ptr() % 16 == 0
            slv.profile(True)
            for name, want, call in (("fwd", want_fwd, lambda: slv.fwd(psi, scans[0], prb, out=out)),
                                     ("adj", want_adj, lambda: slv.adj(y, scans[1], prb)),
                                     ("adj_probe", want_prb, lambda: slv.adj_probe(y, scans[2], psi))):
                if want is None:
                    continue
                call()
                got = {k: n for k, (_, n) in slv.profile_read().items()}
                print("ledger", ndet, options, name, got)
                if got != want:
                    bad.append((ndet, options, name, got, want))
            slv.profile(False)
    assert not bad, bad


# ---- a far plane that is 8 but not 16 bytes aligned -----------------------------------------------------------------------
@pytest.mark.parametrize("ndet,nprb,ntheta", oc.UNALIGNED)
def test_far_plane_aligned_to_8_bytes_only(pt, ndet, nprb, ntheta):
    """complex64 tensors are 8-byte aligned, no more (a view one element into a buffer).  The one-launch tile kernels and
    k_rows_tile / k_rows_slab move 16 bytes per lane and must not run on such a far plane: the dispatch (csrc/host_ops.hpp,
    row_path of csrc/col_path.hpp) takes the two-pass kernels, which move one element at a time.  fwd into it, both
    adjoints and fft2 from it, fft2 into it and in place, each against the oracle; the forward equal to the aligned call
    bit for bit where the profiler shows the same kernels."""
    p, y = oc.unaligned_inputs(ndet, nprb, ntheta)
    w64 = oc.oracles(p["psi"], p["scan"], p["probe"], y, ndet, "double")
    w32 = oc.oracles(p["psi"], p["scan"], p["probe"], y, ndet, "single")
    x = y[0]
    (wf, wb), (sf, sb) = oc.fft2_oracles(x)
    tag = "unaligned %d/%d " % (ndet, nprb)
    two_pass = ndet <= 128                    # sizes at which an aligned call takes the kernels that need 16 bytes
    kernels = lambda ran: sorted(k for k in ran if k != SORT)      # noqa: E731  (a scan sorted before is not sorted again)
    with pt.PtychoCuFFT(12, nprb, ndet, ntheta, p["nz"], p["n"]) as slv:
        psi, scan, prb = dev(p["psi"]), dev(p["scan"]), dev(p["probe"])
        slv.profile(True)
        if two_pass:
            slv.set_tile(False)
        g_al = host(slv.fwd(psi, scan, prb))                       # aligned, and two-pass at every size
        ran_al = launches(slv)
        slv.set_tile(True)
        out = unaligned(y.shape)
        g = slv.fwd(psi, scan, prb, out=out)
        assert g.data_ptr() == out.data_ptr()
        ran = launches(slv)
        print(tag, "fwd aligned", ran_al, "unaligned", ran)
        assert TILE_F not in ran and CF in ran and RF in ran, ran
        check_op(host(g), w64[0], w32[0], tag + "fwd")
        assert kernels(ran) == kernels(ran_al) and same_bits(host(g), g_al), (ran, ran_al)

        yu = unaligned(y.shape, y)
        a = host(slv.adj(yu, scan, prb))
        ran = launches(slv)
        assert RI in ran and CO in ran, ran
        check_op(a, w64[1], w32[1], tag + "adj")
        b = host(slv.adj_probe(yu, scan, psi))
        ran = launches(slv)
        print(tag, "adj_probe unaligned", ran)
        assert TILE_P not in ran and RI in ran and CP in ran, ran
        check_op(b, w64[2], w32[2], tag + "adj_probe")
        assert same_bits(host(yu), y)                              # the operators do not write their input

        # fft2: from it, into it, in place on it; two-pass means a row launch beside the column launch
        xu = unaligned(x.shape, x)
        f1 = host(slv.fft2(xu))
        ran1 = launches(slv)
        f2 = host(slv.fft2(dev(x), out=unaligned(x.shape)))
        ran2 = launches(slv)
        b1 = host(slv.fft2(xu, inverse=True))
        ran3 = launches(slv)
        f3 = host(slv.fft2(xu, out=xu))
        ran4 = launches(slv)
        slv.profile(False)
        print(tag, "fft2", ran1, ran2, ran3, ran4)
        assert RF in ran1 and RF in ran2 and RI in ran3 and RF in ran4, (ran1, ran2, ran3, ran4)
        for what, got in (("from", f1), ("into", f2), ("in place", f3)):
            check_op(got, wf, sf, tag + "fft2 %s an unaligned tensor" % what)
        check_op(b1, wb, sb, tag + "fft2 inverse from an unaligned tensor")
        assert same_bits(f1, f2) and same_bits(f1, f3)             # the same two kernels each time


# ---- single elements: impulses through every plan, cancellation, bilinear weights at the edges of float32 ----------------------
@pytest.mark.parametrize("N", oc.STOCKHAM)
def test_fft2_of_impulses(pt, N):
    """A tile with a single 1.0 at (r, c) transforms to exp(-/+ 2 pi i (r ky + c kx) / N): every output element is one
    product of table entries, of magnitude one, so a wrong twiddle or output index shows at full size in that element and
    nothing dilutes it.  Each element is held to FACTOR times the largest elementwise error of the complex64 CPU transform
    of the same six tiles (not less than 2^-22).  (Bluestein sizes: the impulse response goes through a convolution and has
    no such elementwise argument; they keep the random-input tests.)"""
    x, wf, wb = oc.impulse_tiles(N)
    _, (sf, sb) = oc.fft2_oracles(x)
    bad = []
    with pt.PtychoCuFFT(1, N, N, 1, N + 2, N + 2) as slv:
        for tile in ((True, False) if N <= 128 else (True,)):
            slv.set_tile(tile)
            for what, inverse, want, s32 in (("forward", False, wf, sf), ("inverse", True, wb, sb)):
                got = host(slv.fft2(dev(x), inverse=inverse)).astype(np.complex128)
                e32 = np.abs(s32.astype(np.complex128) - want).max()
                tol = max(FACTOR * e32, OP_FLOOR)
                d = np.abs(got - want)
                worst = np.unravel_index(d.argmax(), d.shape)
                print("impulses %d tile=%d %s: device %.3g at %s | complex64 transform %.3g | bound %.3g"
                      % (N, tile, what, d.max(), worst, e32, tol))
                if not d.max() <= tol:
                    bad.append((N, tile, what, d.max(), worst, tol))
    assert not bad, bad


@pytest.mark.parametrize("ndet", oc.CANCEL_SIZES)
def test_fwd_of_constants_cancels(pt, ndet):
    """psi = 1, probe = 1, integer positions: the near plane is the constant 1 / ndet and the far plane is ndet in bin
    (0, 0) and zero in every other bin.  Relative to the largest element that is the plain oracle check; beside it the
    largest magnitude outside bin (0, 0) may be FACTOR times what the float32 oracle leaves there, not less than 2^-22 of
    the value in bin (0, 0)."""
    c = oc.cancel_inputs(ndet)
    w64 = op.fwd(c["psi"], c["scan"], c["prb"], ndet, "double")
    w32 = op.fwd(c["psi"], c["scan"], c["prb"], ndet, "single")

    def off_dc(a):
        a = np.abs(a.astype(np.complex128))
        a[..., 0, 0] = 0
        return a.max()
    tol = max(FACTOR * off_dc(w32), OP_FLOOR * ndet)
    stockham = ndet in oc.STOCKHAM
    with pt.PtychoCuFFT(4, ndet, ndet, 1, c["nz"], c["n"]) as slv:
        for tile in ((True, False) if ndet <= 128 and stockham else (True,)):
            slv.set_tile(tile)
            g = host(slv.fwd(dev(c["psi"]), dev(c["scan"]), dev(c["prb"])))
            check_op(g, w64, w32, "constants %d tile=%d fwd" % (ndet, tile))
            print("constants %d tile=%d: off-DC device %.3g | float32 oracle %.3g | bound %.3g (DC %g)"
                  % (ndet, tile, off_dc(g), off_dc(w32), tol, ndet))
            assert off_dc(g) <= tol, (ndet, tile, off_dc(g), tol)


@pytest.mark.parametrize("ndet,nprb", oc.WEIGHT_EDGES)
def test_bilinear_weights_at_the_edges_of_float32(pt, ndet, nprb):
    """Fractions 2^-20, 1 - 2^-24, 0.5 and 0 on either axis, and a position whose last taps are the last object row and
    column (oc.weight_edge_inputs): a weight rebuilt in a lossy order, or a tap dropped because its weight is small, is a
    defect of relative size 1e-6 that random fractions hide."""
    c = oc.weight_edge_inputs(ndet, nprb)
    ip, fr, valid = op.split_positions(c["scan"], "double")
    assert valid.all() and np.array_equal(ip, c["want_int"]) and np.array_equal(fr, c["want_frac"])
    psi, scan, prb, y = c["psi"], c["scan"], c["prb"], c["y"]
    w64, w32 = oc.oracles(psi, scan, prb, y, ndet, "double"), oc.oracles(psi, scan, prb, y, ndet, "single")
    with pt.PtychoCuFFT(8, nprb, ndet, 1, c["nz"], c["n"]) as slv:
        for tile in ((True, False) if ndet <= 128 else (True,)):
            slv.set_tile(tile)
            got = [host(slv.fwd(dev(psi), dev(scan), dev(prb))), host(slv.adj(dev(y), dev(scan), dev(prb))),
                   host(slv.adj_probe(dev(y), dev(scan), dev(psi)))]
            for name, g, w, s in zip(NAMES, got, w64, w32):
                check_op(g, w, s, "weight edges %d/%d tile=%d %s" % (ndet, nprb, tile, name))
