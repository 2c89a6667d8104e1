"""The sub-pixel stage of the position registration on its own: every instantiation of the zoom kernels
(``csrc/k_zoom.hpp``, dispatched by ``zoom_impl`` of ``csrc/host_cg.hpp``) against the float64 reference ``cs.zoom`` of
``tests/cg_stages.py``, and the Python side of the registration (torch fallback, real-space wrapper) against the oracle.

The image product is complex64 on both sides and everything after it is float64 on both sides, so the shifts must be
bit-equal wherever the reference's own arg-max is well defined: the test asserts, as a condition on its inputs, that the
relative gap between the reference window's largest and second-largest value is at least ``GAP`` = 1e-9 at every position,
ten times the worst-case float64 summation bound ``N^2 eps`` = 1.2e-10 at ``N`` = 1024.

Sizes: ``k_zoom_argmax<256, 8>`` 48, 80, 112, 144, 240; ``<512, 4>`` 272, 400, 496; ``<1024, 2>`` 528, 720, 1008;
``k_zoom_mfma`` with idle row waves 192, 320, 576, 960 (256, 512 and 1024 are in ``test_hip_cg.py``).  Peaks: random within
+-3 pixels, and whole-pixel indices 0, 1, N/2 - 1, N/2, N/2 + 1, N - 1 on either axis with sub-pixel parts of both signs.
"""
import numpy as np
import pytest

import cg_stages as cs
from hip_common import dev

pytestmark = pytest.mark.gpu

GAP = 1e-9
ERR_ARG = 1                      # PTYCHO_ERR_ARG of include/ptycho_hip.h

SCALAR_256 = [48, 80, 112, 144, 240]
SCALAR_512 = [272, 400, 496]
SCALAR_1024 = [528, 720, 1008]
MFMA_IDLE = [192, 320, 576, 960]
SIZES = SCALAR_256 + SCALAR_512 + SCALAR_1024 + MFMA_IDLE


def npos(ndet):
    return 37 if ndet <= 256 else 9 if ndet <= 512 else 3


@pytest.fixture(scope="module")
def P():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from libtike.hipfft import ptycho
    return ptycho


def solver(P, nb, ndet):
    return P.CGPtychoSolver(nb, ndet, ndet, 1, ndet + 8, ndet + 8)


def packed(idx):
    """the whole-pixel peaks as ``ptycho_cg_argmax`` leaves them (only the low word is read)"""
    return dev(0xffffffff - np.asarray(idx, dtype=np.int64))


def random_peaks(rng, ndet, nb):
    true = rng.uniform(-3, 3, (nb, 2))
    whole = np.round(true).astype(np.int64)
    return true, np.where(whole < 0, whole + ndet, whole)


def edge_pairs(ndet, nb):
    """(row index, column index) pairs, a multiple of ``nb`` of them, in which either axis runs through all six edge indices"""
    e = cs.edge_indices(ndet)
    if nb >= 36:
        pairs = [(a, b) for a in e for b in e]
    else:
        pairs = [(e[i], e[(i + 3) % 6]) for i in range(6)]
        if nb > 6:
            pairs += [(e[2], e[2]), (e[3], e[3]), (e[4], e[5])]
    while len(pairs) % nb:
        pairs.append((e[3], e[4]))
    return np.array(pairs, dtype=np.int64)


def edge_peaks(rng, ndet, pairs):
    n = len(pairs)
    sign = np.stack(((-1.0) ** np.arange(n), (-1.0) ** (np.arange(n) // 2)), axis=1)
    frac = rng.uniform(0.05, 0.45, (n, 2)) * sign
    assert (frac > 0).any(0).all() and (frac < 0).any(0).all()
    return cs.wrap_index(pairs, ndet) + frac, pairs


def check_zoom(P, slv, ip, index, true, factor, what):
    """one batch: the kernel's shifts bit-equal to cs.zoom's, twice; returns the smallest reference gap"""
    ndet = ip.shape[-1]
    window, peak, want, gap = cs.zoom(ip, index[:, 0] * ndet + index[:, 1], factor)
    print("%s: smallest reference gap %.3g" % (what, gap.min()))
    assert np.all(gap >= GAP), "design: one clear peak per position (%s, smallest gap %.3g)" % (what, gap.min())
    assert np.abs(want - true).max() < 2.0 / factor, "design: the reference finds the planted shift"
    dip, best = dev(ip), packed(index[:, 0] * ndet + index[:, 1])
    slv.profile(True)
    got = P._zoom_shifts_native(slv, dip, best, factor)
    assert got is not None, "native zoom kernels declined a case they should cover (%s)" % what
    got = got.cpu().numpy()
    np.testing.assert_array_equal(got, want, err_msg=what)
    again = P._zoom_shifts_native(slv, dip, best, factor).cpu().numpy()
    launches = slv.profile_read().get("k_zoom_argmax", (0.0, 0))[1]
    slv.profile(False)
    assert np.array_equal(got.view(np.uint64), again.view(np.uint64)), "second call differs (%s)" % what
    assert launches == 2, "the zoom kernels ran %d times in two calls (%s)" % (launches, what)
    return gap.min()


@pytest.mark.parametrize("peaks", ["random", "edges"])
@pytest.mark.parametrize("ndet", SIZES)
def test_zoom_kernels_at_every_instantiation(P, ndet, peaks):
    nb = npos(ndet)
    rng = np.random.default_rng(1000 + ndet)
    with solver(P, nb, ndet) as slv:
        if peaks == "random":
            true, index = random_peaks(rng, ndet, nb)
            check_zoom(P, slv, cs.peak_product(rng, ndet, true), index, true, 100, "ndet %d random" % ndet)
        else:
            pairs = edge_pairs(ndet, nb)
            true, index = edge_peaks(rng, ndet, pairs)
            for b in range(0, len(pairs), nb):
                sl = slice(b, b + nb)
                check_zoom(P, slv, cs.peak_product(rng, ndet, true[sl]), index[sl], true[sl], 100,
                           "ndet %d edges %d" % (ndet, b // nb))


# upsample factor, window, detector sizes: a small window with another rank split; all but one thread of the 256-thread
# kernels (scalar and MFMA); a window wider than 256 threads (MFMA <512> and scalar <512, 4>); 512 threads of the 1024-thread kernel
FACTORS = [(10, 15, 112), (10, 15, 128), (170, 255, 112), (170, 255, 192), (200, 300, 320), (200, 300, 400), (341, 512, 576)]


@pytest.mark.parametrize("factor,window,ndet", FACTORS, ids=["up%d-n%d" % (f, n) for f, _, n in FACTORS])
def test_zoom_kernels_at_other_upsample_factors(P, factor, window, ndet):
    from libtike.hipfft import registration as reg
    nb = npos(ndet)
    rng = np.random.default_rng(2000 + ndet + factor)
    assert int(np.ceil(1.5 * factor)) == window
    with solver(P, nb, ndet) as slv:
        fac = reg._zoom_kernel_factors(ndet, factor, "cuda", widest=max(256, ndet))
        assert fac is not None and fac[3] == window and 0 < fac[2] <= 16
        print("factor %d ndet %d: nc = %d" % (factor, ndet, fac[2]))
        true, index = random_peaks(rng, ndet, nb)
        check_zoom(P, slv, cs.peak_product(rng, ndet, true), index, true, factor, "ndet %d factor %d" % (ndet, factor))


@pytest.mark.parametrize("ndet", [112, 128])
def test_an_all_zero_tile_moves_by_minus_three_quarters(P, ndet):
    """A skipped position has an all-zero tile: ``best`` starts at -1, the first ``mag = 0`` wins and ties go to the lowest
    index, so both kernel families return (0 - 75) / 100 on either axis, as the reference does."""
    nb = npos(ndet)
    rng = np.random.default_rng(3000 + ndet)
    true, index = random_peaks(rng, ndet, nb)
    ip = cs.peak_product(rng, ndet, true)
    for z in (0, 5, nb - 1):
        ip[z] = 0
        index[z] = 0
    want = cs.zoom(ip, index[:, 0] * ndet + index[:, 1], 100)[2]
    assert np.array_equal(want[[0, 5, nb - 1]], np.full((3, 2), -0.75))
    with solver(P, nb, ndet) as slv:
        got = P._zoom_shifts_native(slv, dev(ip), packed(index[:, 0] * ndet + index[:, 1]), 100).cpu().numpy()
    np.testing.assert_array_equal(got, want)


def test_zoom_refusals(P):
    """What the kernels do not cover is declined, never run: a window wider than the workgroup, more than 16 terms, an
    upsample factor below 1, a detector size that is no multiple of 16."""
    import torch
    from libtike.hipfft import _native as nat
    from libtike.hipfft.ptycho import _ptr, _stream
    rng = np.random.default_rng(1)
    for ndet in (64, 112, 256):
        with solver(P, 3, ndet) as slv:
            true, index = random_peaks(rng, ndet, 3)
            ip = dev(cs.peak_product(rng, ndet, true))
            best = packed(index[:, 0] * ndet + index[:, 1])
            assert P._zoom_shifts_native(slv, ip, best, 171) is None          # window 257 > 256 threads
            assert P._zoom_shifts_native(slv, ip, best, 170) is not None
    for ndet in (112, 320):
        with solver(P, 3, ndet) as slv:
            true, index = random_peaks(rng, ndet, 3)
            ip = dev(cs.peak_product(rng, ndet, true))
            best = packed(index[:, 0] * ndet + index[:, 1])
            widest = max(256, ndet)
            vt = torch.zeros((ndet, 16), dtype=torch.float64, device="cuda")
            lz = torch.zeros((widest + 1, 16), dtype=torch.float64, device="cuda")
            shifts = torch.full((3, 2), 7.0, dtype=torch.float64, device="cuda")

            def call(nc, ups, up):
                return nat.cg_zoom(slv._h, _ptr(ip), _ptr(best), _ptr(vt), _ptr(lz), nc, ups, up, _ptr(shifts), _stream())
            assert call(9, widest, 100.0) == 0
            assert call(9, widest + 1, 100.0) == ERR_ARG
            assert call(17, 150, 100.0) == ERR_ARG
            assert call(9, 150, 0.5) == ERR_ARG
            assert call(9, 0, 100.0) == ERR_ARG
            shifts.fill_(7.0)
            assert call(17, 150, 100.0) == ERR_ARG and bool((shifts == 7.0).all()), "a refused call writes nothing"
    ndet = 100
    with solver(P, 3, ndet) as slv:
        ip = torch.zeros((3, ndet, ndet), dtype=torch.complex64, device="cuda")
        best = packed(np.zeros(3, np.int64))
        vt = torch.zeros((ndet, 16), dtype=torch.float64, device="cuda")
        lz = torch.zeros((150, 16), dtype=torch.float64, device="cuda")
        shifts = torch.zeros((3, 2), dtype=torch.float64, device="cuda")
        assert nat.cg_zoom(slv._h, _ptr(ip), _ptr(best), _ptr(vt), _ptr(lz), 9, 150, 100.0, _ptr(shifts), _stream()) == ERR_ARG
        assert P._zoom_shifts_native(slv, ip, best, 100) is None


# ---- the image product in work slot 2, and gamma in device memory ------------------------------------------------------
@pytest.mark.parametrize("ndet", [112, 192], ids=["scalar-112", "mfma-192"])
def test_slot_2_form_and_device_gamma(P, ndet):
    """``cg_cross(h, 0, 1, gamma, NULL)`` + ``cg_zoom(h, NULL, ...)`` against the same with a caller's image-product tensor,
    and ``cg_cross_dev`` (gamma in a float64 word on the device) against ``cg_cross``: the same bits everywhere."""
    import torch
    from libtike.hipfft import synthetic as syn
    from libtike.hipfft import _native as nat
    from libtike.hipfft.ptycho import _ptr, _stream
    p = syn.make_problem(3, 3, 9, ndet, ndet, seed=2)
    rng = np.random.default_rng(3)
    gamma = 0.6
    psi, dpsi = cs.shifted_pair(rng, p["psi"].shape, (2.37, -3.41), gamma)
    psi_d, dpsi_d, scan = dev(psi), dev(dpsi), dev(p["scan"])
    ones = torch.ones((1, ndet, ndet), dtype=torch.complex64, device="cuda")
    nb = p["nscan"]
    with P.CGPtychoSolver(nb, ndet, ndet, 1, p["nz"], p["n"]) as slv:
        h = slv._h

        def fill():
            nat.check(nat.cg_fwd_cols(h, 0, _ptr(psi_d), _ptr(scan), _ptr(ones), _stream()))
            nat.check(nat.cg_fwd_cols(h, 1, _ptr(dpsi_d), _ptr(scan), _ptr(ones), _stream()))

        def registration(ip, cross):
            fill()
            nat.check(cross(ip))
            best = torch.zeros(nb, dtype=torch.int64, device="cuda")
            nat.check(nat.cg_argmax(h, 1, _ptr(best), _stream()))
            shifts = P._zoom_shifts_native(slv, ip, best, 100)
            assert shifts is not None
            return best.cpu().numpy(), shifts.cpu().numpy().view(np.uint64)

        ip1 = torch.zeros((nb, ndet, ndet), dtype=torch.complex64, device="cuda")
        best1, sh1 = registration(ip1, lambda ip: nat.cg_cross(h, 0, 1, gamma, _ptr(ip), _stream()))
        best2, sh2 = registration(None, lambda ip: nat.cg_cross(h, 0, 1, gamma, None, _stream()))
        gdev = torch.full((1,), gamma, dtype=torch.float64, device="cuda")
        ip3 = torch.zeros_like(ip1)
        best3, sh3 = registration(ip3, lambda ip: nat.cg_cross_dev(h, 0, 1, _ptr(gdev), _ptr(ip), _stream()))
        best4, sh4 = registration(None, lambda ip: nat.cg_cross_dev(h, 0, 1, _ptr(gdev), None, _stream()))
    assert np.array_equal(best1, best2) and np.array_equal(sh1, sh2), "slot-2 form"
    assert np.array_equal(ip1.cpu().numpy().view(np.uint32), ip3.cpu().numpy().view(np.uint32)), "cross_dev image product"
    assert np.array_equal(best1, best3) and np.array_equal(sh1, sh3), "cross_dev arg-max"
    assert np.array_equal(best1, best4) and np.array_equal(sh1, sh4), "cross_dev, slot-2 form"
    # and the result is the registration of the reference: the same whole-pixel peaks, the moved object found
    f = cs.finish(psi, dpsi, gamma, p["scan"], ndet, 100)
    assert np.all(f["second"] < 0.9 * f["top"]), "design: one clear peak per position"
    assert np.array_equal(0xffffffff - (best1.view(np.uint64) & 0xffffffff), f["idx"].astype(np.uint64))
    assert np.abs(sh1.view(np.float64) - f["shifts"]).max() <= 0.0100001


# ---- the Python side -------------------------------------------------------------------------------------------------
def fallback_pairs(ndet):
    e = cs.edge_indices(ndet)
    if ndet <= 200:
        return np.array([(e[i], e[(i + 3) % 6]) for i in range(6)], dtype=np.int64)
    if ndet <= 1000:
        return np.array([(e[2], e[4]), (e[3], e[5]), (e[4], e[3])], dtype=np.int64)
    return np.array([(e[3], e[4]), (e[4], e[3])], dtype=np.int64)


# the torch GEMM fallback serves ndet % 16 != 0 (30: the dense branch of _zoom_factors; 100, 200, 1000), ndet > 1024 (2048)
# and windows too wide for the kernel (factor 171 at 64)
@pytest.mark.parametrize("ndet,factor", [(30, 100), (100, 100), (200, 100), (1000, 100), (2048, 100), (64, 171)])
def test_torch_fallback_against_the_reference(P, ndet, factor):
    """``_finish_registration`` without an operator (torch GEMMs on the low-rank factors) against ``cs.zoom`` at the edge
    indices; torch divides by a scalar through its reciprocal (1 ulp), hence 1e-13 and not equality."""
    import torch
    rng = np.random.default_rng(4000 + ndet)
    pairs = fallback_pairs(ndet)
    true, index = edge_peaks(rng, ndet, pairs) if len(pairs) > 2 else (cs.wrap_index(pairs, ndet) + [[0.31, -0.17], [-0.23, 0.42]], pairs)
    ip = cs.peak_product(rng, ndet, true)
    window, peak, want, gap = cs.zoom(ip, index[:, 0] * ndet + index[:, 1], factor)
    assert np.all(gap >= GAP), "design: one clear peak per position"
    assert np.abs(want - true).max() < 2.0 / factor
    got = P._finish_registration(dev(ip), dev(index), factor)
    assert got.dtype == torch.float64
    np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=1e-13)
    if factor == 171:        # with an operator the kernel declines the window and the same fallback answers
        with solver(P, len(pairs), ndet) as slv:
            got = P._finish_registration(dev(ip), dev(index), factor, op=slv)
        np.testing.assert_allclose(got.cpu().numpy(), want, rtol=0, atol=1e-13)


@pytest.mark.parametrize("ndet", [100, 112, 192])
def test_real_space_registration_against_the_oracle(P, ndet):
    """``register_translation_batch(a, b, 100, "real", op=slv)``: the operator's own FFTs (float32) of real images moved
    by known sub-pixel shifts of both signs, against the oracle's (float64): within one step of the 1/100 grid of each
    other and within 0.011 of the planted shift."""
    from oracle import cg_oracle as co
    rng = np.random.default_rng(5000 + ndet)
    true = np.array([[1.25, -2.5], [0.0, 0.37], [-3.0, 4.11], [-0.43, -1.62], [2.38, 0.56]])
    nb = len(true)
    f = np.fft.fft2(rng.standard_normal((nb, ndet, ndet)))
    f[:, ndet // 2, :] = 0                        # no Nyquist row / column: the moved image is real too
    f[:, :, ndet // 2] = 0
    ky = np.fft.fftfreq(ndet)[None, :, None]
    kx = np.fft.fftfreq(ndet)[None, None, :]
    a = np.fft.ifft2(f)
    b = np.fft.ifft2(f * np.exp(-2j * np.pi * (ky * true[:, 0, None, None] + kx * true[:, 1, None, None])))
    assert np.abs(a.imag).max() < 1e-12 and np.abs(b.imag).max() < 1e-12
    a, b = a.real.astype(np.float32), b.real.astype(np.float32)
    want = co.register_translation_batch(a.astype(np.float64), b.astype(np.float64), 100, "real")
    with P.PtychoCuFFT(nb, ndet, ndet, 1, ndet + 8, ndet + 8) as slv:
        got = P.register_translation_batch(dev(a), dev(b), 100, "real", op=slv).cpu().numpy()
    assert got.dtype == np.float64
    assert np.abs(got - want).max() <= 0.0100001, np.abs(got - want).max()
    np.testing.assert_allclose(got, -true, atol=0.011)
    np.testing.assert_allclose(want, -true, atol=0.011)


@pytest.mark.parametrize("ndet", [30, 64])
def test_upsample_factor_one_returns_the_wrapped_whole_pixel_shifts(P, ndet):
    import torch
    e = cs.edge_indices(ndet)
    index = np.array([(a, b) for a in e for b in e], dtype=np.int64)
    ip = dev(np.ones((len(index), ndet, ndet), np.complex64))
    want = cs.wrap_index(index, ndet).astype(np.float64)
    got = P._finish_registration(ip, dev(index), 1)
    assert got.dtype == torch.float64
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    with solver(P, len(index), ndet) as slv:
        np.testing.assert_array_equal(P._finish_registration(ip, dev(index), 1, op=slv).cpu().numpy(), want)
