"""Fit residuals on the GPU (csrc/k_fit.hpp, ``libtike.hipfft.fit``, ``PtychoHIP.residuals``) against the float64
restatement of tests/fit_ref.py, the bitwise guarantees, the mask rules, and the solver method against the cost the
CG loop logs.

Error bound of the comparison with float64: ``16 * 2^-23`` times the sum of the absolute magnitudes that enter a
quantity (``frames_mag`` / ``pixels_mag`` of the restatement).  16 covers the float32 roundings of ``|g|^2`` over up to
three modes, the scale, one 1-ulp square root or logarithm and the product, each of relative size ``2^-23``.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import fit_ref as ref  # noqa: E402
from hip_common import dev, pt, same_bits  # noqa: E402, F401

pytestmark = pytest.mark.gpu

BOUND = 16 * ref.ULP


_cases = {}


def case(name, plant=True):
    """Inputs and float64 restatements of one case, computed once; the tests copy before they plant anything."""
    key = (name, plant)
    if key not in _cases:
        g, data = ref.make_case(name, plant=plant)
        plain = ref.frames_pixels(g, data)
        ab = np.array([plain["frames"][..., 2].sum(), plain["frames"][..., 0].sum()])
        c = {"g": g, "data": data, "ab": ab, "f64": {False: plain, True: ref.frames_pixels(g, data, None, ab)}}
        _cases[key] = c
    return _cases[key]


def run_fit(pt, g, data, mask=None, ab=None, pixels=True):
    """``fit_frames`` on host arrays ``g [M, ...]``: the modes before the last one go through ``accumulate_intensity``."""
    inten = None
    for m in range(len(g) - 1):
        inten = pt.accumulate_intensity(dev(g[m]), out=inten)
    out = pt.fit_frames(dev(data), dev(g[-1]), inten, None if mask is None else dev(mask), None if ab is None else dev(ab),
                        pixels=pixels)
    return out["frames"].cpu().numpy(), None if out["pixels"] is None else out["pixels"].cpu().numpy()


# ---- 1. against the float64 restatement -----------------------------------------------------------------------------------
@pytest.mark.parametrize("with_ab", [False, True])
@pytest.mark.parametrize("name", list(ref.CASES))
def test_device_matches_the_float64_restatement(pt, name, with_ab):
    c = case(name)
    ab = c["ab"] if with_ab else None
    want = c["f64"][with_ab]
    frames, pixels = run_fit(pt, c["g"], c["data"], None, ab)
    f32 = ref.frames_pixels(c["g"], c["data"], None, ab, np.float32)
    worst = {}
    for key, got in (("frames", frames), ("pixels", pixels)):
        mag = want[key + "_mag"]
        assert got.shape == want[key].shape and got.dtype == np.float64
        err = np.abs(got - want[key])
        err32 = np.abs(f32[key] - want[key])
        scale = np.where(mag > 0, mag, 1.0) * ref.ULP
        worst[key] = ((err / scale).max(), (err32 / scale).max())
        assert (err[mag == 0] == 0).all()                              # nothing enters: exactly 0
    print("fit %s ab=%d  frames: device %.3f, float32 restatement %.3f;  pixels: device %.3f, float32 restatement %.3f"
          "  (units of 2^-23 x magnitude, bound 16)" % (name, with_ab, *worst["frames"], *worst["pixels"]))
    assert worst["frames"][0] <= 16 and worst["pixels"][0] <= 16, worst


# ---- 2. bits --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B", "C", "E", "F"])
def test_same_inputs_same_bits_and_the_options_do_not_touch_frames(pt, name):
    c = case(name)
    f1, p1 = run_fit(pt, c["g"], c["data"], None, c["ab"])
    f2, p2 = run_fit(pt, c["g"], c["data"], None, c["ab"])
    assert same_bits(f1, f2) and same_bits(p1, p2)
    ones = np.ones(c["data"].shape[-2:], np.uint8)
    f3, p3 = run_fit(pt, c["g"], c["data"], ones, c["ab"])
    assert same_bits(f1, f3) and same_bits(p1, p3)                     # an all-ones mask is no mask
    f4, p4 = run_fit(pt, c["g"], c["data"], None, c["ab"], pixels=False)
    assert p4 is None and same_bits(f1, f4)


def test_permuting_the_frames_permutes_the_rows(pt):
    c = case("C")
    perm = np.random.default_rng(3).permutation(c["data"].shape[1])
    f1, p1 = run_fit(pt, c["g"], c["data"])
    f2, _ = run_fit(pt, c["g"][:, :, perm], c["data"][:, perm])
    assert same_bits(f1[:, perm], f2)


@pytest.mark.parametrize("name", ["A", "C", "D", "F"])
def test_intensity_alone_equals_farplane_alone(pt, name):
    c = case(name)
    g, data = dev(c["g"][0]), dev(c["data"])
    a = pt.fit_frames(data, farplane=g)
    b = pt.fit_frames(data, intensity=pt.accumulate_intensity(g))
    assert same_bits(a["frames"].cpu().numpy(), b["frames"].cpu().numpy())
    assert same_bits(a["pixels"].cpu().numpy(), b["pixels"].cpu().numpy())


def test_unaligned_views_take_the_scalar_loads_and_give_the_same_bits(pt):
    """A tensor that starts 4 bytes into an allocation cannot be read with 16-byte loads."""
    import torch
    c = case("B")
    g, data = dev(c["g"][0]), dev(c["data"])
    want = pt.fit_frames(data, farplane=g)
    shifted = torch.empty(data.numel() + 1, dtype=torch.float32, device="cuda")[1:].view(data.shape)
    shifted.copy_(data)
    assert shifted.data_ptr() % 16 == 4 and shifted.is_contiguous()
    got = pt.fit_frames(shifted, farplane=g)
    assert same_bits(want["frames"].cpu().numpy(), got["frames"].cpu().numpy())
    assert same_bits(want["pixels"].cpu().numpy(), got["pixels"].cpu().numpy())


# ---- 3. mask --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["B", "C"])
def test_unmeasured_pixels_enter_nothing(pt, name):
    c = case(name)
    mask = ref.make_mask(c["data"].shape[-1])
    off = mask == 0
    want = ref.frames_pixels(c["g"], c["data"], mask, c["ab"])
    zd, zg = c["data"].copy(), c["g"].copy()
    zd[..., off] = 0
    zg[..., off] = 0
    f0, p0 = run_fit(pt, zg, zd, mask, c["ab"])
    for key, got in (("frames", f0), ("pixels", p0)):                  # the masked sums are the restatement's
        mag = want[key + "_mag"]
        assert (np.abs(got - want[key]) <= BOUND * mag).all()
    assert (p0[:, :, off] == 0).all() and np.isfinite(p0).all() and np.isfinite(f0).all()
    for garbage in (np.nan, np.inf, 1e30):
        bd = c["data"].copy()
        bd[..., off] = garbage
        bg = c["g"].copy()
        bg[..., off] = np.nan
        f1, p1 = run_fit(pt, bg, bd, mask, c["ab"])
        assert same_bits(f0, f1) and same_bits(p0, p1), garbage


@pytest.mark.parametrize("name", ["B", "C"])
def test_nan_at_a_measured_pixel_stays_in_its_frame(pt, name):
    c = case(name)
    mask = ref.make_mask(c["data"].shape[-1])
    y, x = np.argwhere(mask != 0)[37]
    frame = c["data"].shape[1] - 3
    bg, bd = c["g"].copy(), c["data"].copy()
    bg[-1, 0, frame, y, x] = np.nan                                    # model only: the sums of d alone stay finite
    f, p = run_fit(pt, bg, bd, mask)
    assert np.isnan(f[0, frame, [0, 2, 3, 4, 6]]).all() and np.isfinite(f[0, frame, [1, 5, 7]]).all()
    bd[0, frame, y, x] = np.nan                                        # model and data: the whole row
    f, p = run_fit(pt, bg, bd, mask)
    assert np.isnan(f[0, frame]).all()
    rest = np.ones(f.shape[:2], bool)
    rest[0, frame] = False
    assert np.isfinite(f[rest]).all()                                  # no other frame's row
    nan_pix = np.isnan(p).any(1)
    assert nan_pix[0, y, x] and nan_pix.sum() == 1                     # and no other pixel's sums


# ---- 4. accumulate_intensity ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["C", "F"])
def test_accumulate_intensity_is_the_float32_statement_bit_for_bit(pt, name):
    """Bitwise, not within 2 ulp: the kernel forms re * re, im * im and their sum as three rounded float32 operations
    (fused multiply-add contraction is off in fit_abs2) and adds the modes in order, which is what NumPy does."""
    import torch
    g = case("C")["g"] if name == "C" else np.stack([ref.make_case("F", seed=s)[0][0] for s in range(3)])
    buf = torch.full(g.shape[1:], float("nan"), dtype=torch.float32, device="cuda")
    tail = buf.view(-1)[1:]                                            # 4 bytes off: the loads without alignment
    for target in (None, buf):
        acc = target
        for m in range(3):
            if m == 0 and target is not None:                          # add = 0 overwrites whatever the buffer holds
                from libtike.hipfft import _native as nat
                from libtike.hipfft.operators import _ptr, _stream
                gm = dev(g[0])
                nat.check(nat.fit_accumulate(_ptr(acc), _ptr(gm), gm.numel(), 0, _stream()))
            else:
                acc = pt.accumulate_intensity(dev(g[m]), out=acc)
        want = ref.intensity(g, np.float32)
        assert want.dtype == np.float32
        assert np.array_equal(acc.cpu().numpy().view(np.uint32), want.view(np.uint32))
    gm = dev(g[0]).view(-1)[:tail.numel()]
    from libtike.hipfft import _native as nat
    from libtike.hipfft.operators import _ptr, _stream
    nat.check(nat.fit_accumulate(_ptr(tail), _ptr(gm), gm.numel(), 0, _stream()))
    assert np.array_equal(tail.cpu().numpy().view(np.uint32),
                          ref.intensity(g[:1], np.float32).reshape(-1)[:tail.numel()].view(np.uint32))


# ---- 5. the solver method -------------------------------------------------------------------------------------------------
def random_problem(shape, seed):
    ptheta, nscan, ndet, nmodes = shape
    rng = np.random.default_rng(seed)
    nz, n = ndet + 24, ndet + 40
    psi = ((0.8 + 0.2 * rng.random((ptheta, nz, n))) * np.exp(1j * (rng.random((ptheta, nz, n)) - 0.5))).astype(np.complex64)
    scan = np.stack([rng.uniform(0, nz - ndet - 1, (ptheta, nscan)), rng.uniform(0, n - ndet - 1, (ptheta, nscan))],
                    -1).astype(np.float32)
    y = np.linspace(-2, 2, ndet)
    env = np.exp(-(y[:, None] ** 2 + y[None, :] ** 2))
    probe = (30.0 * (rng.standard_normal((ptheta, nmodes, ndet, ndet)) * 0.2 + 1) * env
             * np.exp(1j * rng.standard_normal((ptheta, nmodes, 1, 1)))).astype(np.complex64)
    probe *= (0.6 ** np.arange(nmodes))[None, :, None, None].astype(np.float32)
    return psi, scan, probe, nz, n


@pytest.mark.parametrize("shape", [ref.CASES["B"], ref.CASES["C"], (1, 64, 64, 2)], ids=["B-bluestein", "C", "64x64x2"])
def test_residuals_is_fit_frames_on_the_solvers_own_farplanes(pt, shape):
    import torch
    ptheta, nscan, ndet, nmodes = shape
    psi, scan, probe, nz, n = random_problem(shape, 11)
    mask = ref.make_mask(ndet)
    with pt.PtychoHIP(nscan, ndet, ndet, ptheta, nz, n) as op:
        psi_d, scan_d, probe_d = dev(psi), dev(scan), dev(probe)
        g = [op.fwd(psi_d, scan_d, probe_d[:, m]) for m in range(nmodes)]
        g_host = np.stack([x.cpu().numpy() for x in g])
        data = np.random.default_rng(12).poisson(0.7 * ref.intensity(g_host)).astype(np.float32)   # flux off by 0.7
        data_d = dev(data)
        inten = None
        for m in range(nmodes - 1):
            inten = pt.accumulate_intensity(g[m], out=inten)
        keep = [t.clone() for t in (data_d, psi_d, scan_d, probe_d)]
        for msk in (None, mask):
            want = pt.fit_frames(data_d, g[-1], inten, None if msk is None else dev(msk))
            got = op.residuals(data_d, psi_d, scan_d, probe_d, mask=msk)
            assert same_bits(got["frames"].cpu().numpy(), want["frames"].cpu().numpy())
            assert same_bits(got["pixels"].cpu().numpy(), want["pixels"].cpu().numpy())
            f = got["frames"].cpu().numpy()
            assert got["cost_gaussian"].shape == (ptheta, nscan) and got["scale"].dim() == 0
            assert np.array_equal(got["cost_gaussian"].cpu().numpy(), f[..., 3])
            assert np.array_equal(got["cost_poisson"].cpu().numpy(), f[..., 4])
            assert np.array_equal(got["deviance"].cpu().numpy(), 2.0 * (f[..., 4] - f[..., 5]))
            assert np.array_equal(got["r_factor"].cpu().numpy(), f[..., 6] / f[..., 7])
            assert np.array_equal(got["flux_ratio"].cpu().numpy(), f[..., 1] / f[..., 0])
            # rescale: a / b of the float64 restatement; the second pass is fit_frames with that (a, b)
            r64 = ref.frames_pixels(g_host, data, msk)["frames"]
            a, b = r64[..., 2].sum(), r64[..., 0].sum()
            res = op.residuals(data_d, psi_d, scan_d, probe_d, mask=msk, rescale=True)
            assert res["scale"].dtype == torch.float64 and res["scale"].dim() == 0
            assert abs(float(res["scale"]) - a / b) <= 4 * BOUND * (a / b)
            assert abs(float(got["scale"]) - a / b) <= 4 * BOUND * (a / b)
            assert 0.7 < a / b < 0.9                                   # about sqrt(0.7): the planted flux error
            ab = torch.stack((want["frames"][..., 2].sum(), want["frames"][..., 0].sum()))
            again = pt.fit_frames(data_d, g[-1], inten, None if msk is None else dev(msk), ab)
            assert same_bits(res["frames"].cpu().numpy(), again["frames"].cpu().numpy())
            assert same_bits(res["pixels"].cpu().numpy(), again["pixels"].cpu().numpy())
            assert float(res["cost_gaussian"].sum()) < float(got["cost_gaussian"].sum())
        for t, k in zip((data_d, psi_d, scan_d, probe_d), keep):       # the inputs are not modified
            assert torch.equal(t, k)
        got3 = op.residuals(data_d, psi_d, scan_d, probe_d[:, 0])      # a 3-D probe is one mode
        one = pt.fit_frames(data_d, g[0])
        assert same_bits(got3["frames"].cpu().numpy(), one["frames"].cpu().numpy())


@pytest.mark.parametrize("model", ["gaussian", "poisson_ml"])
@pytest.mark.parametrize("nmodes", [1, 2])
def test_rescaled_cost_is_the_cost_the_cg_loop_logs(pt, nmodes, model):
    """``sum cost`` of ``residuals(rescale=True)`` against ``history[0]`` of ``run(piter=1)`` from the same start: 2e-4
    relative (twice the 1e-4 that tests/test_hip_cg.py allows the logged cost against the oracle), for poisson_ml
    relative to ``|cost| + sum d`` as tests/test_hip_poisson.py does."""
    import torch
    import libtike.hipfft.synthetic as syn
    ndet = 64
    p = syn.make_problem(8, 8, 6, ndet, ndet, seed=21)
    probe = (syn.hermite_modes(ndet, nmodes) if nmodes > 1 else p["probe"][:, None]).astype(np.complex64)
    with pt.CGPtychoSolver(p["nscan"], ndet, ndet, 1, p["nz"], p["n"]) as slv:
        slv.verbose, slv.log_every = False, 1
        psi_true, scan = dev(p["psi"]), dev(p["scan"])
        inten = sum(np.abs(slv.fwd(psi_true, scan, dev(probe[:, m])).cpu().numpy().astype(np.complex128)) ** 2
                    for m in range(nmodes))
        data = np.random.default_rng(22).poisson(inten * (200.0 / inten.max())).astype(np.float32)
        data_d, psi0, start = dev(data), dev(np.ones_like(p["psi"])), dev(probe * np.float32(1.3))
        res = slv.residuals(data_d, psi0, scan, start, rescale=True)
        key = "cost_gaussian" if model == "gaussian" else "cost_poisson"
        mine = float(res[key].sum())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            slv.run(data_d, psi0.clone(), scan.clone(), start.clone(), piter=1, model=model, recover_prb=True)
        torch.cuda.synchronize()
        logged = slv.history[0][3]
    ref_size = abs(logged) if model == "gaussian" else abs(logged) + float(data.sum())
    print("fit cost vs logged: modes %d %s  residuals %.9e  logged %.9e  relative %.2e (bound 2e-4)"
          % (nmodes, model, mine, logged, abs(mine - logged) / ref_size))
    assert abs(mine - logged) <= 2e-4 * ref_size


def test_rescale_with_a_process_group_is_refused(pt):
    psi, scan, probe, nz, n = random_problem((1, 4, 16, 1), 5)
    with pt.CGPtychoSolver(4, 16, 16, 1, nz, n) as slv:
        slv.group = object()                                           # refused before anything touches the group
        with pytest.raises(NotImplementedError, match="process group"):
            slv.residuals(dev(np.zeros((1, 4, 16, 16), np.float32)), dev(psi), dev(scan), dev(probe), rescale=True)
        slv.group = None


# ---- 6. flag_frames -------------------------------------------------------------------------------------------------------
def test_flag_frames_finds_the_planted_frames(pt):
    c = case("C", plant=False)
    data = c["data"].copy()
    data[0, [5, 64, 129]] *= 3                                         # tests/test_fit_cpu.py: > 50 sigma from the clean frames
    frames, _ = run_fit(pt, c["g"], data)
    import torch
    flagged = pt.flag_frames(torch.as_tensor(frames[..., 3], device="cuda"), nsigma=6.0)
    assert flagged.dtype == torch.bool and flagged.is_cuda
    assert sorted(np.flatnonzero(flagged.cpu().numpy()[0])) == [5, 64, 129]
