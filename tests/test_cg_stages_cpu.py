"""Pin the stage reference of ``tests/cg_stages.py`` against the CG oracles: composed into the first object iteration,
the stage functions must give what ``OracleSolver.run`` and, with a mask or the poisson_ml model, ``ReferenceSolver.run``
compute -- the probe rescale a / b, the projected residual of every mode, the object gradient, the logged cost and the
accepted step -- with and without a mask, for one and three probe modes.  The oracles' intermediates are read by
wrapping the solver instance's ``adj`` (their logic is not touched).  No GPU."""
import numpy as np
import pytest

from oracle import ptycho_oracle as op
from oracle.cg_oracle import OracleSolver
from libtike.hipfft import synthetic as syn

import cg_stages as cs
from cg_reference import ReferenceSolver, random_mask


def setup(ndet, nmodes, masked, seed=3):
    p = syn.make_problem(3, 3, 5, ndet, ndet, seed=seed)
    rng = np.random.default_rng(seed)
    nprb = ndet
    probes = np.stack([(p["probe"][0] * (0.6 ** k) * np.exp(2j * np.pi * rng.random((nprb, nprb))))
                       for k in range(nmodes)])[None].astype(np.complex64)       # [1, M, nprb, nprb]
    truth = p["psi"]
    data = sum(np.abs(op.fwd(truth, p["scan"], probes[:, k], ndet, "double")) ** 2 for k in range(nmodes))
    data = (data * (0.6 + 0.8 * rng.random(data.shape))).astype(np.float32)
    psi0 = (truth * (1 + 0.2 * (rng.standard_normal(truth.shape) + 1j * rng.standard_normal(truth.shape)))).astype(np.complex64)
    mask = None
    if masked:
        mask = random_mask(ndet, 0.25, seed=seed)
        mask[3, :] = 0
        mask[:, 5] = 0
        data = data.copy()
        data[:, :, mask == 0] = np.nan                 # whatever an unmeasured pixel holds is ignored
    return p, probes, psi0, data, mask


def first_iteration(ndet, nmodes, masked, model):
    """The oracle's first object iteration (probe rescale, residuals, gradient, cost, step) and the same composed from
    the stage functions."""
    p, probes, psi0, data, mask = setup(ndet, nmodes, masked)
    cls = ReferenceSolver if model == "poisson_ml" or masked else OracleSolver
    slv = cls(p["nscan"], ndet, ndet, 1, p["nz"], p["n"], precision="double")
    seen = []
    orig_adj = slv.adj

    def adj(far, scan, probe):
        out = orig_adj(far, scan, probe)
        seen.append((np.array(far), np.array(probe), out))
        return out
    slv.adj = adj
    kw = {} if cls is OracleSolver else {"mask": mask}
    prb_run = probes.copy()
    res = slv.run(data.copy(), psi0.copy(), p["scan"].copy(), prb_run, piter=1, model=model, **kw)
    ora = {"scale": prb_run[0, 0].ravel()[np.argmax(np.abs(probes[0, 0]))] / probes[0, 0].ravel()[np.argmax(np.abs(probes[0, 0]))],
           "residuals": [s[0] for s in seen], "gamma": slv.history[0][1], "cost": slv.history[0][3],
           "psi": res["psi"]}

    # ---- the same from the stages (float64) ----
    scan = p["scan"]
    G = [cs.farplane(psi0, scan, probes[:, k], ndet) for k in range(nmodes)]
    if nmodes == 1:
        ab = cs.stats(G[0], data, mask)
    else:
        inten, ab = cs.intensity_modes(G, data, mask)
    s = ab[0] / ab[1]
    scaled = probes * np.float32(s)
    res_k, grad, cost = [], 0, None
    for k in range(nmodes):
        if nmodes == 1:
            r, c, m = cs.project(G[0], data, ab, model, mask)
        else:
            r, c, m = cs.project_multi(G[k], inten, data, ab, 1, model, mask)
        if cost is None:
            cost, scale_cost = c, m
        res_k.append(r)
        grad = grad + op.adj(r, scan, scaled[:, k], p["nz"], p["n"], "double") / np.abs(scaled[:, k]).max() ** 2
    dpsi = -grad.astype(np.complex64)
    G2 = [cs.farplane(dpsi, scan, scaled[:, k], ndet) for k in range(nmodes)]
    # line_search_sqr from step 1 through groups of 16 step lengths: the first trial not above f(p1)
    step, gamma = 1.0, None
    for grp in range(8):
        if nmodes == 1:
            costs, _ = cs.linesearch(G[0], G2[0], data, ab, step, 16, model, mask)
        else:
            costs, _ = cs.linesearch_modes(G, G2, data, ab, step, 16, model, mask)
        ok = np.nonzero(costs[:16] <= costs[16])[0]
        if ok.size:
            gamma = 0.5 * step * 2.0 ** -ok[0]
            break
        step *= 2.0 ** -16
    mine = {"scale": s, "residuals": res_k, "gamma": gamma, "cost": cost, "scale_cost": scale_cost, "dpsi": dpsi}
    return ora, mine, psi0


@pytest.mark.parametrize("model", ["gaussian", "poisson_ml"])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("ndet,nmodes", [(16, 1), (32, 1), (16, 3), (32, 3)])
def test_stages_compose_into_the_oracles_first_iteration(ndet, nmodes, masked, model):
    ora, mine, psi0 = first_iteration(ndet, nmodes, masked, model)
    # a / b: the oracle rescales the probe in place by exactly that factor (float32 probe)
    assert abs(ora["scale"] / mine["scale"] - 1) < 1e-6, (ora["scale"], mine["scale"])
    # The stages take a / b as float32 (the device does) and read the slot made with the probe before its rescale; the
    # oracle uses a / b in float64 and fwd with the rescaled complex64 probe times b / a.  Both differ from the stage
    # composition by float32 rounding of one factor (<= 1e-6 relative); a wrong formula is off by O(1).
    assert len(ora["residuals"]) == nmodes
    for got, want in zip(mine["residuals"], ora["residuals"]):
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    assert abs(mine["cost"] - ora["cost"]) <= 1e-6 * mine["scale_cost"]
    # the accepted step, and the gradient behind it (psi1 = psi0 - gamma grad, stored in complex64 by the oracle)
    assert mine["gamma"] is not None and mine["gamma"] > 0
    assert mine["gamma"] == ora["gamma"], (mine["gamma"], ora["gamma"])
    want = (psi0 + np.complex64(ora["gamma"]) * mine["dpsi"]).astype(np.complex64)
    assert np.abs(ora["psi"] - want).max() <= 1e-6 * np.abs(want).max()


def test_single_precision_reference_is_close_but_not_equal():
    """``precision="single"`` is the same operation evaluated in float32: distinct from float64, within float32 rounding."""
    p, probes, psi0, data, mask = setup(32, 1, True)
    G = cs.farplane(psi0, p["scan"], probes[:, 0], 32)
    G32 = cs.farplane(psi0, p["scan"], probes[:, 0], 32, "single")
    ab = cs.stats(G, data, mask)
    for model in ("gaussian", "poisson_ml"):
        r64, c64, m64 = cs.project(G, data, ab, model, mask)
        r32, c32, _ = cs.project(G32, data, ab, model, mask, "single")
        e = np.abs(r32 - r64).max() / np.abs(r64).max()
        assert 0 < e < 1e-5
        assert 0 < abs(c32 - c64) < 1e-5 * m64
        l64, s64 = cs.linesearch(G, G, data, ab, 0.7, 16, model, mask)
        l32, _ = cs.linesearch(G32, G32, data, ab, 0.7, 16, model, mask, "single")
        assert np.all(np.abs(l32 - l64) < 1e-5 * s64)
    assert np.all(np.isfinite(r64))


def test_mask_selects_before_arithmetic():
    """NaN, -1 and 1e30 at unmeasured pixels change nothing; the residual is 0 there."""
    p, probes, psi0, data, mask = setup(16, 1, True)
    G = cs.farplane(psi0, p["scan"], probes[:, 0], 16)
    outs = []
    for junk in (np.nan, -1.0, 1e30):
        d = data.copy()
        d[:, :, mask == 0] = junk
        ab = cs.stats(G, d, mask)
        r, c, _ = cs.project(G, d, ab, "poisson_ml", mask)
        ls, _ = cs.linesearch(G, G, d, ab, 0.3, 4, "gaussian", mask)
        outs.append((ab, r, c, ls))
        assert np.all(r[:, :, mask == 0] == 0)
    for o in outs[1:]:
        assert np.array_equal(o[0], outs[0][0]) and np.array_equal(o[1], outs[0][1])
        assert o[2] == outs[0][2] and np.array_equal(o[3], outs[0][3])


def test_cross_finds_a_known_shift():
    ndet, shift = 32, (3, -5)
    rng = np.random.default_rng(0)
    U = np.fft.fft2(rng.standard_normal((2, ndet, ndet)) + 1j * rng.standard_normal((2, ndet, ndet)))
    V = np.fft.fft2(np.roll(np.fft.ifft2(U), shift, axis=(-2, -1)))
    gamma = 0.75
    ip, idx, top, second = cs.cross(U[None], ((V - U) / gamma)[None], gamma)
    want = ((-shift[0]) % ndet) * ndet + (-shift[1]) % ndet
    assert np.all(idx == want) and np.all(second < 0.5 * top)
    assert np.allclose(ip, (U * np.conj(V))[None])


# ---- the registration tail: cs.zoom / cs.finish against the oracle's register_translation_batch ---------------------------
def test_zoom_and_finish_reproduce_the_oracles_registration():
    """``cs.finish`` (fwd with the ones probe, ``cs.cross``, ``cs.zoom``) gives the shifts of the oracle's
    ``register_translation_batch(tmp1, tmp2, 100, "fourier")`` bit for bit, and the float32 object update."""
    from oracle.cg_oracle import register_translation_batch
    ndet, nprb = 16, 12
    p = syn.make_problem(3, 3, 5, nprb, ndet, seed=4)
    rng = np.random.default_rng(4)
    gamma = 0.6
    psi, dpsi = cs.shifted_pair(rng, p["psi"].shape, (1.37, -2.41), gamma)
    scan = p["scan"].copy()
    scan[0, 1] = [-1.5, 2.25]                                  # skipped: an all-zero tile
    f = cs.finish(psi, dpsi, gamma, scan, ndet, 100, nprb=nprb)
    ones = np.ones((1, nprb, nprb), np.complex64)
    tmp1 = op.fwd(psi, scan, ones, ndet, "double")[0]
    tmp2 = tmp1 + np.float32(gamma) * op.fwd(dpsi, scan, ones, ndet, "double")[0]
    want = register_translation_batch(tmp1, tmp2, 100, "fourier")
    assert np.array_equal(f["shifts"], want), (f["shifts"], want)
    assert np.array_equal(f["ip"], tmp1 * np.conj(tmp2))
    live = f["top"] > 0
    assert live.sum() == len(live) - 1 and not live[1]
    assert np.all(np.abs(f["shifts"][live] - [-1.37, 2.41]) < 0.1)      # the registration sees the move
    assert np.all(f["gap"][live] > 1e-9)
    # the object update: float32 product, then float32 sum (distinct from the float64 value, within float32 rounding)
    g32 = np.float32(gamma)
    exact = psi.astype(np.complex128) + np.float64(g32) * dpsi.astype(np.complex128)
    assert f["psi"].dtype == np.complex64
    assert np.abs(f["psi"] - exact).max() <= 2.0 ** -23 * np.abs(exact).max()
    assert np.array_equal(f["psi"].real, psi.real + (g32 * dpsi.real).astype(np.float32))
    # float32 farplanes give the same whole-pixel peaks
    f32 = cs.finish(psi, dpsi, gamma, scan, ndet, 100, "single", nprb=nprb)
    assert f32["ip"].dtype == np.complex64 and np.array_equal(f32["idx"][live], f["idx"][live])


def test_an_all_zero_tile_moves_by_minus_three_quarters():
    """Reference quirk: a skipped position has an all-zero tile, both arg-maxima are index 0 and the position moves by
    ``(0 - fix(150 / 2)) / 100`` on each axis."""
    from oracle.cg_oracle import register_translation_batch
    z = np.zeros((2, 16, 16), np.complex128)
    want = register_translation_batch(z, z, 100, "fourier")
    assert np.array_equal(want, np.full((2, 2), -0.75))
    window, peak, shifts, gap = cs.zoom(z, np.zeros(2, np.int64), 100)
    assert np.array_equal(shifts, want) and np.all(peak == 0) and np.all(window == 0) and np.all(np.isinf(gap))


@pytest.mark.parametrize("ndet", [16, 48])
def test_zoom_wraps_the_edge_indices_as_the_oracle_does(ndet):
    """Whole-pixel peaks at 0, 1, N/2 - 1, N/2, N/2 + 1 and N - 1 on either axis (all 36 pairs), sub-pixel parts of both
    signs: the oracle finds the planted index, and ``cs.zoom`` from that index gives the oracle's shifts bit for bit."""
    from oracle.cg_oracle import register_translation_batch
    e = cs.edge_indices(ndet)
    iy, ix = (a.ravel() for a in np.meshgrid(e, e, indexing="ij"))
    rng = np.random.default_rng(ndet)
    frac = rng.uniform(0.05, 0.45, (iy.size, 2)) * np.where(rng.random((iy.size, 2)) < 0.5, -1.0, 1.0)
    assert (frac > 0).any(0).all() and (frac < 0).any(0).all()
    whole = np.stack((cs.wrap_index(iy, ndet), cs.wrap_index(ix, ndet)), axis=1)
    assert set(whole[:, 0]) == {0, 1, ndet // 2 - 1, ndet // 2, 1 - ndet // 2, -1}
    ip = cs.peak_product(rng, ndet, whole + frac).astype(np.complex128)
    want = register_translation_batch(ip, np.ones_like(ip), 100, "fourier")
    window, peak, shifts, gap = cs.zoom(ip, iy * ndet + ix, 100)
    assert np.array_equal(np.round(want), whole), "the oracle's whole-pixel stage finds the planted index"
    assert np.array_equal(shifts, want)
    assert np.abs(shifts - (whole + frac)).max() < 0.02 and np.all(gap > 1e-9)
