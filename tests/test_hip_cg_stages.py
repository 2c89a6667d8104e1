"""Every fused CG stage of the C ABI on its own, against the float64 stage reference of ``tests/cg_stages.py``.

The stages are driven through ``_native`` directly: work slots are filled with ``ptycho_cg_fwd_cols(_modes)`` and each
stage's outputs are read where they land -- device float64 sums and cost tables, the caller's intensity / image-product
/ arg-max arrays, and a projected residual through ``ptycho_cg_adj_cols`` (flg 0: object gradient, flg 1: probe
gradient).  The geometry matrix covers every detector size with fused stages, the full-width and the predicated column
variant of each where both exist, odd position counts, two angles, skipped / -0.0 / integer / overhanging positions and
one problem large enough that every workgroup loops over several row batches.

Tolerances.  For every comparison the error of the float32 evaluation of the same reference (``precision="single"``)
against float64 is measured on the same inputs; the device may be at most ``FACTOR`` times that error off, plus a floor
no larger than the operator bounds: ``REL_MAX`` of the largest element for arrays, ``SUM_REL`` of the sum of the
magnitudes of the terms for sums and costs (a cost near its minimum is bounded by its terms, not by its value).

Section H covers the tail of the object and probe steps (``ptycho_cg_obj_finish`` by route, ``ptycho_cg_prb_finish``): there
the object update must be bit-equal to its float32 restatement and a position's sub-pixel pick must lie within the float32
image product's own distance from the float64 one of the float64 window's top (``check_positions``).
"""
import ctypes

import numpy as np
import pytest

from oracle import ptycho_oracle as op
from libtike.hipfft import synthetic as syn

import cg_stages as cs
from hip_common import FACTOR, REL_MAX, crand, dev, host

pytestmark = pytest.mark.gpu

SUM_REL = 2e-6     # sums, relative to the sum of the magnitudes of their terms

# Detector columns per strip, ColCfg<N>::C of csrc/ptycho_common.hpp (T = N / E of the Stockham plan, fft_core.hpp).  A fused
# row stage runs its full-width variant (FW = true: unpredicated loads) when the strips of the probe, strip_range(), cover the
# whole row: xa = pad / C * C == 0 and xb == N (do_cg_rows; the projection always runs the predicated variant).
STRIP = {16: 16, 32: 32, 48: 48, 64: 64, 80: 16, 96: 16, 112: 16, 128: 32, 192: 16, 256: 16, 512: 16, 1024: 16, 2048: 8}


def full_width(ndet, nprb):
    c = STRIP[ndet]
    pad = (ndet - nprb) // 2
    return pad // c == 0 and ((pad + nprb - 1) // c + 1) * c == ndet


# ndet, nprb, ny, nx, step, ptheta: nscan = ny nx is odd (the last row batch is not full); the second entry of a size is the
# predicated variant wherever one exists (16, 32, 48, 64 have a single strip of the whole row: always full width)
GEOMS = [
    (16, 16, 3, 3, 5, 1), (16, 12, 3, 3, 5, 2),
    (32, 32, 3, 3, 6, 1), (32, 21, 3, 3, 6, 1),
    (48, 48, 3, 3, 7, 2), (48, 30, 3, 3, 7, 1),
    (64, 64, 3, 5, 9, 1), (64, 40, 3, 3, 9, 1),
    (80, 80, 3, 3, 9, 1), (80, 44, 3, 3, 9, 1),
    (96, 96, 3, 3, 9, 1), (96, 58, 3, 3, 9, 2),
    (112, 112, 3, 3, 11, 1), (112, 70, 3, 3, 11, 1),
    (128, 128, 3, 3, 11, 1), (128, 60, 3, 3, 11, 1),
    (192, 192, 1, 3, 13, 1), (192, 150, 1, 3, 13, 2),
    (256, 256, 1, 3, 17, 1), (256, 200, 1, 5, 17, 1),
    (512, 512, 1, 3, 21, 1), (512, 470, 1, 3, 21, 1),
    (1024, 1024, 1, 3, 31, 1), (1024, 990, 1, 3, 31, 1),
    (2048, 2048, 1, 3, 41, 1), (2048, 2000, 1, 3, 41, 1),
    (64, 64, 45, 45, 1, 1),          # 2025 positions: every workgroup loops over several batches, the fold sees the capped grid
]


def gid(g):
    return "n%d-p%d-%s-s%d-t%d" % (g[0], g[1], "full" if full_width(g[0], g[1]) else "pred", g[2] * g[3], g[5])


def make_problem(ndet, nprb, ny, nx, step, ptheta, seed=7):
    """Random-phase probe and the edge positions of test_hip_operators.problem(); psi is the current object, dpsi a
    direction, data = |fwd(truth)|^2 times noise."""
    p = syn.make_problem(ny, nx, step, nprb, ndet, ntheta=ptheta, seed=seed)
    rng = np.random.default_rng(seed + 1)
    prb = (p["probe"] * np.exp(2j * np.pi * rng.random(p["probe"].shape))).astype(np.complex64)
    scan = p["scan"]
    if p["nscan"] >= 3:
        scan[0, 0] = [2.0, 5.0]                              # exactly integer
        scan[0, 1] = [-1.5, 2.25]                            # skipped
        scan[0, 2] = [-0.25, 1.5]                            # trunc -> -0.0, not skipped
    if p["nscan"] >= 4:
        scan[-1, 3] = [p["nz"] - nprb / 2, 3.75]             # hangs over the bottom edge
    truth = p["psi"]
    psi = (truth * (1 + 0.2 * crand(rng, truth.shape))).astype(np.complex64)
    dpsi = (0.3 * crand(rng, truth.shape)).astype(np.complex64)
    data = np.abs(op.fwd(truth, scan, prb, ndet, "double")) ** 2
    data = (data * (0.6 + 0.8 * rng.random(data.shape))).astype(np.float32)
    mask = (rng.random((ndet, ndet)) >= 0.2).astype(np.uint8)
    mask[ndet // 3, :] = 0                                   # a whole row and a whole column unmeasured
    mask[:, ndet // 2 + 1] = 0
    bad = data.copy()
    junk = np.array([np.nan, -1.0, 1e30], np.float32)
    idx = np.nonzero(mask == 0)
    for t in range(bad.shape[0]):
        for s in range(bad.shape[1]):
            bad[t, s][idx] = junk[(idx[0] + idx[1] + s) % 3]
    return dict(p, prb=prb, scan=scan, psi=psi, dpsi=dpsi, data=data, bad=bad, mask=mask, ndet=ndet, nprb=nprb,
                ptheta=ptheta, rng=rng)


class Case:
    """One geometry: host problem, device operands, the float64 / float32 farplanes (made once) and a solver handle."""

    def __init__(self, g):
        import libtike.hipfft as pt
        self.g = g
        self.P = make_problem(*g)
        P = self.P
        self.D = dev
        self.slv = pt.CGPtychoSolver(P["nscan"], P["nprb"], P["ndet"], P["ptheta"], P["nz"], P["n"])
        self.h = self.slv._h
        self.psi, self.dpsi, self.scan, self.prb = (self.D(P[k]) for k in ("psi", "dpsi", "scan", "prb"))
        self.data, self.bad, self.mask = self.D(P["data"]), self.D(P["bad"]), self.D(P["mask"])
        self._far = {}

    def far(self, which, prec):
        """farplane of psi or dpsi with the case's probe, made once per precision"""
        k = (which, prec)
        if k not in self._far:
            self._far[k] = cs.farplane(self.P[which], self.P["scan"], self.P["prb"], self.P["ndet"], prec)
        return self._far[k]

    def close(self):
        self._far.clear()
        self.slv.free()


@pytest.fixture(scope="module", params=GEOMS, ids=gid)
def case(request):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    c = Case(request.param)
    try:
        yield c
    finally:
        c.close()
        torch.cuda.synchronize()
        torch.cuda.empty_cache()


# ---- helpers ---------------------------------------------------------------------------------------------------------
def nat_mod():
    from libtike.hipfft import _native as nat
    from libtike.hipfft.ptycho import _ptr, _stream
    return nat, _ptr, _stream


def set_stage(c, model, masked):
    nat, P_, S_ = nat_mod()
    nat.check(nat.set_option(c.h, b"model", nat.MODEL_POISSON_ML if model == "poisson_ml" else nat.MODEL_GAUSSIAN))
    nat.check(nat.set_mask(c.h, P_(c.mask) if masked else None, S_()))
    return (c.bad if masked else c.data), (c.P["bad"] if masked else c.P["data"]), (c.P["mask"] if masked else None)


def check_sum(got, want, w32, scale, what):
    tol = FACTOR * abs(w32 - want) + SUM_REL * scale
    assert abs(got - want) <= tol, "%s: got %.17g want %.17g (|err| %.3g, float32 ref %.3g, bound %.3g)" % (
        what, got, want, abs(got - want), abs(w32 - want), tol)


def check_array(got, want, w32, what):
    ref = np.abs(want).max()
    e = np.abs(got.astype(np.complex128) - want).max() / ref
    e32 = np.abs(w32.astype(np.complex128) - want).max() / ref
    assert e <= FACTOR * e32 + REL_MAX, "%s: rel err %.3g, float32 ref %.3g" % (what, e, e32)
    return e, e32


def zeros64(n):
    import torch
    return torch.zeros(n, dtype=torch.float64, device="cuda")


# ---- A. statistics ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_stats(case, masked):
    nat, P_, S_ = nat_mod()
    c = case
    d_dev, d, mask = set_stage(c, "gaussian", masked)
    nat.check(nat.cg_fwd_cols(c.h, 0, P_(c.psi), P_(c.scan), P_(c.prb), S_()))
    sums = zeros64(2)
    nat.check(nat.cg_stats(c.h, 0, P_(d_dev), P_(sums), S_()))
    got = host(sums)
    want = cs.stats(c.far("psi", "double"), d, mask)
    w32 = cs.stats(c.far("psi", "single"), d, mask, "single")
    for i, name in enumerate(("sum sqrt(I d)", "sum I")):
        check_sum(got[i], want[i], w32[i], want[i], name)
    nat.check(nat.set_mask(c.h, None, S_()))


# ---- B. projection ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("with_ab", [False, True], ids=["ab1", "ab"])
@pytest.mark.parametrize("model", ["gaussian", "poisson_ml"])
def test_project(case, model, with_ab, masked):
    """Cost, and the residual through adj_cols: flg 0 (object gradient) with {a, b}, flg 1 (probe gradient) without."""
    nat, P_, S_ = nat_mod()
    c = case
    P = c.P
    d_dev, d, mask = set_stage(c, model, masked)
    ab = np.array([0.8123, 0.6311]) if with_ab else None
    ab_dev = c.D(ab) if with_ab else None
    nat.check(nat.cg_fwd_cols(c.h, 0, P_(c.psi), P_(c.scan), P_(c.prb), S_()))
    r64, want, scale = cs.project(c.far("psi", "double"), d, ab, model, mask)
    r32, w32, _ = cs.project(c.far("psi", "single"), d, ab, model, mask, "single")
    flg = 0 if with_ab else 1
    if flg == 0:
        ref = op.adj(r64, P["scan"], P["prb"], P["nz"], P["n"], "double")
        ref32 = op.adj(r32, P["scan"], P["prb"], P["nz"], P["n"], "single")
    else:
        ref = op.adj_probe(r64, P["scan"], P["psi"], P["nprb"], "double")
        ref32 = op.adj_probe(r32, P["scan"], P["psi"], P["nprb"], "single")
    dets = [False, True] if P["ndet"] <= 512 and model == "gaussian" else [False]
    for det in dets:
        c.slv.set_deterministic(det)
        outs = []
        for rep in range(2 if det else 1):
            cost = zeros64(1)
            nat.check(nat.cg_project(c.h, 0, 1, P_(d_dev), P_(ab_dev) if with_ab else None, P_(cost), S_()))
            check_sum(float(host(cost)[0]), want, w32, scale, "cost %s det=%d" % (model, det))
            import torch
            if flg == 0:
                out = torch.zeros_like(c.psi)
                nat.check(nat.cg_adj_cols(c.h, 1, P_(out), P_(c.scan), P_(c.prb), 0, S_()))
            else:
                out = torch.zeros_like(c.prb)
                nat.check(nat.cg_adj_cols(c.h, 1, P_(c.psi), P_(c.scan), P_(out), 1, S_()))
            outs.append(host(out))
            check_array(outs[-1], ref, ref32, "residual through adj_cols flg=%d det=%d" % (flg, det))
        if det:
            assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), "deterministic adjoint not repeatable"
    c.slv.set_deterministic(False)
    nat.check(nat.set_mask(c.h, None, S_()))
    nat.check(nat.set_option(c.h, b"model", nat.MODEL_GAUSSIAN))


# ---- C. line search --------------------------------------------------------------------------------------------------
GAMMA0 = 0.7   # not a power of two


def check_ls(got, want, s64, w32, what):
    n = len(want) - 1
    for j in range(n + 1):
        check_sum(got[j], want[j], w32[j], s64[j], "%s costs[%d]" % (what, j))
    for j in range(n):   # what line_search_sqr reads: the sign of f(trial) - f(p1)
        check_sum(got[j] - got[n], want[j] - want[n], w32[j] - w32[n], s64[j] + s64[n], "%s costs[%d] - f(p1)" % (what, j))


@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
@pytest.mark.parametrize("model", ["gaussian", "poisson_ml"])
def test_linesearch(case, model, masked):
    nat, P_, S_ = nat_mod()
    c = case
    d_dev, d, mask = set_stage(c, model, masked)
    ab = np.array([0.8123, 0.6311])
    nat.check(nat.cg_fwd_cols(c.h, 0, P_(c.psi), P_(c.scan), P_(c.prb), S_()))
    nat.check(nat.cg_fwd_cols(c.h, 1, P_(c.dpsi), P_(c.scan), P_(c.prb), S_()))
    want, s64 = cs.linesearch(c.far("psi", "double"), c.far("dpsi", "double"), d, ab, GAMMA0, 16, model, mask)
    w32, _ = cs.linesearch(c.far("psi", "single"), c.far("dpsi", "single"), d, ab, GAMMA0, 16, model, mask, "single")
    for ncand in (1, 7, 16):
        costs = zeros64(ncand + 1)
        nat.check(nat.cg_linesearch(c.h, 0, 1, P_(d_dev), P_(c.D(ab)), GAMMA0, ncand, P_(costs), S_()))
        sel = list(range(ncand)) + [16]
        check_ls(host(costs), want[sel], s64[sel], w32[sel], "%s ncand=%d" % (model, ncand))
    nat.check(nat.set_mask(c.h, None, S_()))
    nat.check(nat.set_option(c.h, b"model", nat.MODEL_GAUSSIAN))


# ---- D. probe modes, slot pairs --------------------------------------------------------------------------------------
def mode_probes(c, M):
    rng = np.random.default_rng(100 + M)
    P = c.P
    return [(P["prb"] * (0.7 ** k) * np.exp(2j * np.pi * rng.random(P["prb"].shape))).astype(np.complex64) for k in range(M)]


# every mode count the multi-mode loop serves (two fwd_cols_modes launches above 4), each model and mask twice or more
MODE_CASES = [(1, "gaussian", False), (2, "poisson_ml", True), (3, "gaussian", True), (4, "poisson_ml", False),
              (5, "gaussian", False), (5, "poisson_ml", True), (8, "gaussian", True), (8, "poisson_ml", False)]


@pytest.mark.parametrize("M,model,masked", MODE_CASES, ids=["M%d-%s-%s" % (m, md, "mask" if k else "nomask") for m, md, k in MODE_CASES])
def test_modes(case, M, model, masked):
    """fwd_cols_modes (<= 4 modes per launch) + intensity_modes, linesearch_modes in the pair layout with mode0 > 0 and
    inten given or null, project_multi with slot_unscaled 0 and 1 -- at the sizes the multi-mode loop serves."""
    import torch
    nat, P_, S_ = nat_mod()
    c = case
    P = c.P
    if P["ndet"] > 512 or P["nscan"] > 100:
        pytest.skip("the multi-mode stages are exercised at ndet <= 512 (the large case is single-mode)")
    d_dev, d, mask = set_stage(c, model, masked)
    prbs = mode_probes(c, M)
    keep = [c.D(x) for x in prbs]
    ptrs = (ctypes.c_void_p * M)(*[t.data_ptr() for t in keep])
    nat.check(nat.cg_fwd_cols_modes(c.h, M, 0, P_(c.psi), P_(c.scan), ptrs, 0, 0, S_()))
    for k in range(M):
        nat.check(nat.cg_fwd_cols(c.h, 2 * k + 1, P_(c.dpsi), P_(c.scan), P_(keep[k]), S_()))
    G, G32, H, H32 = ([cs.farplane(P[w], P["scan"], x, P["ndet"], prec) for x in prbs]
                      for w, prec in (("psi", "double"), ("psi", "single"), ("dpsi", "double"), ("dpsi", "single")))
    # intensity array (written before the mask) and statistics
    inten = torch.empty(c.data.shape, dtype=torch.float32, device="cuda")
    sums = zeros64(2)
    nat.check(nat.cg_intensity_modes(c.h, M, P_(inten), P_(d_dev), P_(sums), S_()))
    i64, st64 = cs.intensity_modes(G, d, mask)
    i32, st32 = cs.intensity_modes(G32, d, mask, "single")
    check_array(host(inten), i64, i32, "inten M=%d" % M)
    got = host(sums)
    for i in range(2):
        check_sum(got[i], st64[i], st32[i], st64[i], "intensity_modes sums[%d]" % i)
    ab = np.array([0.8123, 0.6311])
    # line search over mode pairs mode0 .. mode0 + nmodes, with the device's inten as p1 or none
    for mode0 in sorted({0, M // 2, M - 1}):
        nm = M - mode0
        for use_inten in (False, True):
            costs = zeros64(17)
            nat.check(nat.cg_linesearch_modes(c.h, mode0, nm, P_(d_dev), P_(inten) if use_inten else None, P_(c.D(ab)),
                                              GAMMA0, 16, P_(costs), S_()))
            sl = slice(mode0, M)
            want, s64 = cs.linesearch_modes(G[sl], H[sl], d, ab, GAMMA0, 16, model, mask, host(inten) if use_inten else None)
            w32, _ = cs.linesearch_modes(G32[sl], H32[sl], d, ab, GAMMA0, 16, model, mask,
                                         host(inten) if use_inten else None, precision="single")
            check_ls(host(costs), want, s64, w32, "linesearch_modes M=%d mode0=%d inten=%d" % (M, mode0, use_inten))
    # projection of the last mode into its pair's second slot, residual through the object adjoint
    k = M - 1
    for unscaled in (1, 0):
        cost = zeros64(1)
        nat.check(nat.cg_project_multi(c.h, 2 * k, 2 * k + 1, P_(d_dev), P_(inten), P_(c.D(ab)), unscaled, P_(cost), S_()))
        r64, want, scale = cs.project_multi(G[k], host(inten), d, ab, unscaled, model, mask)
        r32, w32, _ = cs.project_multi(G32[k], host(inten), d, ab, unscaled, model, mask, "single")
        check_sum(float(host(cost)[0]), want, w32, scale, "project_multi cost unscaled=%d" % unscaled)
        out = torch.zeros_like(c.psi)
        nat.check(nat.cg_adj_cols(c.h, 2 * k + 1, P_(out), P_(c.scan), P_(keep[k]), 0, S_()))
        check_array(host(out), op.adj(r64, P["scan"], prbs[k], P["nz"], P["n"], "double"),
                    op.adj(r32, P["scan"], prbs[k], P["nz"], P["n"], "single"), "project_multi residual unscaled=%d" % unscaled)
    nat.check(nat.set_mask(c.h, None, S_()))
    nat.check(nat.set_option(c.h, b"model", nat.MODEL_GAUSSIAN))
    for s in range(2 * M):
        c.slv.release_work(s)


# ---- D'. compact layout: chunked line search ---------------------------------------------------------------------------
@pytest.mark.parametrize("model", ["gaussian", "poisson_ml"])
@pytest.mark.parametrize("M", [3, 5, 8])
@pytest.mark.parametrize("geom", [(64, 64, 1, 7, 9, 2), (96, 58, 1, 7, 9, 1), (256, 200, 1, 7, 17, 1)],
                         ids=["n64-full-s7-t2", "n96-pred-s7", "n256-pred-s7"])
def test_compact_chunks_sum_to_the_full_search(geom, M, model):
    """compact_modes = M: fwd_cols_modes(into_b = 1, chunk) + linesearch_chunk over all M chunks (positions % M != 0, so
    the last chunk is short) adds up to the float64 search over all positions and modes."""
    import libtike.hipfft as pt
    nat, P_, S_ = nat_mod()
    P = make_problem(*geom)
    assert (P["ptheta"] * P["nscan"]) % M != 0
    rng = np.random.default_rng(M)
    prbs = [(P["prb"] * (0.7 ** k) * np.exp(2j * np.pi * rng.random(P["prb"].shape))).astype(np.complex64) for k in range(M)]
    keep = [dev(x) for x in prbs]
    ptrs = (ctypes.c_void_p * M)(*[t.data_ptr() for t in keep])
    ab = np.array([0.8123, 0.6311])
    with pt.CGPtychoSolver(P["nscan"], P["nprb"], P["ndet"], P["ptheta"], P["nz"], P["n"]) as slv:
        h = slv._h
        psi, dpsi, scan, data = dev(P["psi"]), dev(P["dpsi"]), dev(P["scan"]), dev(P["data"])
        nat.check(nat.set_option(h, b"model", nat.MODEL_POISSON_ML if model == "poisson_ml" else nat.MODEL_GAUSSIAN))
        nat.check(nat.set_option(h, b"compact_modes", M))
        nat.check(nat.cg_fwd_cols_modes(h, M, 0, P_(psi), P_(scan), ptrs, 0, 0, S_()))
        costs = zeros64(17)
        for ch in range(M):
            nat.check(nat.cg_fwd_cols_modes(h, M, 0, P_(dpsi), P_(scan), ptrs, 1, ch, S_()))
            nat.check(nat.cg_linesearch_chunk(h, ch, P_(data), P_(dev(ab)), GAMMA0, 16, P_(costs), S_()))
        got = host(costs)
        nat.check(nat.set_option(h, b"compact_modes", 0))
    G = [cs.farplane(P["psi"], P["scan"], x, P["ndet"]) for x in prbs]
    H = [cs.farplane(P["dpsi"], P["scan"], x, P["ndet"]) for x in prbs]
    G32 = [cs.farplane(P["psi"], P["scan"], x, P["ndet"], "single") for x in prbs]
    H32 = [cs.farplane(P["dpsi"], P["scan"], x, P["ndet"], "single") for x in prbs]
    want, s64 = cs.linesearch_modes(G, H, P["data"], ab, GAMMA0, 16, model)
    w32, _ = cs.linesearch_modes(G32, H32, P["data"], ab, GAMMA0, 16, model, precision="single")
    check_ls(got, want, s64, w32, "compact M=%d" % M)


# ---- E. position-correction cross stage and arg-max ---------------------------------------------------------------------
def test_cross_and_argmax(case):
    """psi2 = psi shifted by a known whole-pixel offset plus noise; dpsi = (psi2 - psi) / gamma.  The image product
    elementwise; the arg-max of every position equal to the float64 one (each has one clear peak); the packed value equal
    to float32 |.| of the float64 maximum."""
    import torch
    nat, P_, S_ = nat_mod()
    c = case
    P = c.P
    if P["nscan"] > 100:
        pytest.skip("single-mode sizes only")
    rng = np.random.default_rng(5)
    gamma = 0.6
    shift = (2, -3)
    psi = crand(rng, P["psi"].shape)          # zero mean and white: the correlation of two patches peaks at the shift only
    psi2 = (np.roll(psi, shift, axis=(-2, -1)) + 0.05 * crand(rng, psi.shape)).astype(np.complex64)
    dpsi = ((psi2 - psi) / np.float32(gamma)).astype(np.complex64)
    ones = np.ones_like(P["prb"])
    ones_d, psi_d, dpsi_d = c.D(ones), c.D(psi), c.D(dpsi)
    nat.check(nat.cg_fwd_cols(c.h, 1, P_(psi_d), P_(c.scan), P_(ones_d), S_()))
    nat.check(nat.cg_fwd_cols(c.h, 2, P_(dpsi_d), P_(c.scan), P_(ones_d), S_()))
    ip = torch.empty((P["ptheta"], P["nscan"], P["ndet"], P["ndet"]), dtype=torch.complex64, device="cuda")
    best = torch.zeros(P["ptheta"] * P["nscan"], dtype=torch.int64, device="cuda")
    nat.check(nat.cg_cross(c.h, 1, 2, gamma, P_(ip), S_()))
    nat.check(nat.cg_argmax(c.h, 2, P_(best), S_()))
    U = cs.farplane(psi, P["scan"], ones, P["ndet"])
    Dd = cs.farplane(dpsi, P["scan"], ones, P["ndet"])
    ip64, idx, top, second = cs.cross(U, Dd, gamma)
    ip32 = cs.cross(cs.farplane(psi, P["scan"], ones, P["ndet"], "single"),
                    cs.farplane(dpsi, P["scan"], ones, P["ndet"], "single"), gamma, "single")[0]
    check_array(host(ip), ip64, ip32, "image product")
    b = host(best).view(np.uint64)
    got_idx = (0xffffffff - (b & 0xffffffff)).astype(np.int64)
    got_val = (b >> 32).astype(np.uint32).view(np.float32)
    live = top > 0
    assert live.sum() >= len(top) - 1                          # only the skipped position has an all-zero tile
    assert np.all(second[live] < 0.9 * top[live]), "design: one clear peak per position"
    assert np.array_equal(got_idx[live], idx[live]), (got_idx, idx)
    assert np.all(got_val[~live] == 0)
    assert np.all(np.abs(got_val[live] - top[live].astype(np.float32)) <= 1e-5 * top[live])
    c.slv.release_work(2)


# ---- F. native stages: object and probe side, line-search pass 5 (7 groups x 16 step lengths in one sweep) ----------------
# words of the device-resident state (include/ptycho_hip.h, enum PTYCHO_ST_*) that _native does not name
DY_OBJ, MAX_PRB, MAX_PSI, LS_GAMMA0, LS_NGROUPS, LS_TRIED, LS_RESOLVED = 4, 10, 11, 14, 16, 17, 18


def state_words(st):
    return host(st)


def float_word(st, i):
    return np.array([host(st)[i]]).view(np.uint64)[0].astype(np.uint32).view(np.float32)


@pytest.mark.parametrize("model", ["gaussian", "poisson_ml"])
def test_native_stages(case, model):
    import torch
    nat, P_, S_ = nat_mod()
    c = case
    P = c.P
    if P["ndet"] not in (64, 112, 256, 1024) or P["nscan"] > 100 or not full_width(P["ndet"], P["nprb"]):
        pytest.skip("native stages at 64, 112, 256, 1024")
    d_dev, d, mask = set_stage(c, model, False)
    S = S_()
    st = zeros64(nat.ST_WORDS)
    st[nat.ST_HINT:nat.ST_HINT + 2] = 14.0
    prb = c.prb.clone()
    no = c.psi
    grad, grad0, dpsi = torch.empty_like(no), torch.zeros_like(no), torch.zeros_like(no)
    nat.check(nat.cg_obj_begin(c.h, P_(st), P_(c.psi), P_(c.scan), P_(prb), P_(d_dev), S))
    w = state_words(st)
    G = c.far("psi", "double")
    want_ab = cs.stats(G, d, mask)
    w32_ab = cs.stats(c.far("psi", "single"), d, mask, "single")
    for i in range(2):
        check_sum(w[i], want_ab[i], w32_ab[i], want_ab[i], "state[A, B][%d]" % i)
    nat.check(nat.cg_obj_grad(c.h, P_(st), P_(c.scan), P_(prb), P_(d_dev), P_(grad), S))
    g_raw = host(grad)
    w = state_words(st)
    s32 = np.float32(np.float32(w[0]) / np.float32(w[1]))
    check_array(host(prb), P["prb"] * s32, P["prb"] * s32, "rescaled probe")
    assert abs(float_word(st, MAX_PRB) / np.abs(host(prb)).max() - 1) < 1e-6, "state[MAX_PRB]"
    ab = w[:2]
    r64, cost64, scale = cs.project(G, d, ab, model, mask)
    r32, cost32, _ = cs.project(c.far("psi", "single"), d, ab, model, mask, "single")
    check_sum(w[nat.ST_COST], cost64, cost32, scale, "state[COST]")
    prb_s = host(prb)
    check_array(g_raw, op.adj(r64, P["scan"], prb_s, P["nz"], P["n"], "double"),
                op.adj(r32, P["scan"], prb_s, P["nz"], P["n"], "single"), "raw object gradient")
    nat.check(nat.cg_obj_dir(c.h, P_(st), 1, P_(c.scan), P_(prb), P_(d_dev), P_(grad), P_(grad0), P_(dpsi), S))
    m2 = np.float32(float_word(st, MAX_PRB)) ** 2
    want_d = -(g_raw / m2)
    check_array(host(dpsi), want_d, want_d, "dpsi (first)")
    # pass 5 on a fresh search: 7 groups of 16 step lengths from gamma0
    g0 = 0.7
    st[LS_RESOLVED], st[LS_GAMMA0], st[LS_NGROUPS], st[LS_TRIED] = 0.0, g0, 0.0, 0.0
    nat.check(nat.cg_ls_next(c.h, P_(st), 0, 5, P_(d_dev), 1, S))
    table = state_words(st)[nat.ST_COSTS:nat.ST_COSTS + nat.ST_NCOSTS].reshape(7, 17)
    dps = host(dpsi)
    H = cs.farplane(dps, P["scan"], prb_s, P["ndet"])
    H32 = cs.farplane(dps, P["scan"], prb_s, P["ndet"], "single")
    for grp in range(7):
        y0 = float(np.float32(g0) * np.float32(2.0 ** (-16 * grp)))
        want, s64 = cs.linesearch(G, H, d, ab, y0, 16, model, mask)
        w32, _ = cs.linesearch(c.far("psi", "single"), H32, d, ab, y0, 16, model, mask, "single")
        check_ls(table[grp], want, s64, w32, "object pass 5 group %d" % grp)
    # a second direction: Dai-Yuan words and the direction of oracle/cg_oracle.py
    rng = np.random.default_rng(9)
    g2_raw = (crand(rng, no.shape) * np.abs(g_raw).max()).astype(np.complex64)
    g0_h, d_h = host(grad0), host(dpsi)
    grad2 = c.D(g2_raw)
    nat.check(nat.cg_obj_dir(c.h, P_(st), 0, P_(c.scan), P_(prb), P_(d_dev), P_(grad2), P_(grad0), P_(dpsi), S))
    gn = (g2_raw / m2).astype(np.complex128)
    dy = np.array([np.sum(np.abs(gn) ** 2), 0.0, 0.0])
    z = np.sum(np.conj(d_h.astype(np.complex128)) * (gn - g0_h))
    dy[1], dy[2] = z.real, z.imag
    w = state_words(st)
    mag = np.sum(np.abs(d_h) * (np.abs(gn) + np.abs(g0_h)))
    for i in range(3):
        check_sum(w[DY_OBJ + i], dy[i], dy[i], dy[0] if i == 0 else mag, "state[DY_OBJ + %d]" % i)
    want_d = -gn + (np.sum(np.abs(gn) ** 2) / z) * d_h
    check_array(host(dpsi), want_d, want_d, "Dai-Yuan direction")

    # probe side: prb_grad -> prb_dir -> pass 5 with which = 1 (no a / b)
    gprb, gprb0, dprb = torch.empty_like(prb), torch.zeros_like(prb), torch.zeros_like(prb)
    nat.check(nat.cg_prb_grad(c.h, P_(st), P_(c.psi), P_(c.scan), P_(prb), P_(d_dev), P_(gprb), S))
    Gp = cs.farplane(P["psi"], P["scan"], prb_s, P["ndet"])
    Gp32 = cs.farplane(P["psi"], P["scan"], prb_s, P["ndet"], "single")
    r64, cost64, scale = cs.project(Gp, d, None, model, mask)
    r32, cost32, _ = cs.project(Gp32, d, None, model, mask, "single")
    w = state_words(st)
    check_sum(w[nat.ST_COST2], cost64, cost32, scale, "state[COST2]")
    gp_raw = host(gprb)
    check_array(gp_raw, op.adj_probe(r64, P["scan"], P["psi"], P["nprb"], "double"),
                op.adj_probe(r32, P["scan"], P["psi"], P["nprb"], "single"), "raw probe gradient")
    nscan_total = float(P["ptheta"] * P["nscan"])
    nat.check(nat.cg_prb_dir(c.h, P_(st), 1, nscan_total, 1.0, P_(c.psi), P_(c.scan), P_(d_dev), P_(gprb), P_(gprb0),
                             P_(dprb), S))
    mp = np.float32(float_word(st, MAX_PSI))
    assert abs(mp / np.abs(P["psi"]).max() - 1) < 1e-6, "state[MAX_PSI]"
    want_dp = -(gp_raw / (mp * mp) / np.float32(nscan_total))
    check_array(host(dprb), want_dp, want_dp, "dprb (first)")
    st[LS_RESOLVED], st[LS_GAMMA0], st[LS_NGROUPS], st[LS_TRIED] = 0.0, g0, 0.0, 0.0
    nat.check(nat.cg_ls_next(c.h, P_(st), 1, 5, P_(d_dev), 0, S))
    table = state_words(st)[nat.ST_COSTS:nat.ST_COSTS + nat.ST_NCOSTS].reshape(7, 17)
    Hp = cs.farplane(P["psi"], P["scan"], host(dprb), P["ndet"])
    Hp32 = cs.farplane(P["psi"], P["scan"], host(dprb), P["ndet"], "single")
    for grp in range(7):
        y0 = float(np.float32(g0) * np.float32(2.0 ** (-16 * grp)))
        want, s64 = cs.linesearch(Gp, Hp, d, None, y0, 16, model, mask)
        w32, _ = cs.linesearch(Gp32, Hp32, d, None, y0, 16, model, mask, "single")
        check_ls(table[grp], want, s64, w32, "probe pass 5 group %d" % grp)
    nat.check(nat.set_option(c.h, b"model", nat.MODEL_GAUSSIAN))


# ---- G. scale invariance of the deterministic adjoints ----------------------------------------------------------------------
def test_deterministic_adjoints_are_scale_invariant(case):
    """ptycho_adj (flg 0 and 1) with option deterministic on y 2^k equals 2^k times the k = 0 result bit for bit: the
    fixed-point scale det_scale_of, evaluated by the accumulating column kernel and by the fold kernel, follows max |y|
    exactly and its +-120 clamp is not reached.  Each result also stays within the float64 tolerance."""
    import torch
    c = case
    P = c.P
    if P["ndet"] > 512 or P["nscan"] > 100:
        pytest.skip("the deterministic adjoints need the windowed kernels (ndet <= 512)")
    y = c.far("psi", "single") - 0.5 * c.far("dpsi", "single")
    want0 = op.adj(y, P["scan"], P["prb"], P["nz"], P["n"], "double")
    want1 = op.adj_probe(y, P["scan"], P["psi"], P["nprb"], "double")
    w32_0 = op.adj(y, P["scan"], P["prb"], P["nz"], P["n"], "single")
    w32_1 = op.adj_probe(y, P["scan"], P["psi"], P["nprb"], "single")
    c.slv.set_deterministic(True)
    base = None
    try:
        for k in (0, -60, -30, 30, 60):
            yk = c.D((y * np.float32(2.0 ** k)).astype(np.complex64))
            o = host(c.slv.adj(yk, c.scan, c.prb))
            q = host(c.slv.adj_probe(yk, c.scan, c.psi))
            if base is None:
                base = (o, q)
            else:
                sc = np.float32(2.0 ** k)
                assert np.array_equal(o, base[0] * sc), "adj at 2^%d is not 2^%d x adj" % (k, k)
                assert np.array_equal(q, base[1] * sc), "adj_probe at 2^%d is not 2^%d x adj_probe" % (k, k)
            check_array(o / np.float32(2.0 ** k), want0, w32_0, "deterministic adj 2^%d" % k)
            check_array(q / np.float32(2.0 ** k), want1, w32_1, "deterministic adj_probe 2^%d" % k)
    finally:
        c.slv.set_deterministic(False)
        torch.cuda.synchronize()


# ---- H. the tail of the object and probe steps: position correction by route, scan += shifts, psi += gamma dpsi ---------
REG_SIZES = (48, 64, 112, 192, 256, 512, 1024)
REG_GAMMA = 0.6
REG_SHIFT = (2.37, -3.41)
UPS, UP = 150, 100                  # the window and the upsample factor of the loop (cg_device.py)


def reg_case(c):
    """Inputs of section H, made once per geometry: white psi, psi2 = psi moved by REG_SHIFT + 5 % noise,
    dpsi = (psi2 - psi) / gamma; the case's scan with its skipped, -0.0, integer and overhanging positions."""
    if not hasattr(c, "_reg"):
        import torch
        from libtike.hipfft.registration import _zoom_kernel_factors
        P = c.P
        rng = np.random.default_rng(11)
        psi, dpsi = cs.shifted_pair(rng, P["psi"].shape, REG_SHIFT, REG_GAMMA)
        fac = _zoom_kernel_factors(P["ndet"], UP, "cuda")
        assert fac is not None and fac[3] == UPS
        c._reg = dict(psi=psi, dpsi=dpsi, ones=torch.ones_like(c.prb), vt=fac[0], lz=fac[1], nc=fac[2],
                      ref=reg_reference(c, psi, dpsi, REG_GAMMA))
    return c._reg


def reg_reference(c, psi, dpsi, gamma):
    """cs.finish in float64, and the image product of the float32 evaluation: E32 = sum |ip32 - ip64| per position bounds
    how far any window value of a float32 farplane can be off (every window-kernel entry has unit modulus)."""
    P = c.P
    f = cs.finish(psi, dpsi, gamma, P["scan"], P["ndet"], UP, nprb=P["nprb"])
    ones = np.ones((1, P["nprb"], P["nprb"]), np.complex64)
    ip32 = cs.cross(cs.farplane(psi[:1], P["scan"][:1], ones, P["ndet"], "single"),
                    cs.farplane(dpsi[:1], P["scan"][:1], ones, P["ndet"], "single"), gamma, "single")[0][0]
    f["e32"] = np.abs(ip32.astype(np.complex128) - f["ip"]).sum(axis=(1, 2))
    return f


def obj_finish(c, route, psi, dpsi, gamma, begin=None):
    """ptycho_cg_obj_finish(route) on fresh copies of psi and the case's scan, the gamma word set by the caller; returns
    (psi, scan) afterwards.  Route 2 runs ptycho_cg_reg_prepare first."""
    nat, P_, S_ = nat_mod()
    r = reg_case(c)
    S = S_()
    st = zeros64(nat.ST_WORDS)
    st[nat.ST_GAMMA_PSI] = gamma
    psi_d, dpsi_d, scan_d = c.D(psi), c.D(dpsi), c.scan.clone()
    nat.check(nat.set_option(c.h, b"trust_order", 0))          # as the loop does: nothing is known about this scan
    c.slv.profile(True)
    if route == 2:
        nat.check(nat.cg_reg_prepare(c.h, P_(st), P_(psi_d), P_(scan_d), P_(r["ones"]), S))
    nat.check(nat.cg_obj_finish(c.h, P_(st), route, P_(psi_d), P_(dpsi_d), P_(scan_d), P_(r["ones"]), P_(r["vt"]), P_(r["lz"]),
                                r["nc"], UPS, float(UP), S))
    out = host(psi_d), host(scan_d)
    prof = c.slv.profile_read()
    c.slv.profile(False)
    ran = {k: prof.get(k, (0.0, 0))[1] for k in ("k_rows_fused<CROSS>", "k_cols_argmax", "k_zoom_argmax")}
    assert all(n == (1 if route else 0) for n in ran.values()), "correct_positions = %d launched %s" % (route, ran)
    nat.check(nat.set_option(c.h, b"trust_order", 0))
    return out


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def check_positions(c, ref, scan_after, what):
    """The rules of section H for angle 0.  The internal shifts are not visible: the 1/100-grid index is recovered from
    scan_after - scan_before, such that float32(scan_before + float32(shift)) is scan_after bit for bit (the reference's
    float32 in-place add) with the reference's whole-pixel part.  The farplanes are float32 on the device, so the pick may
    sit on a neighbouring grid point: it is accepted only where the float64 window is within 2 FACTOR E32 of its top.
    Returns (positions with a single acceptable grid point, live positions, largest E32 / top)."""
    P = c.P
    N = P["ndet"]
    before = P["scan"][0]
    live = ref["top"] > 0
    assert live.sum() >= len(live) - 1, "only the skipped position has an all-zero tile"
    assert np.all(ref["second"][live] < 0.9 * ref["top"][live]), "design: one clear peak per position"
    whole = np.stack((cs.wrap_index(ref["idx"] // N, N), cs.wrap_index(ref["idx"] % N, N)), axis=1).astype(np.float64)
    grid = (np.arange(UPS, dtype=np.float64) - float(UPS // 2)) / float(UP)
    single = 0
    worst = 0.0
    for i in range(len(live)):
        if not live[i]:
            want = before[i] + np.float32(-0.75)
            assert np.array_equal(bits(scan_after[0, i]), bits(want)), "%s: skipped position %d moved by %s" % (
                what, i, scan_after[0, i] - before[i])
            continue
        pick = []
        for ax in range(2):
            cand = (before[i, ax] + (whole[i, ax] + grid).astype(np.float32)).astype(np.float32)
            j = np.nonzero(bits(cand) == bits(scan_after[0, i, ax]))[0]
            assert j.size == 1, "%s: position %d axis %d moved by %r: no shift of the reference's whole pixel %g on the 1/%d grid" % (
                what, i, ax, scan_after[0, i, ax] - before[i, ax], whole[i, ax], UP)
            pick.append(int(j[0]))
        w = ref["window"][i]
        top = w.max()
        margin = 2 * FACTOR * ref["e32"][i]
        worst = max(worst, ref["e32"][i] / top)
        assert w[pick[0], pick[1]] >= top - margin, "%s: position %d picked (%d, %d), window %.17g, top %.17g at %s, margin %.3g" % (
            what, i, pick[0], pick[1], w[pick[0], pick[1]], top, np.unravel_index(w.argmax(), w.shape), margin)
        single += int((w >= top - margin).sum() == 1)
    print("%s: %d of %d live positions with a single acceptable grid point, largest E32 / top %.3g" % (what, single, live.sum(), worst))
    assert single >= live.sum() - 1, "design: the margin must leave one grid point (%s: %d of %d)" % (what, single, live.sum())
    return single, int(live.sum()), worst


def test_obj_finish_by_route(case):
    """ptycho_cg_obj_finish with correct_positions 0, 1, 2 (after ptycho_cg_reg_prepare) and 3 (after obj_begin2 / obj_grad /
    obj_dir2 with the ones probe) against cs.finish; the in-kernel scan[0] += shifts, angle 0 only; k_cg_axpy on all angles.
    Routes 1 and 2 run the same kernels on the same operands, and the paired gather of route 3 multiplies the same patch by
    the ones probe (exact) before the same column DFT, so all three must leave the same bits in scan."""
    import torch
    nat, P_, S_ = nat_mod()
    c = case
    P = c.P
    if P["ndet"] not in REG_SIZES or P["nscan"] > 100:
        pytest.skip("the registration tail at 48, 64, 112, 192, 256, 512, 1024")
    r = reg_case(c)
    psi, dpsi, ref = r["psi"], r["dpsi"], r["ref"]
    # route 0: the object update alone
    psi0, scan0 = obj_finish(c, 0, psi, dpsi, REG_GAMMA)
    assert np.array_equal(bits(psi0), bits(ref["psi"])), "psi + gamma dpsi (float32 product, then float32 sum)"
    assert np.array_equal(bits(scan0), bits(P["scan"])), "correct_positions = 0 moved the scan"
    assert not np.array_equal(bits(psi0), bits(psi))
    # route 1: own column passes
    psi1, scan1 = obj_finish(c, 1, psi, dpsi, REG_GAMMA)
    assert np.array_equal(bits(psi1), bits(ref["psi"]))
    check_positions(c, ref, scan1, "route 1 %s" % gid(c.g))
    assert np.array_equal(bits(scan1[1:]), bits(P["scan"][1:])), "only angle 0 is corrected"
    assert not np.array_equal(bits(scan1[0]), bits(P["scan"][0]))
    again = obj_finish(c, 1, psi, dpsi, REG_GAMMA)
    assert np.array_equal(bits(again[0]), bits(psi1)) and np.array_equal(bits(again[1]), bits(scan1)), "route 1 twice"
    # route 2: slot 2 prepared; the same kernels on the same operands
    psi2, scan2 = obj_finish(c, 2, psi, dpsi, REG_GAMMA)
    assert np.array_equal(bits(psi2), bits(ref["psi"]))
    check_positions(c, ref, scan2, "route 2 %s" % gid(c.g))
    assert np.array_equal(bits(scan2), bits(scan1)), "routes 1 and 2 differ"
    # route 3: the operands ride along with the object step's own column passes (paired gather)
    S = S_()
    st = zeros64(nat.ST_WORDS)
    st[nat.ST_HINT:nat.ST_HINT + 2] = 14.0
    nat.check(nat.set_option(c.h, b"model", nat.MODEL_GAUSSIAN))
    nat.check(nat.set_mask(c.h, None, S))
    nat.check(nat.set_option(c.h, b"trust_order", 0))
    psi_d, scan_d, prb = c.D(psi), c.scan.clone(), c.prb.clone()
    grad, grad0, dd = torch.empty_like(psi_d), torch.zeros_like(psi_d), torch.zeros_like(psi_d)
    nat.check(nat.cg_obj_begin2(c.h, P_(st), P_(psi_d), P_(scan_d), P_(prb), P_(r["ones"]), P_(c.data), S))
    nat.check(nat.cg_obj_grad(c.h, P_(st), P_(scan_d), P_(prb), P_(c.data), P_(grad), S))
    nat.check(nat.cg_obj_dir2(c.h, P_(st), 1, P_(scan_d), P_(prb), P_(r["ones"]), P_(c.data), P_(grad), P_(grad0), P_(dd), S))
    dpsi3 = host(dd)
    assert np.all(np.isfinite(dpsi3.view(np.float32))) and np.abs(dpsi3).max() > 0
    gamma3 = float(np.float32(0.25 * np.abs(psi).max() / np.abs(dpsi3).max()))      # a step that moves psi by a quarter at most
    st[nat.ST_GAMMA_PSI] = gamma3
    nat.check(nat.cg_obj_finish(c.h, P_(st), 3, P_(psi_d), P_(dd), P_(scan_d), P_(r["ones"]), P_(r["vt"]), P_(r["lz"]),
                                r["nc"], UPS, float(UP), S))
    psi3, scan3 = host(psi_d), host(scan_d)
    nat.check(nat.set_option(c.h, b"trust_order", 0))
    ref3 = reg_reference(c, psi, dpsi3, gamma3)
    assert np.array_equal(bits(psi3), bits(ref3["psi"]))
    check_positions(c, ref3, scan3, "route 3 %s" % gid(c.g))
    assert np.array_equal(bits(scan3[1:]), bits(P["scan"][1:])), "only angle 0 is corrected"
    psi31, scan31 = obj_finish(c, 1, psi, dpsi3, gamma3)
    check_positions(c, ref3, scan31, "route 1 on route 3's operands %s" % gid(c.g))
    assert np.array_equal(bits(psi31), bits(psi3))
    print("routes 1 and 3 bit-equal: %s" % np.array_equal(bits(scan31), bits(scan3)))
    assert np.array_equal(bits(scan31), bits(scan3)), "routes 1 and 3 differ: %s" % (scan31[0] - scan3[0])
    for s in (2, 3):
        c.slv.release_work(s)


def test_prb_finish(case):
    """ptycho_cg_prb_finish: probe += float32(state[GAMMA_PRB]) dprb, float32 product then float32 sum, every angle."""
    nat, P_, S_ = nat_mod()
    c = case
    P = c.P
    if P["ndet"] not in REG_SIZES or P["nscan"] > 100:
        pytest.skip("the registration tail at 48, 64, 112, 192, 256, 512, 1024")
    rng = np.random.default_rng(13)
    dprb = (0.3 * crand(rng, P["prb"].shape)).astype(np.complex64)
    gamma = 0.37
    st = zeros64(nat.ST_WORDS)
    st[nat.ST_GAMMA_PRB] = gamma
    st[nat.ST_GAMMA_PSI] = 5.0                    # not the word this stage reads
    prb = c.prb.clone()
    nat.check(nat.cg_prb_finish(c.h, P_(st), P_(prb), P_(c.D(dprb)), S_()))
    want = cs.axpy32(P["prb"], dprb, gamma)
    assert not np.array_equal(bits(want), bits(P["prb"]))
    assert np.array_equal(bits(host(prb)), bits(want))
