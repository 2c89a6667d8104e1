"""The LDS gather window of the forward and probe-adjoint column pass (``k_cols_gatherwin``, csrc/k_cols_window.hpp) at the
edges of its bookkeeping, against the CPU oracle in float64.

The scans come from ``tests/gatherwin_cases.py``: row gaps around the boundary between the window's two load paths, around
``nprb + 1`` (nothing kept / re-anchor) and around the window height (same slots, other rows), writes of slot 0 and of the
mirror row through either path, re-anchors on columns and on the angle, skipped positions inside a run.  Every test first
asks the model of that module, with the device's CU count, whether its case still reaches those events under the launcher
it goes through, so a device that cuts the runs differently cannot silently empty a case.  Expected values come from
``oracle.ptycho_oracle`` alone.

Tolerances are the project's: ``check_op`` of tests/hip_common.py for operator outputs (``FACTOR`` x the float32 oracle's
own error, between a floor and the caps ``REL_MAX`` / ``REL_L2``), ``check_array`` / ``check_sum`` of
tests/test_hip_cg_stages.py (``FACTOR`` x the float32 oracle's own error + floor) for the CG stages.
``pytest -m gpu``.
"""
import ctypes
import functools

import numpy as np
import pytest

from oracle import ptycho_oracle as op

import cg_stages as cs
import gatherwin_cases as gc
import hip_common
from hip_common import FACTOR, REL_MAX, crand, host, rel_errors

pytestmark = pytest.mark.gpu

SUM_REL = 2e-6     # tests/test_hip_cg_stages.py
TILE_KERNELS = ("k_fwd_tile", "k_adjprb_tile")


@pytest.fixture(scope="module")
def pt():   # not hip_common.pt: this one gives the shared cases and the device memory back when the module is done
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import libtike.hipfft as pt
    yield pt
    for f in (case, want_fwd, want_adj_probe, mode_probes, mode_intensity):
        f.cache_clear()
    torch.cuda.synchronize()
    torch.cuda.empty_cache()


def dev(x):
    import torch
    return torch.as_tensor(np.array(x), device="cuda")   # a copy: the shared case arrays are read-only


def n_cu():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count   # what ptycho_create reads (hipDeviceProp_t)


def frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def case(name):
    """The problem of a named scan, made once and shared read-only: two objects, a probe of random phase whose amplitude
    stays above a half (every row and column of a patch counts), a random farplane for the adjoint."""
    ndet, nprb, ntheta, nz, n, scan = gc.case_scan(name)
    rng = np.random.default_rng(99)
    nscan = scan.shape[1]
    psi = [crand(rng, (ntheta, nz, n)) for _ in range(2)]
    probe = ((0.5 + 0.5 * rng.random((ntheta, nprb, nprb))) * np.exp(2j * np.pi * rng.random((ntheta, nprb, nprb)))).astype(np.complex64)
    y = crand(rng, (ntheta, nscan, ndet, ndet))
    data = (0.5 + rng.random((ntheta, nscan, ndet, ndet))).astype(np.float32)
    frozen(psi[0], psi[1], probe, y, data)
    return dict(name=name, ndet=ndet, nprb=nprb, ntheta=ntheta, nz=nz, n=n, nscan=nscan, scan=scan, psi=psi, probe=probe, y=y,
                data=data, skipped=~gc.decode(scan)[2])


@functools.lru_cache(maxsize=None)
def want_fwd(name, which, precision="double"):
    c = case(name)
    return frozen(op.fwd(c["psi"][which], c["scan"], c["probe"], c["ndet"], precision))[0]


@functools.lru_cache(maxsize=None)
def want_adj_probe(name, which, precision="double"):
    c = case(name)
    return frozen(op.adj_probe(c["y"], c["scan"], c["psi"][which], c["nprb"], precision))[0]


def check_events(name, launchers, chunk=0):
    """the case still reaches its events on this device, under every launcher it is there for"""
    for launch in launchers:
        ev = gc.plan_events(gc.case_scan(name), launch, n_cu(), chunk)
        print(name, launch, "CUs", n_cu(), {k: v for k, v in ev.items() if k != "runs"}, "runs of", sorted(set(ev["runs"])))
        gc.assert_events(name, launch, ev)


def check_op(what, got, want, name, which):
    """``want(name, which)`` in double is the reference, in single the float32 restatement that sets the bound"""
    return hip_common.check_op(got, want(name, which), want(name, which, "single"), what)[0]


def configure(slv, options):
    if "split" in options:
        slv.set_split(options["split"])
    if "tile" in options:
        slv.set_tile(options["tile"])
    if "chunk" in options:
        slv.set_chunk(options["chunk"])


# ---- operators -----------------------------------------------------------------------------------------------------------
# (case, options, launchers whose events are asserted): the plans of gc.PLANS, with the options that reach them
SPLIT, UNSPLIT = ("fwd_split", "adj_probe_split"), ("fwd", "adj_probe")
OP_CONFIGS = [
    ("rows256", {}, ("adj_probe_split",)),
    ("rows256w", {}, ("fwd_split",)),
    ("rows256", {"split": False}, UNSPLIT),
    ("rows256", {"chunk": 37}, ("adj_probe_split",)),
    ("rows512", {}, UNSPLIT),
    ("rows192", {}, UNSPLIT),
    ("rows128", {"tile": False}, UNSPLIT),
    ("cols256", {}, SPLIT),
    ("cols256", {"split": False}, UNSPLIT),
    ("cols512", {}, UNSPLIT),
    ("cols192", {}, UNSPLIT),
    ("cols128", {"tile": False}, UNSPLIT),
]


def op_id(cfg):
    return cfg[0] + "".join("-%s%d" % (k, v) for k, v in sorted(cfg[1].items()))


@pytest.mark.parametrize("cfg", OP_CONFIGS, ids=op_id)
def test_fwd_and_adj_probe_match_oracle(pt, cfg):
    """fwd and adj_probe on object 0, object 1 and object 0 again on one handle (no window state may outlive a call), the
    forward output exactly zero at skipped positions and bit-equal on the repeat; adj_probe again under the deterministic
    option, against the oracle and twice bit-equal; the profiler shows the column kernels ran and not the tile kernels."""
    name, options, launchers = cfg
    check_events(name, launchers, options.get("chunk", 0))
    c = case(name)
    with pt.PtychoCuFFT(c["nscan"], c["nprb"], c["ndet"], c["ntheta"], c["nz"], c["n"]) as slv:
        configure(slv, options)
        scan, prb, y = dev(c["scan"]), dev(c["probe"]), dev(c["y"])
        psi = [dev(c["psi"][0]), dev(c["psi"][1])]
        slv.profile(True)
        first = None
        for which in (0, 1, 0):
            g = host(slv.fwd(psi[which], scan, prb))
            check_op("%s fwd object %d" % (op_id(cfg), which), g, want_fwd, name, which)
            assert np.all(g[c["skipped"]] == 0), "forward output at a skipped position"
            if first is None:
                first = g
            elif which == 0:
                assert np.array_equal(first.view(np.uint32), g.view(np.uint32)), "fwd of object 0 after object 1 differs"
            p = host(slv.adj_probe(y, scan, psi[which]))
            check_op("%s adj_probe object %d" % (op_id(cfg), which), p, want_adj_probe, name, which)
        ran = {k: n for k, (_, n) in slv.profile_read().items()}
        slv.profile(False)
        print(op_id(cfg), "launches", ran)
        total, chunk = c["ntheta"] * c["nscan"], options.get("chunk") or c["ntheta"] * c["nscan"]
        launches = -(-total // chunk)                        # the forward pass is one launch, the adjoint one per chunk
        assert ran.get("k_cols<FWD>") == 3 and ran.get("k_cols<ADJ_PRB>") == 3 * launches, ran
        assert not any(k in ran for k in TILE_KERNELS), ran
        slv.set_deterministic(True)
        a1 = host(slv.adj_probe(y, scan, psi[0]))
        a2 = host(slv.adj_probe(y, scan, psi[0]))
        check_op("%s adj_probe deterministic" % op_id(cfg), a1, want_adj_probe, name, 0)
        assert np.array_equal(a1.view(np.uint32), a2.view(np.uint32)), "deterministic option: two runs differ"


@pytest.mark.parametrize("name", ["rows256", "rows256w", "cols256"])
def test_split_and_unsplit_agree(pt, name):
    """ndet 256: the split passes (one radix-16 step in the row pass; 32-column strips forward) against the un-split ones"""
    check_events(name, {"rows256": ("adj_probe_split", "fwd", "adj_probe"), "rows256w": ("fwd_split",), "cols256": SPLIT + UNSPLIT}[name])
    c = case(name)
    out = {}
    with pt.PtychoCuFFT(c["nscan"], c["nprb"], c["ndet"], c["ntheta"], c["nz"], c["n"]) as slv:
        scan, prb, y, psi = dev(c["scan"]), dev(c["probe"]), dev(c["y"]), dev(c["psi"][0])
        for split in (True, False):
            slv.set_split(split)
            out[split] = host(slv.fwd(psi, scan, prb)), host(slv.adj_probe(y, scan, psi))
    for i, what in enumerate(("fwd", "adj_probe")):
        e = rel_errors(out[True][i], out[False][i].astype(np.complex128))
        print("%s %s split against un-split: rel_max %.3g (< %g)" % (name, what, e[0], 2 * REL_MAX))
        assert e[0] < 2 * REL_MAX, (what, e)


# ---- CG column stages, through _native as tests/test_hip_cg_stages.py drives them --------------------------------------------
def nat_mod():
    from libtike.hipfft import _native as nat
    from libtike.hipfft.ptycho import _ptr, _stream
    return nat, _ptr, _stream


def zeros64(n):
    import torch
    return torch.zeros(n, dtype=torch.float64, device="cuda")


def check_sum(got, want, w32, scale, what):
    tol = FACTOR * abs(w32 - want) + SUM_REL * scale
    print("%s: |err| %.3g, float32 ref %.3g, bound %.3g" % (what, abs(got - want), abs(w32 - want), tol))
    assert abs(got - want) <= tol, "%s: got %.17g want %.17g (|err| %.3g, float32 ref %.3g, bound %.3g)" % (
        what, got, want, abs(got - want), abs(w32 - want), tol)


MAX_MODES = 7


@functools.lru_cache(maxsize=None)
def mode_probes(name):
    """probes of independent random phase, amplitudes 0.7^k"""
    c = case(name)
    rng = np.random.default_rng(107)
    return frozen(*[(c["probe"] * (0.7 ** k) * np.exp(2j * np.pi * rng.random(c["probe"].shape))).astype(np.complex64)
                    for k in range(MAX_MODES)])


MODE_CONFIGS = [("rows256", 4), ("rows256", 2), ("rows256", 1), ("rows256", 7), ("rows512", 4), ("rows512", 2), ("rows512", 1),
                ("cols256", 4), ("cols256", 2), ("cols256", 1)]


@functools.lru_cache(maxsize=None)
def mode_intensity(name):
    """``{M: (i64, e32)}`` for the mode counts a case is run with: ``cs.intensity_modes`` of the oracle farplanes of the first
    M probes in float64, and the error of its float32 evaluation relative to the largest element.  Every farplane is made
    once: the sum of ``cs.intensity_modes`` runs over the modes in order, so its partial sums are the smaller counts'."""
    c = case(name)
    out, i64, i32 = {}, None, None
    for k, p in enumerate(mode_probes(name)[:max(m for nm, m in MODE_CONFIGS if nm == name)]):
        a = cs.intensity_modes([cs.farplane(c["psi"][0], c["scan"], p, c["ndet"], "double")])[0]
        b = cs.intensity_modes([cs.farplane(c["psi"][0], c["scan"], p, c["ndet"], "single")], precision="single")[0]
        i64, i32 = (a, b) if i64 is None else (i64 + a, i32 + b)
        if (name, k + 1) in MODE_CONFIGS:
            out[k + 1] = frozen(i64.copy())[0], np.abs(i32.astype(np.float64) - i64).max() / np.abs(i64).max()
    return out


@pytest.mark.parametrize("name,M", MODE_CONFIGS, ids=["%s-M%d" % m for m in MODE_CONFIGS])
def test_fwd_cols_modes(pt, name, M):
    """ptycho_cg_fwd_cols_modes: M = 4 and M = 2 are one launch of the NM = 4 / NM = 2 kernel (patch values gathered once for
    all modes), M = 1 the single-probe pass (windowed whatever option window says), M = 7 all three in one call; the summed
    intensity of the M slots against the oracle."""
    import torch
    nat, P_, S_ = nat_mod()
    check_events(name, ("modes", "fwd"))
    c = case(name)
    with pt.CGPtychoSolver(c["nscan"], c["nprb"], c["ndet"], c["ntheta"], c["nz"], c["n"]) as slv:
        h = slv._h
        psi, scan, data = dev(c["psi"][0]), dev(c["scan"]), dev(c["data"])
        keep = [dev(p) for p in mode_probes(name)[:M]]
        ptrs = (ctypes.c_void_p * M)(*[t.data_ptr() for t in keep])
        slv.profile(True)
        nat.check(nat.cg_fwd_cols_modes(h, M, 0, P_(psi), P_(scan), ptrs, 0, 0, S_()))
        ran = {k: n for k, (_, n) in slv.profile_read().items()}
        slv.profile(False)
        assert ran.get("k_cols<FWD>") == {1: 1, 2: 1, 4: 1, 7: 3}[M] and not any(k in ran for k in TILE_KERNELS), ran
        inten = torch.empty(c["data"].shape, dtype=torch.float32, device="cuda")
        sums = zeros64(2)
        nat.check(nat.cg_intensity_modes(h, M, P_(inten), P_(data), P_(sums), S_()))
        got = host(inten)
        for s in range(2 * M):
            slv.release_work(s)
    i64, e32 = mode_intensity(name)[M]
    e = np.abs(got.astype(np.float64) - i64).max() / np.abs(i64).max()
    print("%s M=%d intensity: rel err %.3g, float32 ref %.3g, bound %.3g" % (name, M, e, e32, FACTOR * e32 + REL_MAX))
    assert e <= FACTOR * e32 + REL_MAX, "inten M=%d: rel err %.3g, float32 ref %.3g" % (M, e, e32)
    assert np.all(got[c["skipped"]] == 0), "intensity at a skipped position"


@pytest.mark.parametrize("name", ["rows256", "cols256"])
def test_cg_fwd_cols_window(pt, name):
    """ptycho_cg_fwd_cols with option window on (un-split, as the stages always are), read through ptycho_cg_stats"""
    nat, P_, S_ = nat_mod()
    check_events(name, ("fwd",))
    c = case(name)
    with pt.CGPtychoSolver(c["nscan"], c["nprb"], c["ndet"], c["ntheta"], c["nz"], c["n"]) as slv:
        slv.set_window(True)
        psi, scan, prb, data = dev(c["psi"][0]), dev(c["scan"]), dev(c["probe"]), dev(c["data"])
        slv.profile(True)
        nat.check(nat.cg_fwd_cols(slv._h, 0, P_(psi), P_(scan), P_(prb), S_()))
        ran = {k: n for k, (_, n) in slv.profile_read().items()}
        slv.profile(False)
        assert ran.get("k_cols<FWD>") == 1 and not any(k in ran for k in TILE_KERNELS), ran
        sums = zeros64(2)
        nat.check(nat.cg_stats(slv._h, 0, P_(data), P_(sums), S_()))
        got = host(sums)
        slv.release_work(0)
    want = cs.stats(want_fwd(name, 0), c["data"])
    w32 = cs.stats(want_fwd(name, 0, "single"), c["data"], None, "single")
    for i, what in enumerate(("sum sqrt(I d)", "sum I")):
        check_sum(got[i], want[i], w32[i], want[i], "%s %s" % (name, what))
