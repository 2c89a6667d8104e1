"""The scan-position gradient on the device (``PtychoHIP.adj_scan``, ``ptycho_adj_scan``, csrc/k_scangrad.hpp) and
``PtychoHIP.fwd_autograd``.  Everything here needs a real MI355X: ``pytest -m gpu``.

Tolerance: the rule of tests/hip_common.py through ``check_op``: the device may have ``FACTOR`` = 4 times the error that the
float32 restatement (``scan_grad_ref.adj_scan_ref(..., "single")``; for autograd ``fwd_torch`` in complex64) has against the
float64 one, between the operators' floor and caps.  The geometries, their positions and the references live in
tests/scan_grad_ref.py; tests/test_scan_grad_cpu.py checks the references themselves."""
import ctypes
import functools

import numpy as np
import pytest

import scan_grad_ref as sg
from hip_common import check_op, dev, host, pt, same_bits  # noqa: F401

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def case(ndet, nprb, nscan, ptheta):
    """Inputs and the two references of one geometry, computed once for every test that uses it."""
    c = sg.grad_case(ndet, nprb, nscan, ptheta)
    c["want64"] = sg.adj_scan_ref(c["farplane"], c["scan"], c["psi"], c["probe"], "double")
    c["want32"] = sg.adj_scan_ref(c["farplane"], c["scan"], c["psi"], c["probe"], "single")
    return c


def solver(pt, c, ndet, nprb, nscan, ptheta):
    return pt.PtychoCuFFT(nscan, nprb, ndet, ptheta, c["nz"], c["n"])


@pytest.mark.parametrize("ndet,nprb,nscan,ptheta", sg.GRAD_CASES)
def test_adj_scan_matches_the_formula(pt, ndet, nprb, nscan, ptheta):
    """No pad (16 / 16), pad (32 / 16), two angles with a probe each (64 / 24), Bluestein (100), mixed radix (112), 256 with
    nprb 64 and 256, and 512 / 512 (several items per thread).  Every case holds an exact integer, a -0.3 coordinate, a
    skipped -1.5 coordinate, a patch overhanging the bottom and right edges and a position wholly outside the object."""
    c = case(ndet, nprb, nscan, ptheta)
    with solver(pt, c, ndet, nprb, nscan, ptheta) as slv:
        g, scan, psi, prb = dev(c["farplane"]), dev(c["scan"]), dev(c["psi"]), dev(c["probe"])
        g0 = g.clone()
        got = slv.adj_scan(g, scan, psi, prb)
        assert got.dtype == g.real.dtype and tuple(got.shape) == (ptheta, nscan, 2)
        again = host(slv.adj_scan(g, scan, psi, prb))
        assert same_bits(host(g), host(g0))                      # the farplane is never modified
    got = host(got)
    check_op(got, c["want64"], c["want32"], "adj_scan %d/%d" % (ndet, nprb))
    flat, s = got.reshape(-1, 2), c["special"]
    assert same_bits(flat[s["skipped"]], np.zeros(2, np.float32)) and same_bits(flat[s["outside"]], np.zeros(2, np.float32))
    assert np.all(flat[s["overhang"]] != 0) and np.all(flat[s["negative_fraction"]] != 0) and np.all(flat[s["integer"]] != 0)
    assert same_bits(got, again)                                 # two calls, the same bits


@pytest.mark.parametrize("ndet,nprb,nscan,ptheta", [(32, 16, 7, 1), (64, 24, 33, 2), (100, 20, 6, 1), (256, 64, 9, 1)])
def test_adj_scan_bits_do_not_depend_on_the_chunk(pt, ndet, nprb, nscan, ptheta):
    """``chunk=1``, ``chunk=nscan - 1`` (a last chunk that is not full) and ``chunk=None``; ``out=`` is written in full."""
    import torch
    c = case(ndet, nprb, nscan, ptheta)
    with solver(pt, c, ndet, nprb, nscan, ptheta) as slv:
        g, scan, psi, prb = dev(c["farplane"]), dev(c["scan"]), dev(c["psi"]), dev(c["probe"])
        ref = host(slv.adj_scan(g, scan, psi, prb))
        for chunk in (1, nscan - 1):
            assert same_bits(host(slv.adj_scan(g, scan, psi, prb, chunk=chunk)), ref), chunk
        out = torch.full((ptheta, nscan, 2), float("nan"), dtype=torch.float32, device="cuda")
        assert slv.adj_scan(g, scan, psi, prb, out=out, chunk=2) is out
        assert same_bits(host(out), ref)
        with pytest.raises(ValueError):
            slv.adj_scan(g, scan, psi, prb, chunk=0)


def test_adj_scan_accepts_a_strided_farplane(pt):
    import torch
    ndet, nprb, nscan, ptheta = 32, 16, 7, 1
    c = case(ndet, nprb, nscan, ptheta)
    with solver(pt, c, ndet, nprb, nscan, ptheta) as slv:
        g, scan, psi, prb = dev(c["farplane"]), dev(c["scan"]), dev(c["psi"]), dev(c["probe"])
        wide = torch.zeros((ptheta, nscan, ndet, 2 * ndet), dtype=torch.complex64, device="cuda")
        view = wide[..., ::2]
        view.copy_(g)
        assert not view.is_contiguous()
        assert same_bits(host(slv.adj_scan(view, scan, psi, prb)), host(slv.adj_scan(g, scan, psi, prb)))
        with pytest.raises(ValueError):
            slv.adj_scan(g[:, :-1], scan, psi, prb)


def test_c_abi_rejects_bad_arguments(pt):
    """With a live handle: a null operand, ``work_tiles == 0`` and ``work == g`` return ``PTYCHO_ERR_ARG`` with a message."""
    import torch
    from libtike.hipfft import _native as nat
    ndet, nprb, nscan, ptheta = 32, 16, 7, 1
    c = case(ndet, nprb, nscan, ptheta)
    with solver(pt, c, ndet, nprb, nscan, ptheta) as slv:
        g, scan, psi, prb = dev(c["farplane"]), dev(c["scan"]), dev(c["psi"]), dev(c["probe"])
        out = torch.empty((ptheta, nscan, 2), dtype=torch.float32, device="cuda")
        work = torch.empty((2, ndet, ndet), dtype=torch.complex64, device="cuda")
        good = [out, g, psi, scan, prb, work]
        p = lambda t: ctypes.c_void_p(t.data_ptr())
        for k in range(len(good)):
            args = [None if i == k else p(t) for i, t in enumerate(good)]
            assert nat.adj_scan(slv._h, *args, 2, None) == 1, k
            assert b"null operand" in nat.last_error()
        assert nat.adj_scan(slv._h, *[p(t) for t in good], 0, None) == 1
        assert b"work_tiles" in nat.last_error()
        assert nat.adj_scan(slv._h, p(out), p(g), p(psi), p(scan), p(prb), p(g), 2, None) == 1
        assert b"work must not be g" in nat.last_error()
        assert nat.adj_scan(slv._h, *[p(t) for t in good], 2, None) == 0
        torch.cuda.synchronize()
        assert same_bits(host(out), host(slv.adj_scan(g, scan, psi, prb)))


# ---- autograd -------------------------------------------------------------------------------------------------------------------
def masked_loss(mask, sqrt_d):
    import torch
    return lambda farplane: (mask * (torch.abs(farplane) - sqrt_d) ** 2).sum()


@functools.lru_cache(maxsize=None)
def autograd_case(ndet, nprb, nscan, ptheta):
    """The geometry's inputs, a mask and data, and the gradients of ``sum m (|G| - sqrt d)^2`` by the restated ``fwd`` in
    float64 and float32."""
    import torch
    c = dict(sg.grad_case(ndet, nprb, nscan, ptheta, seed=1))
    rng = np.random.default_rng(ndet + nprb)
    shape = (ptheta, nscan, ndet, ndet)
    c["mask"] = (rng.random(shape) < 0.8).astype(np.float32)
    c["sqrt_d"] = (np.sqrt(ndet) * rng.random(shape) * 4).astype(np.float32)
    for name, precision, rt in (("want64", "double", torch.float64), ("want32", "single", torch.float32)):
        loss = masked_loss(torch.tensor(c["mask"], dtype=rt), torch.tensor(c["sqrt_d"], dtype=rt))
        c[name] = sg.torch_grads(loss, c["psi"], c["scan"], c["probe"], ndet, precision)
    return c


@pytest.mark.parametrize("ndet,nprb,nscan,ptheta", [(32, 16, 7, 1), (64, 24, 33, 2)])
def test_autograd_gradients_match_the_restated_fwd(pt, ndet, nprb, nscan, ptheta):
    """``psi.grad``, ``probe.grad`` and ``scan.grad`` of a masked amplitude loss; then only ``scan`` and only ``psi``
    requiring a gradient (the same values, nothing for the others); and the value of ``fwd_autograd`` is ``fwd``'s."""
    c = autograd_case(ndet, nprb, nscan, ptheta)
    loss = masked_loss(dev(c["mask"]), dev(c["sqrt_d"]))
    tag = "autograd %d/%d " % (ndet, nprb)
    with solver(pt, c, ndet, nprb, nscan, ptheta) as slv:
        def leaves(*wrt):
            t = dict(psi=dev(c["psi"]), scan=dev(c["scan"]), probe=dev(c["probe"]))
            for name in wrt:
                t[name].requires_grad_(True)
            return t

        t = leaves("psi", "scan", "probe")
        g = slv.fwd_autograd(t["psi"], t["scan"], t["probe"])
        assert g.requires_grad and g.grad_fn is not None
        plain = slv.fwd(t["psi"], t["scan"], t["probe"])
        assert not plain.requires_grad and same_bits(host(g), host(plain))
        loss(g).backward()
        full = {}
        for k, name in enumerate(("psi", "scan", "probe")):
            full[name] = host(t[name].grad)
            assert t[name].grad.dtype == t[name].dtype and t[name].grad.shape == t[name].shape
            check_op(full[name], c["want64"][k], c["want32"][k], tag + name + ".grad")
        skipped = c["special"]["skipped"]
        assert same_bits(full["scan"].reshape(-1, 2)[skipped], np.zeros(2, np.float32))

        for only in ("scan", "psi"):
            t = leaves(only)
            loss(slv.fwd_autograd(t["psi"], t["scan"], t["probe"])).backward()
            assert all((t[name].grad is None) == (name != only) for name in t), only
            if only == "scan":
                assert same_bits(host(t[only].grad), full[only])       # adj_scan: a fixed summation order
            else:                                                       # adj adds with float atomics: not the same bits
                check_op(host(t[only].grad), c["want64"][0], c["want32"][0], tag + "psi.grad alone")

        t = leaves()
        assert not slv.fwd_autograd(t["psi"], t["scan"], t["probe"]).requires_grad


def test_autograd_accepts_a_lazily_conjugated_gradient(pt):
    """``backward`` with a gradient that is a conjugate view: resolved before pointers are taken."""
    import torch
    ndet, nprb, nscan, ptheta = 32, 16, 7, 1
    c = case(ndet, nprb, nscan, ptheta)
    with solver(pt, c, ndet, nprb, nscan, ptheta) as slv:
        scan, psi, prb = dev(c["scan"]).requires_grad_(True), dev(c["psi"]), dev(c["probe"])
        gbar = torch.conj(dev(np.conj(c["farplane"])))
        assert gbar.is_conj()
        slv.fwd_autograd(psi, scan, prb).backward(gbar)
        assert same_bits(host(scan.grad), host(slv.adj_scan(dev(c["farplane"]), scan.detach(), psi, prb)))


def test_positions_are_recovered_by_adam_on_scan_alone(pt):
    """End to end (``scan_grad_ref.refine_scenario``): object and probe known, positions off by uniform +-0.45 px, Adam
    (lr 0.05, 80 steps) on ``scan`` through ``fwd_autograd``; the rms position error must fall to at most half its start.
    Measured: float64 restatement on the CPU 0.3682 -> 0.0037 px (ratio 0.010, loss 3.069 -> 2.2e-4); on an MI355X
    0.3682 -> 0.0037 px (ratio 0.010, loss 3.069 -> 2.2e-4)."""
    import torch
    s = sg.refine_scenario()
    e0 = sg.rms_error(s["scan_start"], s["scan_true"])
    with pt.PtychoCuFFT(64, s["nprb"], s["ndet"], 1, s["nz"], s["n"]) as slv:
        psi, prb, scan = dev(s["psi"]), dev(s["probe"]), dev(s["scan_start"])
        sqrt_d = dev(np.sqrt(s["data"]).astype(np.float32))
        losses = sg.refine(lambda x: slv.fwd_autograd(psi, x, prb), scan, sqrt_d)
        torch.cuda.synchronize()
    e1 = sg.rms_error(host(scan), s["scan_true"])
    print("refine (device): rms %.4f -> %.4f px (ratio %.3f), loss %.4g -> %.4g" % (e0, e1, e1 / e0, losses[0], losses[-1]))
    assert e1 <= 0.5 * e0, (e0, e1)
