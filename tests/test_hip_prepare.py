"""Frame preparation on the GPU (csrc/k_prepare.hpp, ``libtike.hipfft.prepare``) against the NumPy restatement of
tests/prepare_ref.py: ``data`` and ``mask`` bit for bit, maxima and saturation counts exactly, the float64 sums within
``N * 2^-52 * mag`` (``N`` terms of absolute sum ``mag``: the bound of float64 summation in any order); the bitwise
guarantees, the load paths, the mask rules, the input variants, ``initial_probe`` and the chain into ``run``.
"""
import os
import sys
import warnings

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prepare_ref as ref  # noqa: E402
from hip_common import dev, pt, same_bits  # noqa: E402, F401

pytestmark = pytest.mark.gpu


_cases = {}


def case(name):
    """Inputs and restatement of one case, computed once; the tests copy before they plant anything."""
    if name not in _cases:
        raw, kw = ref.make_case(name)
        _cases[name] = (raw, kw, ref.prepare(raw, **kw))
    return _cases[name]


def host(out):              # not hip_common.host: a dict of tensors, some of them None
    return {k: None if v is None else v.cpu().numpy() for k, v in out.items()}


def assert_same_outputs(a, b):
    for key in ("data", "mask", "frames", "pixels"):
        assert same_bits(a[key], b[key]), key


def assert_matches(got, want, ndet, nscan):
    """The comparison of the module docstring."""
    assert got["data"].dtype == np.float32 and got["mask"].dtype == np.uint8
    assert same_bits(got["data"], want["data"]) and same_bits(got["mask"], want["mask"])
    f, p = got["frames"], got["pixels"]
    assert f.dtype == np.float64 and p.dtype == np.float64
    assert np.array_equal(f[..., 2:], want["frames"][..., 2:], equal_nan=True)       # maximum, saturation count
    assert np.array_equal(p[:, 2:], want["pixels"][:, 2:], equal_nan=True)
    worst = []
    for col in (0, 1):
        for g, w, m, n in ((f[..., col], want["frames"][..., col], want["frames_mag"][..., col], ndet * ndet),
                           (p[:, col], want["pixels"][:, col], want["pixels_mag"][:, col], nscan)):
            fin = np.isfinite(w) & np.isfinite(g) & (m > 0)
            worst.append(float((np.abs(g[fin] - w[fin]) / (m[fin] * 2.0 ** -52)).max()) if fin.any() else 0.0)
            assert ref.sums_close(g, w, m, n), (col, n)
    return worst


# ---- 1. against the restatement --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(ref.CASES))
def test_device_matches_the_restatement(pt, name):
    raw, kw, want = case(name)
    got = host(pt.prepare_frames(raw, **kw))
    ptheta, nscan, ndet = ref.CASES[name]
    worst = assert_matches(got, want, ndet, nscan)
    print("prepare %s  sums against the restatement, in units of 2^-52 x magnitude: frames %.2f %.2f (bound %d), pixels "
          "%.2f %.2f (bound %d)" % (name, worst[0], worst[2], ndet * ndet, worst[1], worst[3], nscan))


@pytest.mark.parametrize("name", ["B", "C", "E", "F"])
def test_same_inputs_same_bits_and_pixels_do_not_touch_the_rest(pt, name):
    raw, kw, _ = case(name)
    raw_d = dev(raw)
    a, b = host(pt.prepare_frames(raw_d, **kw)), host(pt.prepare_frames(raw_d, **kw))
    assert_same_outputs(a, b)
    c = host(pt.prepare_frames(raw_d, pixels=False, **kw))
    assert c["pixels"] is None
    for key in ("data", "mask", "frames"):
        assert same_bits(a[key], c[key])


# ---- 2. alignment and mask robustness ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["F", "A", "C", "G", "H"])
def test_a_view_shifted_by_one_element_gives_the_same_bits(pt, name):
    """One element into an allocation the raw frames cannot be read with vector loads (A, C, G, H otherwise are), and the
    scalar loads of F start on another byte; ``out`` shifted by one float takes the 4-byte stores."""
    import torch
    raw, kw, want = case(name)
    raw_d = dev(raw)
    shifted = torch.empty(raw_d.numel() + 1, dtype=raw_d.dtype, device="cuda")[1:].view(raw_d.shape)
    shifted.copy_(raw_d)
    assert shifted.data_ptr() % (4 * raw_d.element_size()) == raw_d.element_size() and shifted.is_contiguous()
    a, b = host(pt.prepare_frames(raw_d, **kw)), host(pt.prepare_frames(shifted, **kw))
    assert_same_outputs(a, b)
    assert same_bits(a["data"], want["data"])
    out = torch.empty(a["data"].size + 1, dtype=torch.float32, device="cuda")[1:].view(a["data"].shape)
    assert out.data_ptr() % 16 == 4
    c = host(pt.prepare_frames(raw_d, out=out, **kw))
    assert_same_outputs(a, c)


def test_unmeasured_raw_pixels_may_hold_anything(pt):
    raw, kw, want = case("C")
    a = host(pt.prepare_frames(raw, **kw))
    assert np.isfinite(a["data"]).all() and np.isfinite(a["frames"]).all() and np.isfinite(a["pixels"]).all()
    ys, xs = np.nonzero(kw["bad"])
    for garbage in (np.nan, -np.inf, 1e30):
        raw2, dark2, gain2 = raw.copy(), kw["dark"].copy(), kw["gain"].copy()
        raw2[:, ys, xs], dark2[ys, xs], gain2[ys, xs] = garbage, np.nan, garbage
        assert_same_outputs(a, host(pt.prepare_frames(raw2, **{**kw, "dark": dark2, "gain": gain2})))


@pytest.mark.parametrize("value", [np.nan, np.inf])
def test_a_non_finite_value_at_a_measured_pixel_stays_in_its_pixel_and_frame(pt, value):
    raw, kw, _ = case("C")
    raw = raw.copy()
    frame, y, x = 101, 20, 9                                            # in the second frame range; not a bad pixel
    assert not kw["bad"][y, x]
    raw[frame, y, x] = value
    want = ref.prepare(raw, **kw)
    got = host(pt.prepare_frames(raw, **kw))
    assert_matches(got, want, 16, raw.shape[0])
    odd = ~np.isfinite(got["data"])
    assert odd.sum() == 1 and odd[0, frame].sum() == 1
    r, c = np.argwhere(odd[0, frame])[0]
    assert ((r + 8) % 16, (c + 8) % 16) == (y // 2, x // 2)
    bad_rows = ~np.isfinite(got["frames"]).all(-1)
    assert bad_rows.sum() == 1 and bad_rows[0, frame]
    bad_pix = ~np.isfinite(got["pixels"]).all(1)
    assert bad_pix.sum() == 1 and bad_pix[0, r, c]
    assert np.isfinite(got["frames"][0, frame, 2]) or value == np.inf   # the maximum skips a NaN


# ---- 3. input variants -----------------------------------------------------------------------------------------------------
def test_no_index_is_the_identity_index(pt):
    raw, kw, _ = case("H")
    index = np.broadcast_to(np.arange(raw.shape[1], dtype=np.int64), raw.shape[:2]).copy()
    assert_same_outputs(host(pt.prepare_frames(raw, **kw)), host(pt.prepare_frames(raw, index=index, **kw)))
    raw, kw, _ = case("F")
    assert_same_outputs(host(pt.prepare_frames(raw, **kw)),
                        host(pt.prepare_frames(raw, index=dev(np.arange(raw.shape[0], dtype=np.int64)), **kw)))


def test_an_index_out_of_range_gives_a_zero_frame_and_leaves_its_neighbours(pt):
    raw, kw, _ = case("B")
    got = host(pt.prepare_frames(raw, **kw))
    for t, j in ((0, 2), (1, 1)):
        assert not got["data"][t, j].any() and not got["frames"][t, j].any()
    inside = kw["index"].copy()
    inside[0, 2], inside[1, 1] = 1, 2
    full = host(pt.prepare_frames(raw, **{**kw, "index": inside}))
    for t, j in ((0, 0), (0, 1), (1, 0), (1, 2)):
        assert same_bits(got["data"][t, j], full["data"][t, j]) and same_bits(got["frames"][t, j], full["frames"][t, j])
    assert full["data"][0, 2].any() and full["frames"][1, 1, 0] != 0
    assert same_bits(got["mask"], full["mask"])


@pytest.mark.parametrize("name", ["B", "D", "E"])
def test_numpy_and_device_inputs_give_the_same_bits(pt, name):
    raw, kw, _ = case(name)
    kw_d = {k: dev(v) if isinstance(v, np.ndarray) else v for k, v in kw.items()}
    assert_same_outputs(host(pt.prepare_frames(raw, **kw)), host(pt.prepare_frames(dev(raw), **kw_d)))


def test_out_is_written_in_place(pt):
    import torch
    raw, kw, want = case("E")
    out = torch.full(want["data"].shape, float("nan"), dtype=torch.float32, device="cuda")
    res = pt.prepare_frames(raw, out=out, **kw)
    assert res["data"] is out and same_bits(out.cpu().numpy(), want["data"])
    with pytest.raises(ValueError, match="contiguous tensor on raw's device"):
        pt.prepare_frames(raw, out=out.cpu(), **kw)


def test_the_call_does_not_wait_for_the_device(pt):
    """With device inputs nothing synchronises: the call returns while work queued before it on the stream is still
    running, so an event recorded after the call has not completed when the call is back."""
    import torch
    raw, kw, want = case("F")
    raw_d = dev(raw)
    pt.prepare_frames(raw_d, **kw)                                      # first call: the kernels are loaded
    torch.cuda.synchronize()
    done = torch.cuda.Event()
    torch.cuda._sleep(200_000_000)                                      # the device spins for about 0.1 s; the host does not
    res = pt.prepare_frames(raw_d, **kw)
    done.record()
    pending = not done.query()
    torch.cuda.synchronize()
    assert pending
    assert same_bits(res["data"].cpu().numpy(), want["data"])


# ---- 4. initial_probe ------------------------------------------------------------------------------------------------------
def known_probe(ndet):
    y = np.linspace(-2, 2, ndet)
    env = np.exp(-(y[:, None] ** 2 + y[None, :] ** 2))
    rng = np.random.default_rng(8)
    return (env * (1 + 0.2 * rng.standard_normal((ndet, ndet))) * np.exp(0.5j * rng.standard_normal((ndet, ndet)))
            ).astype(np.complex64)[None]


def test_initial_probe_reproduces_its_pattern(pt):
    import torch
    ndet, nscan = 32, 4
    scan = dev(np.array([[[0, 0], [3.5, 1.25], [7, 2], [1, 6.75]]], np.float32))
    with pt.PtychoHIP(nscan, ndet, ndet, 1, ndet + 8, ndet + 8) as op:
        ones = torch.ones((1, ndet + 8, ndet + 8), dtype=torch.complex64, device="cuda")
        far = op.fwd(ones, scan, dev(known_probe(ndet)))
        pattern = (far.real * far.real + far.imag * far.imag)[:, 0].contiguous()          # [1, ndet, ndet], data layout
        probe = pt.initial_probe(pattern, ndet)
        assert probe.shape == (1, 1, ndet, ndet) and probe.dtype == torch.complex64 and probe.is_cuda
        again = op.fwd(ones, scan, probe[:, 0].contiguous())
        inten = (again.real * again.real + again.imag * again.imag).cpu().numpy()
    pat = pattern.cpu().numpy()
    bound = 16 * 2.0 ** -23 * pat.max()
    err = np.abs(inten - pat[:, None]).max()
    print("initial_probe: |fwd|^2 against the pattern, worst %.3e, bound %.3e" % (err, bound))
    assert err <= bound
    small = pt.initial_probe(pattern, 16)
    assert small.shape == (1, 1, 16, 16) and torch.equal(small, probe[:, :, 8:24, 8:24])
    scaled = pt.initial_probe(pat, 16, power=5.0)                                         # NumPy input
    assert float((scaled.abs() ** 2).sum()) == pytest.approx(5.0, rel=1e-5)
    ratio = (scaled / small).cpu().numpy()
    assert np.allclose(ratio, ratio.flat[0], rtol=1e-5) and abs(ratio.flat[0].imag) < 1e-6


# ---- 5. end to end ---------------------------------------------------------------------------------------------------------
def test_prepared_frames_run_as_the_restatements_do(pt):
    import torch
    import libtike.hipfft.synthetic as syn
    ndet = 32
    p = syn.make_problem(4, 4, 6, ndet, ndet, seed=31)
    nscan = p["nscan"]
    assert nscan == 16
    rng = np.random.default_rng(32)
    with pt.CGPtychoSolver(nscan, ndet, ndet, 1, p["nz"], p["n"]) as slv:
        slv.verbose = False
        scan, probe = dev(p["scan"]), dev(p["probe"])
        far = slv.fwd(dev(p["psi"]), scan, probe).cpu().numpy()
        inten = np.abs(far.astype(np.complex128)) ** 2
        counts = np.minimum(np.rint(inten * (3000.0 / inten.max())), 65000).astype(np.uint16)[0]   # operators' layout
        dark = (20 + 5 * rng.random((48, 40))).astype(np.float32)
        raw = np.rint(np.broadcast_to(dark, (nscan, 48, 40))).astype(np.uint16)
        cy, cx = 25, 21
        raw[:, cy - 16:cy + 16, cx - 16:cx + 16] += np.fft.fftshift(counts, axes=(-2, -1))   # stored centred
        bad = np.zeros((48, 40), np.uint8)
        bad[cy + 3, cx - 5] = bad[cy - 9, cx + 2] = 1
        kw = dict(ndet=ndet, center=(cy, cx), dark=dark, bad=bad, scale=1.0 / 3000.0)
        want = ref.prepare(raw, **kw)
        assert (want["mask"] == 0).sum() == 2 and want["data"].max() > 0.5
        got = pt.prepare_frames(raw, **kw)
        assert same_bits(got["data"].cpu().numpy(), want["data"]) and same_bits(got["mask"].cpu().numpy(), want["mask"])
        results = []
        for data, mask in ((got["data"], got["mask"]), (dev(want["data"]), want["mask"])):
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                res = slv.run(data, dev(np.ones_like(p["psi"])), dev(p["scan"].copy()), dev(p["probe"][:, None].copy()), piter=4,
                              mask=mask)
            torch.cuda.synchronize()
            results.append((res["psi"].cpu().numpy(), res["probe"].cpu().numpy()))
    assert same_bits(results[0][0], results[1][0]) and same_bits(results[0][1], results[1][1])
    assert np.isfinite(results[0][0]).all() and not np.array_equal(results[0][0], np.ones_like(p["psi"]))
