"""Free-space propagation on the GPU (``libtike.hipfft.propagate``, csrc/k_propagate.hpp) against the float64
restatement of tests/propagate_ref.py and the analytic Gaussian beam.

Tolerances.  A plane's error is the max-norm of its difference from the float64 restatement over ``max |want|``.  The
device may be ``FACTOR`` times the complex64 restatement's own error off (with the floor ``FLOOR`` where complex64
happens to be almost exact), and never more than ``CAP``; a wrong phase reduction or a wrong tile mapping gives errors of
order 1.  Observed: 1.8e-7 ... 3.2e-7 on the sides with a plan, 5.9e-7 at 100 (Bluestein), against 7e-8 ... 9e-8 of the
complex64 restatement; the floor is 3.4 times the largest.  The eight figures are compared with the restatement's ``metrics`` of the DEVICE's planes: they are float64 sums
of the same float32 values, so the sums agree to ``SUM_TOL`` (the order of the additions is all that differs; n eps / 2
of a sum of n <= 65536 non-negative terms is 7e-12 at the very worst and 1e-15 typically) and the maximum and its index
are equal.  The observed errors behind these figures are in profiles/r15/propagate.txt.
"""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import propagate_ref as ref  # noqa: E402
from hip_common import bound, dev, pt  # noqa: E402, F401

pytestmark = pytest.mark.gpu

FLOOR = 2e-6
CAP = 1e-5
SUM_TOL = 1e-12
LAM, PIX = 0.05, 1.0
METHODS = ("fresnel", "angular")


@pytest.fixture(scope="module")
def lib(pt):
    return sys.modules["libtike.hipfft.propagate"]


def rel_err(got, want):     # not hip_common.rel_max: the difference in the arrays' own precision (complex64 against complex64)
    return np.abs(got - want).max() / np.abs(want).max()


def distances(S):
    """0, +z, -z, a fraction of z, and a distance whose phase at the corner of the band is about 1e7 turns."""
    z = 0.6 * S * PIX ** 2 / LAM
    q_corner = (LAM / (S * PIX)) ** 2 * (S * S / 2.0)
    return np.array([0.0, z, -z, 0.37 * z, 1e7 / q_corner * LAM])


def fields(nf, S, seed):
    rng = np.random.default_rng(seed)
    return (rng.standard_normal((nf, S, S)) + 1j * rng.standard_normal((nf, S, S))).astype(np.complex64)


def native(pt, z, lam, pix, method, S, field=None, spec=None, tile=True, planes=True, metrics=True):
    """One ``ptycho_propagate`` call on a handle of its own: host ``(planes [nf, D, S, S], metrics [nf, D, 8])``."""
    import torch
    nat = sys.modules["libtike.hipfft._native"]
    ops = sys.modules["libtike.hipfft.operators"]
    z = np.atleast_1d(np.asarray(z, dtype=np.float64))
    nf, nd = (field if spec is None else spec).shape[0], z.shape[0]
    with pt.PtychoHIP(nf, S, S, 1, S + 2, S + 2) as op:
        op.set_tile(tile)
        sp = op.fft2(dev(field)) if spec is None else dev(np.ascontiguousarray(spec, dtype=np.complex64))
        zl = dev(z / lam)
        words = int(nat.propagate_work_words(op._h, nf, nd, int(planes)))
        fused = tile and S <= 128 and S in (16, 32, 48, 64, 80, 96, 112, 128)
        assert words == (0 if planes or fused else nf * nd * S * S)
        work = torch.empty(max(words, 2), dtype=torch.float64, device="cuda")
        out = torch.full((nf, nd, S, S), np.nan, dtype=torch.complex64, device="cuda") if planes else None
        met = torch.full((nf, nd, 8), np.nan, dtype=torch.float64, device="cuda") if metrics else None
        ptr = lambda t: None if t is None else ctypes.c_void_p(t.data_ptr())  # noqa: E731
        nat.check(nat.propagate(op._h, ptr(out), ptr(met), ptr(sp), nf, ptr(zl), nd, (lam / (S * pix)) ** 2,
                                nat.PROPAGATE_METHODS[method], ptr(work), ops._stream()))
        torch.cuda.synchronize()
    return (None if out is None else out.cpu().numpy()), (None if met is None else met.cpu().numpy())


def check_metrics(got, planes):
    """``got`` ``[nf, D, 8]`` against the restatement's metrics of the device's own ``planes``; returns the worst sum error."""
    worst = 0.0
    for f in range(planes.shape[0]):
        for d in range(planes.shape[1]):
            want = ref.metrics(planes[f, d])
            with np.errstate(divide="ignore", invalid="ignore"):
                e = np.where(want[:6] == 0, (got[f, d, :6] != 0) * 1.0, np.abs(got[f, d, :6] - want[:6]) / np.abs(want[:6]))
            worst = max(worst, e.max())
            assert e.max() <= SUM_TOL, (f, d, got[f, d], want)
            assert got[f, d, 6] == want[6] and got[f, d, 7] == want[7], (f, d, got[f, d], want)
    return worst


# S, fields, tile option: 16 x 37 fields x 5 distances = 185 pairs: a dozen trips of a workgroup's 16 tiles, the last one
# partly idle, four tiles to a wave; 15 pairs at 32 leave one of the last workgroup's four tiles idle
CASES = [(16, 37, True), (32, 3, True), (48, 3, True), (64, 3, True), (112, 2, True), (128, 2, True),
         (16, 5, False), (32, 3, False), (48, 2, False), (64, 2, False), (112, 2, False), (128, 2, False),
         (192, 2, True), (256, 2, True), (100, 2, True)]


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("S,nf,tile", CASES)
def test_planes_and_metrics_match_the_restatement(pt, S, nf, tile, method):
    u = fields(nf, S, seed=S + nf)
    z = distances(S)
    planes, met = native(pt, z, LAM, PIX, method, S, field=u, tile=tile)
    assert not np.isnan(planes).any() and not np.isnan(met).any()
    worst, worst32 = 0.0, 0.0
    for d, zz in enumerate(z):
        want = ref.propagate(u, zz, LAM, PIX, method)
        e32 = rel_err(ref.propagate(u, zz, LAM, PIX, method, precision="single"), want)
        e = rel_err(planes[:, d], want)
        worst, worst32 = max(worst, e), max(worst32, e32)
        assert e <= bound(e32, FLOOR, CAP), (d, zz, e, e32)
    assert rel_err(planes[:, 0], u) <= bound(worst32, FLOOR, CAP)           # z = 0 returns the field
    esum = check_metrics(met, planes)
    print("S %d fields %d tile %s %s: plane err %.2e (complex64 restatement %.2e), sums err %.1e"
          % (S, nf, tile, method, worst, worst32, esum))
    # the call without planes gives the same bits, and so does a second run
    _, met2 = native(pt, z, LAM, PIX, method, S, field=u, tile=tile, planes=False)
    assert np.array_equal(met, met2)
    planes3, met3 = native(pt, z, LAM, PIX, method, S, field=u, tile=tile)
    assert np.array_equal(planes, planes3) and np.array_equal(met, met3)


def test_thirty_seven_pairs_at_16(pt):
    """One distance, 37 fields: three trips of 16 tiles, five live tiles in the last."""
    u = fields(37, 16, seed=5)
    z = distances(16)[1:2]
    planes, met = native(pt, z, LAM, PIX, "fresnel", 16, field=u)
    want = ref.propagate(u, z[0], LAM, PIX)
    assert rel_err(planes[:, 0], want) <= bound(rel_err(ref.propagate(u, z[0], LAM, PIX, precision="single"), want), FLOOR, CAP)
    check_metrics(met, planes)
    _, only = native(pt, z, LAM, PIX, "fresnel", 16, field=u, planes=False)
    assert np.array_equal(only, met)


@pytest.mark.parametrize("S,tile", [(16, True), (32, True), (128, True), (64, False), (256, True)])
def test_duplicated_maximum(pt, S, tile):
    """A spectrum that is nonzero in row ky = 0 only: the row transform leaves one nonzero row, and the column transform
    of a column whose only nonzero entry is its first one copies it to every y exactly (every twiddle it meets is 1).  So
    at z = 0 every row of the plane holds the same bits and the maximum is there S times: the first one, in row 0, is
    the answer.  Field 0: a constant row, the peak in column 0; field 1: a ramp that puts it in column S - 3."""
    x0 = S - 3
    spec = np.zeros((2, S, S), dtype=np.complex64)
    spec[0, 0, :] = 1.0
    spec[1, 0, :] = np.exp(-2j * np.pi * np.fft.fftfreq(S) * x0)
    planes, met = native(pt, [0.0], LAM, PIX, "fresnel", S, spec=spec, tile=tile)
    for f, col in ((0, 0), (1, x0)):
        v = ref.intensity32(planes[f, 0])
        assert np.all(v == v[0][None, :]), "the rows of the plane differ: the test's premise does not hold"
        assert np.count_nonzero(v == v.max()) == S and v[0, col] == v.max()
        assert met[f, 0, 7] == col and met[f, 0, 6] == v.max()
    check_metrics(met, planes)
    _, only = native(pt, [0.0], LAM, PIX, "fresnel", S, spec=spec, tile=tile, planes=False)
    assert np.array_equal(only, met)


def test_fused_and_two_pass_agree_at_64(pt):
    u = fields(3, 64, seed=64)
    z = distances(64)
    for method in METHODS:
        a, _ = native(pt, z, LAM, PIX, method, 64, field=u, tile=True, metrics=False)
        b, _ = native(pt, z, LAM, PIX, method, 64, field=u, tile=False, metrics=False)
        for d, zz in enumerate(z):
            want = ref.propagate(u, zz, LAM, PIX, method)
            e32 = rel_err(ref.propagate(u, zz, LAM, PIX, method, precision="single"), want)
            assert np.abs(a[:, d] - b[:, d]).max() / np.abs(want).max() <= bound(e32, FLOOR, CAP)


def power_bound(want, b):
    """|d power| / power <= 2 ||d plane||_2 / ||plane||_2 <= 2 b max|plane| S / ||plane||_2 for a max-norm error b."""
    S = want.shape[-1]
    return 2.0 * b * np.abs(want).max() * S / np.sqrt((np.abs(want) ** 2).sum(axis=(-2, -1)).min())


def test_round_trip_and_power(pt):
    import torch
    S = 64
    u = fields(2, S, seed=11)
    z = distances(S)[1]
    tu = dev(u)
    fwd = pt.propagate(tu, z, LAM, PIX)
    assert fwd.shape == tu.shape and fwd.dtype == torch.complex64
    back = pt.propagate(fwd, -z, LAM, PIX).cpu().numpy()
    want = ref.propagate(u, z, LAM, PIX)
    e32 = rel_err(ref.propagate(u, z, LAM, PIX, precision="single"), want)
    e1, e = rel_err(fwd.cpu().numpy(), want), rel_err(back, u)
    print("one way err %.2e, round trip err %.2e (complex64 restatement, one way, %.2e)" % (e1, e, e32))
    assert e1 <= bound(e32, FLOOR, CAP)
    assert e <= 2 * bound(e32, FLOOR, CAP) * max(1.0, np.abs(want).max() / np.abs(u).max())   # two calls, each within its bound
    assert rel_err(pt.propagate(tu, 0.0, LAM, PIX).cpu().numpy(), u) <= bound(e32, FLOOR, CAP)
    # Fresnel: |H| = 1, the power is that of the field at every distance
    zs = distances(S)
    fs = pt.focus_series(tu, zs, LAM, PIX)
    p0 = (np.abs(u.astype(np.complex128)) ** 2).sum(axis=(-2, -1))
    b = power_bound(u, bound(e32, FLOOR, CAP))
    dp = np.abs(fs["power"] / p0[:, None] - 1.0).max()
    print("fresnel power drift %.2e (bound %.2e)" % (dp, b))
    assert dp <= b
    # angular spectrum with lambda = 1.9 p: q > 1 beyond |k| = 0.526 S (the band's corners, 14 % of it): evanescent, dropped
    lam = 1.9 * PIX
    assert not ref.turns(S, 1.0, (lam / (S * PIX)) ** 2, "angular")[1].all()
    fa = pt.focus_series(tu, [3.0, -3.0], lam, PIX, method="angular")
    want = np.stack([ref.propagate(u, zz, lam, PIX, "angular") for zz in (3.0, -3.0)], axis=1)
    share = (np.abs(want) ** 2).sum(axis=(-2, -1)) / p0[:, None]
    assert share.max() < 0.95
    da = np.abs(fa["power"] / p0[:, None] - share).max()
    print("angular power share %s, off by %.2e" % (share[:, 0].tolist(), da))
    assert da <= power_bound(want, bound(e32, FLOOR, CAP))


def test_analytic_gaussian(pt):
    S = 64
    w0 = 4 * PIX
    zr = ref.rayleigh(w0, LAM)
    u0 = ref.gaussian_beam(S, w0, LAM, PIX, 0.0)
    for method in METHODS:
        for z in (0.5 * zr, -0.8 * zr):
            got = pt.propagate(u0, z, LAM, PIX, method=method).cpu().numpy()
            want = ref.gaussian_beam(S, w0, LAM, PIX, z) if method == "fresnel" else ref.propagate(u0, z, LAM, PIX, method)
            e32 = rel_err(ref.propagate(u0, z, LAM, PIX, method, precision="single"), want)
            e = rel_err(got, want)
            print("gaussian %s z / zR %+.1f: err %.2e (complex64 restatement %.2e)" % (method, z / zr, e, e32))
            assert e <= bound(e32, FLOOR, CAP)


def test_focus_series_finds_the_waist(pt):
    S = 64
    w0 = 3 * PIX
    zr = ref.rayleigh(w0, LAM)
    u0 = ref.gaussian_beam(S, w0, LAM, PIX, 0.7 * zr)
    z = np.linspace(-1.4 * zr, 0.0, 29)
    step = z[1] - z[0]
    fs = pt.focus_series(u0.astype(np.complex64), z, LAM, PIX)
    m = np.stack([ref.metrics(ref.propagate(u0.astype(np.complex64), zz, LAM, PIX)) for zz in z])
    b, f, ok = ref.focus(z, ref.sharpness(m))
    off = abs(float(fs["focus"]) - f) / step
    print("focus %.6f of a step off the restatement's (cap 0.02), sharpness err %.1e"
          % (off, np.abs(fs["sharpness"] / ref.sharpness(m) - 1).max()))
    assert fs["best"] == b == 14 and bool(fs["bracketed"]) and ok
    assert off <= 0.02
    assert fs["width"][b] == pytest.approx(w0 / np.sqrt(2), rel=1e-4)
    assert fs["sampled"].all() and fs["distance"].tolist() == z.tolist()
    assert np.array_equal(fs["peak_index"][b], [S // 2, S // 2])


def test_shapes_padding_and_chunks(pt, lib, monkeypatch):
    import torch
    rng = np.random.default_rng(3)
    s, S, lo = 40, 64, 12
    yy, xx = np.mgrid[:s, :s]
    blob = np.exp(-((yy - 25.0) ** 2 + (xx - 13.0) ** 2) / 8.0)
    u = (blob * np.exp(1j * rng.uniform(0, 0.3, (2, 3, s, s)))).astype(np.complex64)
    z = np.array([0.0, 150.0, -90.0])
    got = pt.propagate(dev(u), z, LAM, PIX, size=S)
    assert tuple(got.shape) == (2, 3, 3, s, s)
    padded = np.zeros((2, 3, S, S), dtype=np.complex64)
    padded[..., lo:lo + s, lo:lo + s] = u
    for d, zz in enumerate(z):
        want = ref.propagate(padded, zz, LAM, PIX)
        e32 = rel_err(ref.propagate(padded, zz, LAM, PIX, precision="single"), want)
        assert rel_err(got[:, :, d].cpu().numpy(), want[..., lo:lo + s, lo:lo + s]) <= bound(e32, FLOOR, CAP)
    fs = pt.focus_series(dev(u), z, LAM, PIX, size=S, planes=True)
    assert fs["power"].shape == (2, 3, 3) and fs["peak_index"].shape == (2, 3, 3, 2) and fs["best"].shape == (2, 3)
    assert np.array_equal(fs["peak_index"][:, :, 0], np.broadcast_to([25, 13], (2, 3, 2)))     # field coordinates
    assert np.abs(fs["centroid"][:, :, 0] - [25.0, 13.0]).max() < 1e-3
    assert torch.equal(fs["planes"], got) and fs["planes"].is_cuda
    # a NumPy input, a scalar distance, a 2-D field: the same bits
    assert torch.equal(pt.propagate(u, z, LAM, PIX, size=S), got)
    one = pt.propagate(dev(u), float(z[1]), LAM, PIX, size=S)
    assert tuple(one.shape) == (2, 3, s, s) and torch.equal(one, got[:, :, 1])
    flat = pt.propagate(dev(u[1, 2]), z, LAM, PIX, size=S)
    assert tuple(flat.shape) == (3, s, s) and torch.equal(flat, got[1, 2])
    f2 = pt.focus_series(u[1, 2], z, LAM, PIX, size=S)
    assert f2["power"].shape == (3,) and np.array_equal(f2["power"], fs["power"][1, 2]) and f2["best"].shape == ()
    # chunks of one distance per native call: bit for bit the unchunked result
    monkeypatch.setattr(lib, "CHUNK_BYTES", 6 * S * S * 8)
    fc = pt.focus_series(dev(u), z, LAM, PIX, size=S, planes=True)
    for key in ("power", "sharpness", "peak", "peak_index", "centroid", "width", "focus", "best"):
        assert np.array_equal(fc[key], fs[key]), key
    assert torch.equal(fc["planes"], fs["planes"])
    assert torch.equal(pt.propagate(dev(u), z, LAM, PIX, size=S), got)
    with pytest.raises(ValueError, match="size="):
        pt.propagate(dev(u[..., :12, :12]), z, LAM, PIX)   # 12 is no transform side


def test_initial_probe_to_the_sample_and_back(pt):
    S = 64
    w0 = 3.0
    zr = ref.rayleigh(w0, LAM)
    k = np.fft.fftfreq(S)
    amp = np.exp(-(np.pi * w0) ** 2 * (k[:, None] ** 2 + k[None, :] ** 2))        # far field of exp(-r^2 / w0^2)
    probe = pt.initial_probe((amp ** 2).astype(np.float32)[None], S)
    z = 0.7 * zr
    at_sample = pt.propagate(probe, z, LAM, PIX)
    assert tuple(at_sample.shape) == (1, 1, S, S)
    grid = np.linspace(-1.4 * zr, 0.0, 29)
    fs = pt.focus_series(at_sample, grid, LAM, PIX)
    step = grid[1] - grid[0]
    print("initial probe: focus %.6f of a step off -z" % (abs(fs["focus"][0, 0] + z) / step))
    assert fs["best"][0, 0] == 14 and fs["bracketed"][0, 0]
    assert abs(fs["focus"][0, 0] + z) <= 0.02 * step
    assert fs["width"][0, 0, 14] == pytest.approx(w0 / np.sqrt(2), rel=1e-3)
