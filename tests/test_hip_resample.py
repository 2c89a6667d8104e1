"""B-spline resampling on the device (``libtike.hipfft.resample``, csrc/k_resample.hpp) against the float64 NumPy
restatement of tests/resample_ref.py: the prefilter across its segment plan, the warp on both of its paths, the wrappers,
the moments, and bitwise repeatability.

Tolerances.  The error of a result is the max-norm of its difference from the float64 restatement over ``max |want|``.
The device may be ``FACTOR = 4`` times the error ``e32`` of a float32 NumPy run of the same recursion and taps on the same
input, with a floor and never more than ``CAP = 1e-4`` (a wrong tap, reflection or tile mapping gives 0.1 ... 1; float32
coordinates give 1e-4 at 2048).  ``FLOOR = 1e-6`` is sixteen float32 spacings of the largest value: the device contracts
multiply-adds that NumPy rounds one by one and restarts the recursion from zero state at segment borders (off by at most
1e-9), so where ``e32`` happens to be small (orders 0 and 1, tiny images) the factor alone would ask for NumPy's own
rounding pattern.  profiles/r16/resample.txt records, case by case, the device's error beside ``e32``.
Observed on an MI355X: the largest device error is 8.8e-7 (order 5, minification by 5) beside ``e32`` 6.6e-7; the largest
ratio of the two is 2.9 (order 4 prefilter of the 2 x 2 image, 1.0e-7 beside 3.5e-8).
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as ref  # noqa: E402
from hip_common import bound, dev, host, pt  # noqa: E402, F401

pytestmark = pytest.mark.gpu

FLOOR, CAP = 1e-6, 1e-4
SUM_TOL = 1e-12
ORDERS = (0, 1, 2, 3, 4, 5)
A = np.deg2rad(17.3)
MATRIX = 0.83 * np.array([[np.cos(A), np.sin(A)], [-np.sin(A), np.cos(A)]])
OFFSET = np.array([3.2, -1.7])


@pytest.fixture(scope="module")
def rs():
    import libtike.hipfft.resample as rs
    return rs


@pytest.fixture(scope="module")
def L():
    from libtike.hipfft import _native
    return _native.SPLINE_SEGMENT


def err(got, want):         # not hip_common.rel_max: the difference is taken in the dtype of ``want``, real or complex
    return float(np.abs(got.astype(want.dtype) - want).max() / np.abs(want).max())


_images = {}


def image(shape, cplx=False, seed=3):
    """A float32 / complex64 test image, made once per (shape, kind) and never changed."""
    key = (tuple(shape), cplx, seed)
    if key not in _images:
        rng = np.random.default_rng(seed)
        x = rng.normal(size=shape)
        _images[key] = (x + 1j * rng.normal(size=shape)).astype(np.complex64) if cplx else x.astype(np.float32)
    return _images[key]


def check(name, got, fn):
    """``got`` against ``fn(dtype)`` in float64, bounded by the float32 run of the same ``fn``; prints the figures."""
    want, f32 = fn(np.float64), fn(np.float32)
    e_dev, e32 = err(got, want), err(f32, want)
    print("resample %s: device %.2e, float32 restatement %.2e, bound %.2e" % (name, e_dev, e32, bound(e32, FLOOR, CAP)))
    assert got.shape == want.shape
    assert e_dev <= bound(e32, FLOOR, CAP), (name, e_dev, e32)
    return e_dev


# ---- prefilter --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("order", [2, 3, 4, 5])
def test_prefilter(pt, L, order, cplx):
    # every line inside one segment; interior warm-ups on each axis with a partly filled last segment; the smallest image
    for shape in ((3, 37, 53), (2, 2 * L + 1, 70), (2, 70, 2 * L + 1), (1, 2, 2)):
        x = image(shape, cplx)
        got = pt.spline_prefilter(dev(x), order)
        assert got.is_cuda and got.dtype == (torch.complex64 if cplx else torch.float32)
        check("prefilter order %d %s %s" % (order, "complex" if cplx else "real", shape), host(got),
              lambda dt: ref.prefilter(x, order, dt))
    x = image((2, 2 * L + 1, 70), cplx)
    t = dev(x)
    a = host(pt.spline_prefilter(t, order))
    assert pt.spline_prefilter(t, order, out=t) is t and np.array_equal(host(t), a)      # in place: the same bits
    odd = image((2 * L + 1, 71), cplx)                                                    # rows of an odd length: scalar accesses
    check("prefilter order %d odd rows" % order, host(pt.spline_prefilter(odd, order)), lambda dt: ref.prefilter(odd, order, dt))


def test_prefilter_orders_0_and_1_copy(pt):
    x = image((3, 37, 53), True)
    for order in (0, 1):
        assert np.array_equal(host(pt.spline_prefilter(x, order)), x)


# ---- warp -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_warp_rotation_scale_offset_on_both_paths(pt, rs, order):
    x = image((37, 53), True)
    got, path = rs._warp(dev(x), MATRIX, OFFSET, (41, 47), order, "constant", 2 - 3j, True, None, paths=True)
    check("warp order %d 37x53 -> 41x47" % order, host(got),
          lambda dt: ref.warp(x, MATRIX, OFFSET, (41, 47), order, cval=2 - 3j, dtype=dt))
    sy, sx = ref.coordinates(MATRIX, OFFSET, (41, 47))
    ok = ref.inside(sy, sx, 37, 53, "constant")[2]
    assert 0.5 < ok.mean() < 1 and (host(got)[~ok] == np.complex64(2 - 3j)).all()
    path = host(path)                                                                     # the LDS path; tile (1, 1) lies outside
    assert path.shape == (2, 2) and (path[0] == 1).all() and path[1, 0] == 1 and path[1, 1] == 0 and not ok[32:, 32:].any()
    forced, path2 = rs._warp(dev(x), MATRIX, OFFSET, (41, 47), order, "constant", 2 - 3j, True, None, force_global=True,
                             paths=True)
    assert (host(path2)[path == 1] == 2).all() and np.array_equal(host(forced), host(got))   # global reads: the same bits
    mirror = pt.warp(dev(x), MATRIX, OFFSET, (41, 47), order, mode="mirror")
    check("warp order %d mirror" % order, host(mirror),
          lambda dt: ref.warp(x, MATRIX, OFFSET, (41, 47), order, mode="mirror", dtype=dt))
    assert np.array_equal(host(mirror)[ok], host(got)[ok])


@pytest.mark.parametrize("order", ORDERS)
def test_warp_batch_partial_tiles_and_minification(pt, rs, order):
    x = image((3, 37, 53))
    maps = np.stack([MATRIX, np.array([[1.0, 0.3], [0.0, 0.9]]), MATRIX.T * 0.7])
    offs = np.array([[3.2, -1.7], [0.5, 0.25], [14.0, 6.0]])
    got = pt.warp(dev(x), maps, offs, (41, 47), order, cval=-1.5)
    check("warp order %d batch of 3" % order, host(got), lambda dt: ref.warp(x, maps, offs, (41, 47), order, cval=-1.5, dtype=dt))
    half = np.diag([0.5, 0.55])
    got = pt.warp(dev(x[0]), half, [0.25, 0.5], (70, 90), order)                         # 3 x 3 tiles, the last ones partly filled
    check("warp order %d 70x90" % order, host(got), lambda dt: ref.warp(x[0], half, [0.25, 0.5], (70, 90), order, dtype=dt))
    big = image((300, 300), True, seed=5)
    got, path = rs._warp(dev(big), np.diag([5.0, 5.0]), None, (60, 60), order, "constant", 0.0, True, None, paths=True)
    assert (host(path) == 2).all()                                                        # 160 x 160 sources per tile: global reads
    check("warp order %d minification by 5" % order, host(got),
          lambda dt: ref.warp(big, np.diag([5.0, 5.0]), None, (60, 60), order, dtype=dt))


@pytest.mark.parametrize("order", (0, 3, 4))
def test_warp_tiles_outside_are_cval(rs, order):
    x = image((37, 53))
    got, path = rs._warp(dev(x), None, [-40.0, 20.0], (70, 90), order, "constant", 7.25, True, None, paths=True)
    path, got = host(path), host(got)
    assert path.shape == (3, 3) and (path[0] == 0).all() and (path[:, 2] == 0).all() and path[1, 0] == 1 and path[2, 1] == 1
    want = ref.warp(x, None, [-40.0, 20.0], (70, 90), order, cval=7.25)
    outside = want == 7.25
    assert outside[:32].all() and outside[:, 64:].all() and 0.05 < (~outside).mean() < 0.3
    assert (got[outside] == np.float32(7.25)).all()
    assert err(got, want) <= bound(err(ref.warp(x, None, [-40.0, 20.0], (70, 90), order, cval=7.25, dtype=np.float32), want), FLOOR, CAP)


# ---- exactness ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", ORDERS)
def test_exactness(pt, order):
    x = image((37, 53), True)
    if order <= 1:                                                                        # an integer shift copies bit by bit
        s = host(pt.shift(dev(x), (-3, 5), order=order, cval=0.0))
        assert np.array_equal(s[:-3, 5:], x[3:, :-5]) and (s[-3:] == 0).all() and (s[:, :5] == 0).all()
    same = host(pt.warp(dev(x), order=order))
    e32 = err(ref.warp(x, order=order, dtype=np.float32), x.astype(np.complex128))
    print("resample identity order %d: device %.2e, float32 restatement %.2e" % (order, err(same, x.astype(np.complex128)), e32))
    assert err(same, x.astype(np.complex128)) <= bound(e32, FLOOR, CAP)
    z = host(pt.zoom(dev(x), 2, order=order, cval=np.nan))
    assert z.shape == (74, 106) and not np.isnan(z).any()                                 # the last row and column: never cval
    corners = (np.array([0, 0, -1, -1]), np.array([0, -1, 0, -1]))
    assert np.abs(z[corners] - x[corners]).max() <= bound(e32, FLOOR, CAP) * np.abs(x).max()


# ---- wrappers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", (1, 3, 5))
def test_rotate_zoom_shift_against_the_restatements_maps(pt, order):
    x = image((3, 37, 53))
    angles = np.array([-23.0, 10.0, 171.0])
    got = host(pt.rotate(dev(x), angles, order=order))
    for i in range(3):
        m, o = ref.rotate_map(angles[i], (37, 53))
        check("rotate order %d by %g" % (order, angles[i]), got[i], lambda dt: ref.warp(x[i], m, o, None, order, dtype=dt))
    m, o = ref.rotate_map(-23.0, (37, 53), (24, 30), (15.5, 30.25))                       # rotate, recentre and crop in one pass
    got = host(pt.rotate(dev(x[0]), -23.0, center=(15.5, 30.25), shape=(24, 30), order=order))
    check("rotate order %d about (15.5, 30.25) into 24x30" % order, got, lambda dt: ref.warp(x[0], m, o, (24, 30), order, dtype=dt))
    for factor in (1.37, (0.6, 2.2)):
        m, o, shape = ref.zoom_map((37, 53), factor)
        got = host(pt.zoom(dev(x), factor, order=order, cval=np.nan))
        assert got.shape == (3,) + shape and not np.isnan(got).any()
        check("zoom order %d by %s" % (order, factor), got, lambda dt: ref.warp(x, m, o, shape, order, dtype=dt))
    sh = np.array([[2.25, -4.6], [0.0, 0.5], [-7.5, 3.0]])
    check("shift order %d" % order, host(pt.shift(dev(x), sh, order=order)), lambda dt: ref.warp(x, None, -sh, None, order, dtype=dt))


def test_numpy_and_device_input_and_out(pt):
    x = image((3, 37, 53), True)
    a, b = pt.warp(x, MATRIX, OFFSET, (41, 47), 3), pt.warp(dev(x), MATRIX, OFFSET, (41, 47), 3)
    assert a.is_cuda and np.array_equal(host(a), host(b))
    into = torch.full((3, 41, 47), float("nan"), dtype=torch.complex64, device="cuda")
    assert pt.warp(x, MATRIX, OFFSET, (41, 47), 3, out=into) is into and np.array_equal(host(into), host(a))
    coef = pt.spline_prefilter(x, 3)
    assert np.array_equal(host(pt.warp(coef, MATRIX, OFFSET, (41, 47), 3, prefilter=False)), host(a))
    assert np.array_equal(host(pt.spline_prefilter(x, 5)), host(pt.spline_prefilter(dev(x), 5)))
    t = dev(x)[:, :, ::2]                                                                 # not contiguous: copied
    assert np.array_equal(host(pt.warp(t, order=1)), x[:, :, ::2])
    with pytest.raises(ValueError, match="contiguous"):
        pt.warp(dev(x), out=torch.zeros((3, 53, 37), dtype=torch.complex64, device="cuda").transpose(1, 2))


# ---- moments ------------------------------------------------------------------------------------------------------------------
def close(got, want):
    return bool((np.abs(got - want) <= SUM_TOL * np.abs(want)).all())


def test_center_of_mass(pt):
    rng = np.random.default_rng(8)
    pos = rng.uniform(0.1, 1.0, (3, 37, 53)).astype(np.float32)
    got = pt.center_of_mass(dev(pos))
    s = ref.moments(pos)
    assert got["sums"].dtype == torch.float64 and got["center"].shape == (3, 2) and got["center"].is_cuda
    assert close(host(got["sums"]), s)
    assert np.allclose(host(got["center"]), s[:, 1:3] / s[:, :1], rtol=1e-11, atol=0) and close(host(got["mass"]), s[:, 0])
    assert np.allclose(host(got["second"]), s[:, 3:5] / s[:, :1] - (s[:, 1:3] / s[:, :1]) ** 2, rtol=1e-9)
    mixed = image((300, 301))                                                             # several workgroups per image
    assert (mixed < 0).mean() > 0.4
    assert close(host(pt.center_of_mass(dev(mixed), which="positive")["sums"]), ref.moments(mixed, which="positive"))
    assert close(host(pt.center_of_mass(mixed, which="power")["sums"]), ref.moments(mixed, which="power"))
    w = rng.uniform(0.0, 2.0, (3, 37, 53)).astype(np.float32)
    assert close(host(pt.center_of_mass(dev(pos), dev(w))["sums"]), ref.moments(pos, w))
    c = image((2, 37, 53), True)
    assert close(host(pt.center_of_mass(dev(c), which="power")["sums"]), ref.moments(c))
    one = pt.center_of_mass(dev(pos[1]))
    assert one["center"].shape == (2,) and np.array_equal(host(one["sums"]), host(got["sums"])[1])
    zero = pt.center_of_mass(torch.zeros((2, 9, 12), dtype=torch.float32, device="cuda"))
    assert np.isnan(host(zero["center"])).all() and (host(zero["mass"]) == 0).all()


def test_phase_to_projection_chain(pt):
    """What the README shows: centre of mass of the positive part, then one warp that rotates, recentres and crops."""
    y, x = np.meshgrid(np.arange(96.0), np.arange(160.0), indexing="ij")
    blob = (np.exp(-((y - 40.0) ** 2 / 200.0 + (x - 95.0) ** 2 / 450.0)) - 0.05).astype(np.float32)
    com = host(pt.center_of_mass(dev(blob), which="positive")["center"])
    assert np.abs(com - [40.0, 95.0]).max() < 0.05
    proj = pt.rotate(dev(blob), -30.0, center=com, shape=(64, 64), order=5)
    back = host(pt.center_of_mass(proj, which="positive")["center"])
    assert proj.shape == (64, 64) and np.abs(back - 31.5).max() < 0.05                    # the mass sits on the crop's centre


# ---- repeatability ------------------------------------------------------------------------------------------------------------
def test_two_calls_give_identical_bits(pt, rs, L):
    x = dev(image((2, 2 * L + 1, 70), True))
    for order in (2, 5):
        assert torch.equal(pt.spline_prefilter(x, order), pt.spline_prefilter(x, order))
    big = dev(image((300, 300), True, seed=5))
    for kw in (dict(), dict(force_global=True)):
        a = rs._warp(x, MATRIX, OFFSET, (70, 90), 3, "constant", 0.0, True, None, **kw)
        assert torch.equal(a, rs._warp(x, MATRIX, OFFSET, (70, 90), 3, "constant", 0.0, True, None, **kw))
    assert torch.equal(pt.zoom(big, 0.2, order=4), pt.zoom(big, 0.2, order=4))
    m = dev(image((300, 301)))
    assert torch.equal(pt.center_of_mass(m, which="power")["sums"], pt.center_of_mass(m, which="power")["sums"])
