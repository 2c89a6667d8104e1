"""B-spline resampling, host side: the NumPy restatement of tests/resample_ref.py held against SciPy, the properties that
the cases of tests/test_hip_resample.py rely on, the index logic of csrc/k_resample.hpp built with the host compiler and
walked as the kernels walk it, and the argument checks of the C ABI and of ``libtike.hipfft.resample``.  No GPU needed."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libtike-cufft_amd", "csrc")
TOL = 1e-11          # relative; observed <= 1.1e-12 (coefficients) and 5e-14 (samples)
ORDERS = (0, 1, 2, 3, 4, 5)
A = np.deg2rad(17.3)
MATRIX = 0.83 * np.array([[np.cos(A), np.sin(A)], [-np.sin(A), np.cos(A)]])
OFFSET = np.array([3.2, -1.7])


@pytest.fixture(scope="module")
def lib():
    import libtike.hipfft.resample as lib
    return lib


@pytest.fixture(scope="module")
def nat():
    from libtike.hipfft import _native
    return _native


def image(shape=(37, 53), cplx=False, seed=3):
    rng = np.random.default_rng(seed)
    x = rng.normal(size=shape)
    return x + 1j * rng.normal(size=shape) if cplx else x


def relerr(got, want):
    return np.abs(got - want).max() / np.abs(want).max()


def scipy_of(fn, x, *args, **kw):
    """A SciPy filter on a real or complex array (real and imaginary part apart)."""
    if np.iscomplexobj(x):
        return fn(x.real, *args, **kw) + 1j * fn(x.imag, *args, **kw)
    return fn(x, *args, **kw)


# ---- the restatement against SciPy ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cplx", [False, True])
@pytest.mark.parametrize("order", ORDERS)
def test_restatement_against_scipy(order, cplx):
    ndi = pytest.importorskip("scipy.ndimage")
    x = image(cplx=cplx)
    coef = ref.prefilter(x, order)
    if order >= 2:
        want = scipy_of(ndi.spline_filter, x, order=order, mode="mirror")
        assert relerr(coef, want) <= TOL
    else:
        assert np.array_equal(coef, x)
    got = ref.warp(x, MATRIX, OFFSET, (41, 47), order, mode="mirror")
    want = scipy_of(ndi.affine_transform, x, MATRIX, OFFSET, (41, 47), order=order, mode="mirror")
    sy, sx = ref.coordinates(MATRIX, OFFSET, (41, 47))
    ok = ref.inside(sy, sx, 37, 53, "constant")[2]
    assert 0.5 < ok.mean() < 1.0
    assert np.abs(got - want)[ok].max() <= TOL * np.abs(want[ok]).max()
    const = ref.warp(x, MATRIX, OFFSET, (41, 47), order, cval=-7.5)
    assert np.array_equal(const[ok], got[ok]) and (const[~ok] == -7.5).all()   # outside the extent: exactly cval


@pytest.mark.parametrize("order", ORDERS)
def test_rotate_and_zoom_maps_against_scipy(order):
    ndi = pytest.importorskip("scipy.ndimage")
    x = image()
    m, o = ref.rotate_map(-23.0, x.shape)
    got = ref.warp(x, m, o, None, order, mode="mirror")
    want = ndi.rotate(x, -23.0, reshape=False, order=order, mode="mirror")
    ok = ref.inside(*ref.coordinates(m, o, x.shape), 37, 53, "constant")[2]
    assert np.abs(got - want)[ok].max() <= TOL * np.abs(want).max()
    for factor in (2, 1.37, (0.6, 2.2)):
        m, o, shape = ref.zoom_map(x.shape, factor)
        got = ref.warp(x, m, o, shape, order)
        want = ndi.zoom(x, factor, order=order, mode="mirror")
        assert got.shape == want.shape
        assert relerr(got, want) <= TOL                                   # every pixel: none may fall outside
    got = ref.warp(x, None, [-2.25, 4.6], None, order, mode="mirror")
    want = ndi.shift(x, (2.25, -4.6), order=order, mode="mirror")
    assert relerr(got, want) <= TOL


@pytest.mark.parametrize("order", ORDERS)
def test_interpolating_splines_reproduce_the_samples(order):
    x = image(cplx=True)
    assert relerr(ref.warp(x, order=order), x) <= 1e-13
    m, o, shape = ref.zoom_map(x.shape, 2)
    z = ref.warp(x, m, o, shape, order, cval=np.nan)
    assert shape == (74, 106) and not np.isnan(z).any()
    corners = (np.array([0, 0, -1, -1]), np.array([0, -1, 0, -1]))
    assert np.abs(z[corners] - x[corners]).max() <= 1e-13 * np.abs(x).max()
    if order <= 1:                                                        # an integer shift copies
        s = ref.warp(x, None, [3, -5], None, order, cval=0.0)
        assert np.array_equal(s[:-3, 5:], x[3:, :-5]) and (s[-3:] == 0).all() and (s[:, :5] == 0).all()


def test_float32_run_is_close_and_batches_take_their_own_maps():
    x = image((3, 37, 53))
    maps = np.stack([MATRIX, np.eye(2), MATRIX.T])
    offs = np.array([[3.2, -1.7], [0.5, 0.25], [-4.0, 6.0]])
    got = ref.warp(x, maps, offs, (41, 47), 3)
    for i in range(3):
        assert np.array_equal(got[i], ref.warp(x[i], maps[i], offs[i], (41, 47), 3))
    f32 = ref.warp(x.astype(np.float32), maps, offs, (41, 47), 3, dtype=np.float32)
    assert f32.dtype == np.float32 and 1e-9 < relerr(f32, ref.warp(x.astype(np.float32), maps, offs, (41, 47), 3)) < 1e-5
    w = ref.weights(np.linspace(0, 0.999, 50), 5)
    assert np.abs(w.sum(0) - 1).max() < 1e-14
    assert np.allclose(ref.weights(0.0, 5), np.array([1, 26, 66, 26, 1, 0]) / 120.0, atol=1e-15)
    assert np.allclose(ref.weights(0.0, 4), np.array([1, 76, 230, 76, 1]) / 384.0, atol=1e-15)


def test_moments_restatement():
    x = image((2, 9, 12)).astype(np.float32)
    s = ref.moments(x, which="positive")
    p = np.where(x > 0, x, 0).astype(np.float64)
    y = np.arange(9.0)[:, None]
    assert np.allclose(s[:, 0], p.sum((1, 2)), rtol=1e-14) and np.allclose(s[:, 1], (p * y).sum((1, 2)), rtol=1e-14)
    assert ref.moments(np.zeros((4, 4), np.float32)).tolist() == [0.0] * 5


# ---- the index logic of csrc/k_resample.hpp, built for the host ---------------------------------------------------------------
def test_host_walk_of_the_plan_the_reflection_and_the_boxes(tmp_path):
    out = subprocess.run(["make", "-C", CSRC, "host_resample", "HOST_OUT=%s" % (tmp_path / "pty_host_resample")],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.splitlines()
    assert "host_resample: 0 errors" in lines
    plan = [ln for ln in lines if ln.startswith("prefilter:")][0]
    assert float(plan.split()[-5]) <= 1e-8, plan
    boxes = [ln for ln in lines if ln.startswith("boxes:")][0].split()
    assert min(int(boxes[1]), int(boxes[4]), int(boxes[6])) > 0          # tiles outside, on the LDS path, on the global path


# ---- symbols and argument checks --------------------------------------------------------------------------------------------
NAMES = {"ptycho_spline_work_words": "size_t", "ptycho_spline_prefilter": "int", "ptycho_warp": "int",
         "ptycho_moments_work_words": "size_t", "ptycho_moments": "int"}


def test_resample_symbols_are_declared_exported_and_documented(nat):
    text = open(os.path.join(ROOT, "include", "ptycho_hip.h")).read()
    for name, res in NAMES.items():
        assert "%s %s(" % (res, name) in text
        assert name in nat.SYMBOLS and hasattr(nat.lib, name)
        assert text.count(name) >= 2                                      # the declaration and the comment that documents it
    assert "#define PTYCHO_SPLINE_SEGMENT 64" in text and nat.SPLINE_SEGMENT == 64
    assert "#define PTYCHO_WARP_MIRROR 1" in text and "#define PTYCHO_WARP_GLOBAL 2" in text
    assert (nat.WARP_MIRROR, nat.WARP_GLOBAL) == (1, 2)
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_resample.hpp" in make and "host_resample.hpp" in make and "host_resample:" in make


def test_resample_abi_rejects_bad_arguments_without_a_gpu(nat):
    d, e = ctypes.c_void_p(0x1000), ctypes.c_void_p(0x2000)     # never dereferenced: every rejection comes before any HIP call
    pre = dict(out=d, inp=e, nimg=1, ny=8, nx=8, cplx=0, order=3, work=ctypes.c_void_p(0x3000))
    warp = dict(out=d, coef=e, xf=d, nimg=1, ny=8, nx=8, oh=8, ow=8, cplx=0, order=3, flags=0, cre=0.0, cim=0.0, path=None)
    mom = dict(sums=d, x=e, weight=None, nimg=1, ny=8, nx=8, cplx=0, which=0, work=d)
    for fn, ok, required in ((nat.spline_prefilter, pre, ("out", "inp", "work")), (nat.warp, warp, ("out", "coef", "xf")),
                             (nat.moments, mom, ("sums", "x", "work"))):
        call = lambda **over: fn(*{**ok, **over}.values(), None)   # noqa: E731
        for name in required:
            assert call(**{name: None}) == 1
            assert b"null" in nat.last_error()
        for over in (dict(ny=1), dict(nx=1), dict(ny=0)):
            assert call(**over) == 1
            assert b"at least 2" in nat.last_error()
        for over in (dict(ny=65537), dict(ny=65536, nx=32768)):
            assert call(**over) == 1
            assert b"2^31" in nat.last_error()
        for bad in (0, 65536):
            assert call(nimg=bad) == 1
            assert b"nimg" in nat.last_error()
    for fn, ok in ((nat.spline_prefilter, pre), (nat.warp, warp)):
        for bad in (-1, 6):
            assert fn(*{**ok, "order": bad}.values(), None) == 1
            assert b"order" in nat.last_error()
    assert nat.spline_prefilter(*{**pre, "work": d}.values(), None) == 1 and b"work" in nat.last_error()
    assert nat.warp(*{**warp, "coef": d}.values(), None) == 1 and b"coef" in nat.last_error()
    assert nat.warp(*{**warp, "flags": 4}.values(), None) == 1 and b"flags" in nat.last_error()
    for over in (dict(oh=0), dict(ow=65537), dict(oh=65536, ow=32768)):
        assert nat.warp(*{**warp, **over}.values(), None) == 1 and b"output" in nat.last_error()
    assert nat.moments(*{**mom, "which": 3}.values(), None) == 1 and b"which" in nat.last_error()
    assert nat.moments(*{**mom, "cplx": 1, "which": 0}.values(), None) == 1 and b"complex" in nat.last_error()
    assert nat.spline_work_words(2, 37, 53, 1) == 2 * 37 * 53 and nat.spline_work_words(1, 3, 3, 0) == 5
    assert nat.spline_work_words(1, 1, 8, 0) == 0 and nat.moments_work_words(0, 8, 8) == 0
    assert nat.moments_work_words(3, 64, 64) == 3 * 8 and nat.moments_work_words(1, 2048, 2048) == 512 * 8


def args(**over):
    a = {"x": np.zeros((3, 9, 12), np.float32), "matrix": None, "offset": None, "shape": None, "order": 3,
         "mode": "constant", "cval": 0.0, "prefilter": True, "out": None}
    a.update(over)
    return a


def test_checker_accepts_the_documented_shapes(lib):
    import torch
    lead, ny, nx, oh, ow, cplx, xf = lib.check_warp(**args())
    assert (lead, ny, nx, oh, ow, cplx) == ((3,), 9, 12, 9, 12, False)
    assert xf.shape == (3, 6) and xf.dtype == np.float64 and xf.tolist() == [[1, 0, 0, 1, 0, 0]] * 3
    per = np.arange(12.0).reshape(3, 2, 2)
    xf = lib.check_warp(**args(matrix=per, offset=[0.5, -1], shape=(4, 30)))[6]
    assert xf[2].tolist() == [8, 9, 10, 11, 0.5, -1]
    assert lib.check_warp(np.zeros((2, 2), np.complex64), cval=1 + 2j, order=np.int64(0), mode="mirror")[5] is True
    t = torch.zeros((2, 5, 9, 12))
    assert lib.check_warp(t, offset=np.zeros((2, 5, 2)), out=torch.zeros((2, 5, 3, 4)), shape=(3, 4))[0] == (2, 5)


@pytest.mark.parametrize("over, exc, match", [
    ({"x": [[0.0]]}, TypeError, "x must be an array"),
    ({"x": np.zeros((9, 12), np.float64)}, TypeError, "x must be float32 or complex64, got float64"),
    ({"x": np.zeros((12,), np.float32)}, ValueError, r"x must be \[..., ny, nx\]"),
    ({"x": np.zeros((3, 1, 12), np.float32)}, ValueError, "sides in"),
    ({"x": np.zeros((0, 9, 12), np.float32)}, ValueError, "1 to 65535 images"),
    ({"matrix": np.eye(3)}, ValueError, "matrix must have shape"),
    ({"matrix": np.zeros((2, 2, 2))}, ValueError, "matrix must have shape"),
    ({"matrix": [[1.0, np.nan], [0.0, 1.0]]}, ValueError, "matrix must be finite"),
    ({"matrix": [[1.0, np.inf], [0.0, 1.0]]}, ValueError, "matrix must be finite"),
    ({"matrix": "turn"}, TypeError, "matrix must be an array of real numbers"),
    ({"offset": [1.0, 2.0, 3.0]}, ValueError, "offset must have shape"),
    ({"offset": [np.inf, 0.0]}, ValueError, "offset must be finite"),
    ({"shape": (0, 4)}, ValueError, "shape must hold"),
    ({"shape": (4.0, 4)}, ValueError, "shape must hold"),
    ({"shape": 7}, ValueError, "shape must be"),
    ({"order": 6}, ValueError, "order must be"),
    ({"order": -1}, ValueError, "order must be"),
    ({"order": 2.0}, ValueError, "order must be"),
    ({"order": True}, ValueError, "order must be"),
    ({"mode": "wrap"}, ValueError, "mode must be"),
    ({"cval": "zero"}, TypeError, "cval must be a number"),
    ({"cval": 1j}, TypeError, "cval must be real"),
    ({"prefilter": 1}, TypeError, "prefilter must be a bool"),
    ({"out": np.zeros((3, 9, 12), np.complex64)}, TypeError, "out must be float32"),
    ({"out": np.zeros((9, 12), np.float32)}, ValueError, "out must have shape"),
])
def test_bad_arguments_raise_before_device_use(lib, over, exc, match):
    import libtike.hipfft as pt
    a = args(**over)
    with pytest.raises(exc, match=match):
        lib.check_warp(**a)
    with pytest.raises(exc, match=match):                                 # the public function checks first
        pt.warp(**a)
    if set(over) <= {"x", "order"}:
        with pytest.raises(exc, match=match):
            pt.spline_prefilter(a["x"], a["order"])
        for fn, arg in ((pt.rotate, 10.0), (pt.zoom, 2), (pt.shift, (1.0, 2.0))):
            with pytest.raises(exc, match=match):
                fn(a["x"], arg, order=a["order"])
    if set(over) <= {"x"}:
        with pytest.raises(exc, match=match):
            pt.center_of_mass(a["x"])


def test_wrappers_check_their_own_arguments(lib):
    import torch
    x = np.zeros((3, 9, 12), np.float32)
    with pytest.raises(ValueError, match="angle must have shape"):
        lib.rotate(x, [1.0, 2.0])
    with pytest.raises(ValueError, match="angle must be finite"):
        lib.rotate(x, np.nan)
    with pytest.raises(ValueError, match="center must have shape"):
        lib.rotate(x, 1.0, center=[1.0])
    with pytest.raises(ValueError, match="factor must be positive"):
        lib.zoom(x, -2)
    with pytest.raises(ValueError, match="leaves no pixels"):
        lib.zoom(x, 0.01)
    with pytest.raises(ValueError, match="shift must have shape"):
        lib.shift(x, 1.0)
    with pytest.raises(ValueError, match="which must be"):
        lib.center_of_mass(x, which="absolute")
    with pytest.raises(ValueError, match="which must be 'power'"):
        lib.center_of_mass(x.astype(np.complex64))
    with pytest.raises(TypeError, match="weight must be float32"):
        lib.center_of_mass(x, weight=np.ones((3, 9, 12)))
    with pytest.raises(ValueError, match="weight must have x's shape"):
        lib.center_of_mass(x, weight=np.ones((9, 12), np.float32))
    with pytest.raises(ValueError, match="device tensors or NumPy arrays"):
        lib.warp(torch.zeros((8, 8)))


def test_resample_functions_are_exported_with_their_documented_signatures(lib):
    import libtike.hipfft as pt
    from libtike.hipfft import ptycho as P
    for name in ("spline_prefilter", "warp", "rotate", "zoom", "shift", "center_of_mass"):
        assert getattr(pt, name) is getattr(lib, name)
    assert lib.__all__ == ["spline_prefilter", "warp", "rotate", "zoom", "shift", "center_of_mass", "check_warp"]
    sig = inspect.signature(pt.warp).parameters
    assert list(sig) == ["x", "matrix", "offset", "shape", "order", "mode", "cval", "prefilter", "out"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, None, None, 3, "constant", 0.0, True, None]
    assert inspect.signature(lib.check_warp) == inspect.signature(pt.warp)
    assert list(inspect.signature(pt.spline_prefilter).parameters) == ["x", "order", "out"]
    assert list(inspect.signature(pt.rotate).parameters)[:4] == ["x", "angle", "center", "order"]
    assert list(inspect.signature(pt.zoom).parameters)[:3] == ["x", "factor", "order"]
    assert list(inspect.signature(pt.center_of_mass).parameters) == ["x", "weight", "which"]
    assert "warp" not in P.__all__ and len(P.__all__) == 6
