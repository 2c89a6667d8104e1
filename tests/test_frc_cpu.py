"""Fourier ring correlation, host side: the float64 restatement of tests/frc_ref.py held to its defining properties,
the host code of ``libtike.hipfft.frc`` (window, threshold, crossing, curve) against the restatement, the ring
enumeration of csrc/k_frc.hpp built with the host compiler for every supported crop side, and the argument checks of the
C ABI and of ``frc``.  No GPU needed."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_build  # noqa: E402
import frc_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIDES = list(range(16, 1025)) + [2048]


@pytest.fixture(scope="module")
def lib():
    """The host half of ``libtike.hipfft.frc`` (the package attribute ``frc`` is the function)."""
    import libtike.hipfft  # noqa: F401
    return sys.modules["libtike.hipfft.frc"]


def field(shape, rng, complex_=True):
    x = rng.standard_normal(shape)
    return x + 1j * rng.standard_normal(shape) if complex_ else x


# ---- the restatement's properties -------------------------------------------------------------------------------------
@pytest.mark.parametrize("align", [False, True])
@pytest.mark.parametrize("taper", [0.0, 0.25, 1.0])
def test_identical_images_correlate_fully(align, taper):
    a = field((2, 40, 48), np.random.default_rng(1))
    r = ref.frc(a, a.copy(), region=(4, 8, 32), taper=taper, align=align)
    power = r["sums"][..., 2] > 0
    assert power[:, 1:].all()
    assert np.allclose(r["frc"][power], 1.0, atol=1e-12)
    assert np.allclose(r["shift"], 0.0)
    assert not r["crossed"].any() and np.all(r["crossing"] == 16)


@pytest.mark.parametrize("c", [3.0, -0.5j, 2.0 * np.exp(1.1j)])
def test_complex_scale_is_not_a_difference(c):
    a = field((1, 64, 64), np.random.default_rng(2))
    r = ref.frc(a, c * a, taper=0.25, align=True)
    assert np.allclose(r["frc"][r["sums"][..., 2] > 0], 1.0, atol=1e-12)
    assert np.isclose(np.exp(1j * r["phase"][0]), np.conj(c) / abs(c))


def test_real_inputs_keep_phase_zero():
    a = field((1, 32, 32), np.random.default_rng(3), complex_=False)
    r = ref.frc(a, -a, taper=0.0, align=False)
    assert r["phase"][0] == 0.0
    assert np.allclose(r["frc"][0, 1:], -1.0)


def test_threshold_is_one_for_a_single_pixel(lib):
    for kind in ("half-bit", "one-bit"):
        assert abs(ref.threshold([1], kind)[0] - 1.0) < 1e-4
        assert abs(lib.threshold_curve([1], kind)[0] - 1.0) < 1e-4
        t = ref.threshold(np.arange(1, 10000), kind)
        assert np.all(np.diff(t) < 0)                                  # more pixels, lower threshold
    assert abs(ref.threshold([10 ** 12], "half-bit")[0] - 0.2071 / 1.2071) < 1e-5
    assert np.all(ref.threshold([1, 5, 70], 1 / 7) == 1 / 7)


def test_crossing_on_a_hand_made_curve(lib):
    thr = np.full(6, 0.5)
    curve = np.array([1.0, 0.9, 0.7, 0.4, 0.6, 0.1])
    for fn in (ref.crossing, lib.crossing):
        kc, crossed = fn(curve, thr)
        assert crossed and kc == pytest.approx(2 + 0.2 / 0.3)        # between rings 2 (g = 0.2) and 3 (g = -0.1)
        assert fn(np.array([1.0, 0.4, 0.9]), np.full(3, 0.5)) == (1.0, True)
        assert fn(np.ones(5), np.full(5, 0.5)) == (4.0, False)
        assert fn(np.array([0.0, 0.5, 0.5]), np.full(3, 0.5)) == (2.0, False)   # equal is not below


def test_independent_noise_stays_near_zero():
    rng = np.random.default_rng(4)
    a, b = field((3, 128, 128), rng), field((3, 128, 128), rng)
    r = ref.frc(a, b, taper=0.0, align=False)
    n = r["count"]
    assert np.all(np.abs(r["frc"][:, 1:]) <= 3 / np.sqrt(n[1:]))
    assert np.all(r["crossing"] < 3)


def test_integer_ring_definition_is_rint_sqrt():
    r2 = np.arange(1, 2 * 1025 ** 2 + 1, dtype=np.int64)
    k = np.rint(np.sqrt(r2)).astype(np.int64)
    assert np.all(k * k - k < r2) and np.all((k + 1) * (k + 1) - (k + 1) >= r2)   # k is the largest with k^2 - k < r2


# ---- the library's host code against the restatement ------------------------------------------------------------------
@pytest.mark.parametrize("s", [16, 17, 100, 1000, 2048])
@pytest.mark.parametrize("taper", [0.0, 0.1, 0.25, 0.5, 1.0])
def test_window_is_scipy_tukey(lib, s, taper):
    from scipy.signal import windows
    want = windows.tukey(s, taper)
    assert np.abs(lib.tukey_window(s, taper) - want).max() < 1e-14
    assert np.abs(ref.tukey(s, taper) - want).max() < 1e-14


@pytest.mark.parametrize("real", [False, True])
@pytest.mark.parametrize("kind", ["half-bit", "one-bit", 1 / 7])
def test_curve_from_sums_matches_restatement(lib, real, kind):
    rng = np.random.default_rng(5)
    a = field((2, 64, 64), rng)
    b = a + 0.7 * field((2, 64, 64), rng) * np.linspace(0, 3, 64)[None, None, :]
    want = ref.frc(a, b, taper=0.25, align=False, threshold=kind)
    got = lib.curve_from_sums(want["sums"], real, kind, 64)
    want = ref.curve(want["sums"], real, kind, 64)
    for key in ("frequency", "count", "frc", "threshold", "crossing", "half_period_px", "crossed", "phase"):
        assert np.allclose(got[key], want[key], rtol=1e-12, atol=1e-14), key


def test_default_side(lib):
    assert [lib.default_side(m) for m in (15, 16, 100, 1024, 1500, 2047, 2048, 5000)] == \
        [None, 16, 100, 1024, 1024, 1024, 2048, 2048]
    assert all(lib.supported_side(s) for s in SIDES)
    assert not any(lib.supported_side(s) for s in (15, 1025, 1536, 4096))


# ---- the ring enumeration of csrc/k_frc.hpp, built for the host ---------------------------------------------------------
def test_host_ring_enumeration_covers_every_pixel_once(tmp_path):
    out = host_build.build("host_frc", tmp_path)(stdin=" ".join(map(str, SIDES)) + "\n")
    lines = out.stdout.split("\n")[:-1]
    assert len(lines) == len(SIDES)
    ring_of_r2 = np.rint(np.sqrt(np.arange(2 * 1024 ** 2 + 1))).astype(np.int64)
    for s, line in zip(SIDES, lines):
        words = [int(w) for w in line.split()]
        assert words[0] == s and words[1] == 0, "S = %d: %d pixels visited wrongly" % (s, words[1])
        f2 = ref.freqs(s) ** 2
        r2 = np.bincount((f2[:, None] + f2[None, :]).ravel())
        want = np.bincount(ring_of_r2[:r2.size], weights=r2, minlength=s // 2 + 1)[:s // 2 + 1]
        assert words[2:] == want.astype(np.int64).tolist(), s


# ---- argument checks --------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nat():
    from libtike.hipfft import _native
    return _native


def test_frc_symbols_are_declared_and_exported(nat):
    text = open(os.path.join(ROOT, "include", "ptycho_hip.h")).read()
    for name in ("ptycho_frc_prepare", "ptycho_frc_rings"):
        assert "int %s(" % name in text
        assert name in nat.SYMBOLS and hasattr(nat.lib, name)


def test_frc_abi_rejects_bad_arguments_without_a_gpu(nat):
    d = ctypes.c_void_p(0x1000)              # never dereferenced: every rejection comes before any HIP call
    # ptycho_frc_prepare(out, a, b, ptheta, nz, n, y0, x0, s, window, stream)
    assert nat.frc_prepare(None, d, d, 1, 64, 64, 0, 0, 64, None, None) == 1
    assert b"null" in nat.last_error()
    assert nat.frc_prepare(d, None, d, 1, 64, 64, 0, 0, 64, None, None) == 1
    assert nat.frc_prepare(d, d, None, 1, 64, 64, 0, 0, 64, None, None) == 1
    for s in (0, 15, 1025, 1100, 1536, 4096):
        assert nat.frc_prepare(d, d, d, 1, 5000, 5000, 0, 0, s, None, None) == 1
        assert b"s must be" in nat.last_error()
    assert nat.frc_prepare(d, d, d, 0, 64, 64, 0, 0, 64, None, None) == 1               # ptheta == 0
    assert nat.frc_prepare(d, d, d, 32768, 64, 64, 0, 0, 64, None, None) == 1           # too many angles
    for y0, x0, nz, n in ((1, 0, 64, 64), (0, 1, 64, 64), (0, 0, 63, 64), (0, 0, 64, 63), (65, 0, 64, 64)):
        assert nat.frc_prepare(d, d, d, 1, nz, n, y0, x0, 64, None, None) == 1
        assert b"outside" in nat.last_error()
    # ptycho_frc_rings(sums, spec, ptheta, s, shift, stream)
    assert nat.frc_rings(None, d, 1, 64, None, None) == 1
    assert nat.frc_rings(d, None, 1, 64, None, None) == 1
    for s in (15, 1100, 1536):
        assert nat.frc_rings(d, d, 1, s, d, None) == 1
        assert b"s must be" in nat.last_error()
    assert nat.frc_rings(d, d, 0, 64, None, None) == 1


@pytest.mark.parametrize("kwargs, b_shape, match", [
    ({}, (40, 41), "differ in shape"),
    ({"region": (0, 0, 15)}, None, "not supported"),
    ({"region": (0, 0, 1100)}, None, "not supported"),
    ({"region": (0, 0, 1536)}, None, "not supported"),
    ({"region": (30, 0, 16)}, None, "outside"),
    ({"region": (0, -1, 16)}, None, "outside"),
    ({"region": (0, 0)}, None, "region"),
    ({"taper": -0.1}, None, "taper"),
    ({"taper": 1.5}, None, "taper"),
    ({"taper": float("nan")}, None, "taper"),
    ({"threshold": "third-bit"}, None, "threshold"),
    ({"threshold": None}, None, "threshold"),
])
def test_frc_raises_value_error_before_device_use(kwargs, b_shape, match):
    import torch
    import libtike.hipfft as pt
    a = np.zeros((40, 40), np.complex64)
    b = np.zeros(b_shape or a.shape, np.complex64)
    for x, y in ((a, b), (torch.from_numpy(a), torch.from_numpy(b))):
        with pytest.raises(ValueError, match=match):
            pt.frc(x, y, **kwargs)
    with pytest.raises(ValueError, match="smaller"):
        pt.frc(np.zeros((8, 40)), np.zeros((8, 40)))
    with pytest.raises(ValueError, match="ptheta"):
        pt.frc(np.zeros((2, 2, 40, 40)), np.zeros((2, 2, 40, 40)))


def test_frc_is_exported_with_its_documented_signature():
    import libtike.hipfft as pt
    import libtike.cufft as alias
    assert pt.frc is alias.frc and callable(pt.frc)
    params = inspect.signature(pt.frc).parameters
    assert list(params) == ["a", "b", "region", "taper", "align", "threshold"]
    assert [params[k].default for k in ("region", "taper", "align", "threshold")] == [None, 0.25, True, "half-bit"]
