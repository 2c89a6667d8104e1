"""CPU-side checks of the propagation module: the native symbols and their argument checks, ``check_arguments``, the
NumPy restatement (tests/propagate_ref.py) against the analytic Gaussian beam, its focus search, and the host program
that walks the plain C++ of csrc/k_propagate.hpp.  No GPU."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_build  # noqa: E402
import propagate_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build_native()
    from libtike.hipfft import _native
    return _native


@pytest.fixture(scope="module")
def lib(nat):
    import importlib
    return importlib.import_module("libtike.hipfft.propagate")   # (the package's attribute of that name is the function)


def test_symbols_and_null_handle(nat):
    for name in ("ptycho_propagate", "ptycho_propagate_work_words"):
        assert name in nat.SYMBOLS
        assert hasattr(nat.lib, name)
    assert nat.propagate(None, None, None, None, 1, None, 1, 0.0, 0, None, None) == 1
    assert b"null handle" in nat.last_error()
    assert nat.propagate_work_words(None, 4, 64, 0) == 0
    import libtike.hipfft as pt
    assert pt.propagate is not None and pt.focus_series is not None and pt.object_pixel_size is not None


def test_object_pixel_size(lib):
    assert lib.object_pixel_size(1e-10, 2.0, 75e-6, 256) == pytest.approx(1e-10 * 2.0 / (256 * 75e-6), rel=1e-15)
    for bad in ((0, 1, 1, 8), (1, -1, 1, 8), (1, 1, float("inf"), 8), (1, 1, 1, 0), (1, 1, 1, 2.5)):
        with pytest.raises(ValueError):
            lib.object_pixel_size(*bad)


def test_check_arguments(lib):
    u = np.zeros((2, 3, 64, 64), dtype=np.complex64)
    s, big, z, scalar = lib.check_arguments(u, 1e-3, 1e-10, 1e-8)
    assert (s, big, scalar) == (64, 64, True) and z.tolist() == [1e-3] and z.dtype == np.float64
    s, big, z, scalar = lib.check_arguments(u[0, 0, :40, :40], [0.0, -1.0, 2.0], 1.0, 1.0, "angular", size=64)
    assert (s, big, scalar) == (40, 64, False) and z.tolist() == [0.0, -1.0, 2.0]
    with pytest.raises(ValueError):                     # not square
        lib.check_arguments(u[..., :32], 0.0, 1.0, 1.0)
    with pytest.raises(ValueError):                     # no two axes
        lib.check_arguments(u[0, 0, 0], 0.0, 1.0, 1.0)
    with pytest.raises(TypeError):                      # real
        lib.check_arguments(u.real, 0.0, 1.0, 1.0)
    with pytest.raises(TypeError):                      # not an array
        lib.check_arguments([[1j]], 0.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="method"):
        lib.check_arguments(u, 0.0, 1.0, 1.0, method="rayleigh")
    for bad in (0.0, -1.0, float("nan"), float("inf"), True, "1"):
        with pytest.raises(ValueError, match="wavelength"):
            lib.check_arguments(u, 0.0, bad, 1.0)
        with pytest.raises(ValueError, match="pixel_size"):
            lib.check_arguments(u, 0.0, 1.0, bad)
    for bad in (float("nan"), float("inf"), [0.0, float("-inf")]):
        with pytest.raises(ValueError, match="finite"):
            lib.check_arguments(u, bad, 1.0, 1.0)
    with pytest.raises(ValueError, match="non-empty"):
        lib.check_arguments(u, [], 1.0, 1.0)
    with pytest.raises(ValueError, match="non-empty"):
        lib.check_arguments(u, [[0.0, 1.0]], 1.0, 1.0)
    with pytest.raises(ValueError, match="size="):      # size < s
        lib.check_arguments(u, 0.0, 1.0, 1.0, size=48)
    with pytest.raises(ValueError, match="size="):      # unsupported size
        lib.check_arguments(u, 0.0, 1.0, 1.0, size=1100)
    with pytest.raises(TypeError):
        lib.check_arguments(u, 0.0, 1.0, 1.0, size=64.0)
    with pytest.raises(ValueError, match="size="):      # an unsupported field side names the way out
        lib.check_arguments(np.zeros((12, 12), dtype=np.complex128), 0.0, 1.0, 1.0)
    with pytest.raises(ValueError, match="size="):
        lib.check_arguments(np.zeros((1, 1030, 1030), dtype=np.complex64), 0.0, 1.0, 1.0)
    assert lib.check_arguments(np.zeros((12, 12), dtype=np.complex128), 0.0, 1.0, 1.0, size=16)[:2] == (12, 16)


def test_figures_on_the_host(lib):
    """``figures`` (the host half of ``focus_series``) on the restatement's metrics: coordinates, focus, flags."""
    S, lo, p, lam, w0 = 64, 12, 1.0, 0.05, 3.0
    zr = ref.rayleigh(w0, lam)
    z = np.linspace(-1.4 * zr, 0.0, 29)
    u0 = ref.gaussian_beam(S, w0, lam, p, 0.7 * zr, centre=30)
    m = np.stack([ref.metrics(ref.propagate(u0, zz, lam, p)) for zz in z])
    res = lib.figures(m[None], z, S, lo)
    b, f, ok = ref.focus(z, ref.sharpness(m))
    assert res["best"].shape == (1,) and res["best"][0] == b == 14 and res["bracketed"][0] and ok
    assert abs(res["focus"][0] - f) <= 1e-9 * (z[1] - z[0])
    assert np.array_equal(res["peak_index"][0, b], [30 - lo, 30 - lo])
    assert np.abs(res["centroid"][0, b] - (30 - lo)).max() < 1e-6
    assert res["width"][0, b] == pytest.approx(w0 / np.sqrt(2), rel=1e-6)
    assert np.allclose(res["power"], m[:, 0]) and np.allclose(res["sharpness"][0], ref.sharpness(m))
    ends = lib.figures(m[None, :15], z[:15], S, lo)     # the maximum is the last sample: not bracketed
    assert ends["best"][0] == 14 and not ends["bracketed"][0] and ends["focus"][0] == z[14]


def test_reference_matches_the_analytic_gaussian():
    S, p, lam = 64, 1.0, 0.05
    w0 = 4 * p
    zr = ref.rayleigh(w0, lam)
    u0 = ref.gaussian_beam(S, w0, lam, p, 0.0)
    for z in (0.5 * zr, -0.8 * zr):
        want = ref.gaussian_beam(S, w0, lam, p, z)
        fres = ref.propagate(u0, z, lam, p, "fresnel")
        ang = ref.propagate(u0, z, lam, p, "angular")
        e_f = np.abs(fres - want).max() / np.abs(want).max()
        e_a = np.abs(ang - fres).max() / np.abs(want).max()
        print("z / zR %+.1f: fresnel vs analytic %.1e, angular vs fresnel %.1e" % (z / zr, e_f, e_a))
        assert e_f <= 1e-12
        assert e_a <= 1e-5
    assert np.abs(ref.propagate(u0, 0.0, lam, p, "angular") - u0).max() <= 1e-14
    m = ref.metrics(u0)
    cy, cx = m[2] / m[0], m[3] / m[0]
    assert cy == pytest.approx(S // 2, abs=1e-6) and cx == pytest.approx(S // 2, abs=1e-6)
    assert np.sqrt(m[4] / m[0] - cy * cy) == pytest.approx(w0 / 2, rel=1e-6)
    assert np.sqrt(m[5] / m[0] - cx * cx) == pytest.approx(w0 / 2, rel=1e-6)
    assert ref.width(m) == pytest.approx(w0 / np.sqrt(2), rel=1e-6)
    assert m[6] == 1.0 and m[7] == (S // 2) * S + S // 2


def test_reference_metrics_rules():
    plane = np.zeros((16, 16), dtype=np.complex64)
    plane[3, 5] = plane[9, 2] = 2.0
    plane[4, 4] = np.nan
    m = ref.metrics(plane)
    assert m[6] == 4.0 and m[7] == 3 * 16 + 5 and np.isnan(m[0])     # first maximum; the NaN is in the sums only
    m = ref.metrics(np.full((16, 16), np.nan, dtype=np.complex64))
    assert m[6] == -np.inf and m[7] == -1


def test_reference_focus():
    S, p, lam = 64, 1.0, 0.05
    w0 = 3 * p
    zr = ref.rayleigh(w0, lam)
    u0 = ref.gaussian_beam(S, w0, lam, p, 0.7 * zr)

    def series(z):
        return np.array([ref.sharpness(ref.metrics(ref.propagate(u0, zz, lam, p))) for zz in z])

    z = np.linspace(-1.4 * zr, 0.0, 29)
    step = z[1] - z[0]
    b, f, ok = ref.focus(z, series(z))
    print("focus error on the grid: %.1e of a step" % (abs(f + 0.7 * zr) / step))
    assert ok and b == 14 and abs(f + 0.7 * zr) <= 1e-6 * step
    # a grid whose nearest sample is a third of a step off the focus: the sharpness of a Gaussian is a Lorentzian in z,
    # 1 / (1 + (dz / zR)^2), not a parabola; three samples at -2/3, 1/3, 4/3 of a step h put the vertex at
    # dz = -(h / 3) (h / zR)^2 (8 / 9) / (1 - ...) -- evaluated here from the Lorentzian itself, not from the device
    z3 = z + step / 3.0
    b3, f3, ok3 = ref.focus(z3, series(z3))
    lor = 1.0 / (1.0 + ((z3[b3 - 1:b3 + 2] + 0.7 * zr) / zr) ** 2)
    want = ref.focus(z3[b3 - 1:b3 + 2], lor)[1]
    print("third-of-a-step grid: parabola error %.2e of a step, Lorentzian prediction %.2e"
          % ((f3 + 0.7 * zr) / step, (want + 0.7 * zr) / step))
    assert ok3 and abs(z3[b3] + 0.7 * zr) <= 0.34 * step
    assert abs(f3 - want) <= 1e-6 * step
    assert abs(f3 + 0.7 * zr) <= 0.01 * step     # (h / zR)^2 / 3 of a step with h = zR / 20: under 1e-3


def test_host_program(tmp_path):
    out = host_build.build("host_propagate", tmp_path)().stdout
    assert out.startswith("host_propagate:") and out.strip().endswith(" 0 errors"), out
