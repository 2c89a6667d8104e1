"""Illumination map and gauge fixing, host side: the float64 restatement of tests/gauge_ref.py held to its defining
properties (it places whole-pixel patches as tests/recon_metrics.py does, it recovers a planted gauge to rounding, an
object it has fixed has no gauge left), the index logic of csrc/k_gauge.hpp built with the host compiler and walked as
the kernel walks it, and the argument checks of the C ABI and of ``libtike.hipfft.gauge``.  No GPU needed."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_build  # noqa: E402
import gauge_ref as ref  # noqa: E402
import recon_metrics as rm  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import libtike.hipfft.gauge as lib
    return lib


@pytest.fixture(scope="module")
def nat():
    from libtike.hipfft import _native
    return _native


# ---- the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nmodes", [None, 1, 3])
def test_restatement_places_whole_pixel_patches(nmodes):
    rng = np.random.default_rng(1)
    nz, n, nprb = 40, 56, 16
    probe = ref.random_probe(rng, 1, nmodes, nprb).astype(np.complex128)   # recon_metrics squares in the input's precision
    scan = np.stack([rng.integers(0, nz - nprb, 12), rng.integers(0, n - nprb, 12)], -1).astype(np.float32)[None]
    scan[0, 3] = scan[0, 7]                                           # two identical positions add twice
    got = ref.illumination(scan, probe, nz, n)
    want = rm.illumination(scan[0], probe[0], nz, n)
    assert got.shape == (1, nz, n) and got.dtype == np.float64
    assert np.abs(got[0] - want).max() <= 1e-12 * want.max()


def test_restatement_weights_sum_to_one_and_skip_what_the_operators_skip():
    scan, nz, n, nprb = ref.case_a_scan()
    probe = np.ones((2, 2, nprb, nprb), np.complex64)                 # A = 2 everywhere
    ill = ref.illumination(scan, probe, nz, n)
    keep = [[ref.split(p[0])[0] and ref.split(p[1])[0] for p in scan[t]] for t in range(2)]
    assert keep[0] == [True] * 5 + [False, False, True, True]
    assert keep[1] == [True, True, True, False, True, False, True, True, True]
    one = ref.illumination(np.array([[[7.25, 30.75]]], np.float32), probe[:1], nz, n)[0]
    assert np.allclose(one[8:7 + nprb, 31:30 + nprb], 2.0) and one.sum() == pytest.approx(2.0 * nprb * nprb)
    for t in range(2):                                                # skipped positions contribute nothing
        kept = scan[t][keep[t]][None]
        assert np.array_equal(ref.illumination(kept, probe[t:t + 1], nz, n)[0], ill[t])
    assert ref.split(np.float32(-0.5)) == (True, 0, np.float32(-0.5))  # modff: the integer part -0.0 is not negative


def planted(rng, ptheta=1, nz=33, n=47, gy=0.31, gx=-0.27, phi=0.9, s0=1.7):
    r = rng.standard_normal((ptheta, nz, n)) + 1j * rng.standard_normal((ptheta, nz, n))
    w = np.zeros((ptheta, nz, n))
    w[:, 3:-4, 5:-2] = rng.uniform(0.2, 1.0, (ptheta, nz - 7, n - 7))   # zero border
    y, x = np.arange(nz)[:, None], np.arange(n)[None, :]
    yc = (w * y).sum((1, 2), keepdims=True) / w.sum((1, 2), keepdims=True)
    xc = (w * x).sum((1, 2), keepdims=True) / w.sum((1, 2), keepdims=True)
    psi = s0 * r * np.exp(1j * (phi + gy * (y - yc) + gx * (x - xc)))
    return psi, r, w, np.array([gy, gx, phi, s0]), yc.ravel(), xc.ravel()


def test_fit_recovers_a_planted_gauge():
    psi, r, w, g, yc, xc = planted(np.random.default_rng(2), ptheta=2)
    got = ref.fit(psi, w, r)
    assert got.shape == (2, 6)
    assert np.abs(got[:, :4] - g).max() < 1e-12
    assert np.abs(got[:, 4] - yc).max() < 1e-12 and np.abs(got[:, 5] - xc).max() < 1e-12
    assert ref.fit(psi[0], w[0], r[0]).shape == (6,)


def test_object_fixed_by_apply_has_no_gauge_left():
    psi, r, w, _, _, _ = planted(np.random.default_rng(3))
    fixed = ref.apply(psi, ref.fit(psi, w, r), "object")
    again = ref.fit(fixed, w, r)
    assert np.abs(again[:, :3]).max() < 1e-12 and abs(again[0, 3] - 1) < 1e-12
    assert np.abs(fixed - r).max() < 1e-12 * np.abs(r).max() * 10     # psi was ref in another gauge
    g0 = ref.fit(psi, w)                                              # without ref: unit weighted RMS amplitude
    alone = ref.fit(ref.apply(psi, g0, "object"), w)
    assert abs(alone[0, 2]) < 1e-12 and abs(alone[0, 3] - 1) < 1e-12


def test_fit_of_zero_weight_is_the_identity():
    psi, r, w, _, _, _ = planted(np.random.default_rng(4), ptheta=2)
    w[1] = 0
    got = ref.fit(psi, w, r)
    assert np.array_equal(got[1], [0, 0, 0, 1, 0, 0]) and got[0, 3] == pytest.approx(1.7)


def test_object_and_probe_companion_keep_whole_pixel_exit_waves():
    rng = np.random.default_rng(5)
    psi = rng.standard_normal((1, 30, 34)) + 1j * rng.standard_normal((1, 30, 34))
    prb = ref.random_probe(rng, 1, 2, 8).astype(np.complex128)
    g = np.array([[0.4, -0.7, 1.1, 2.5, 13.2, 17.9]])
    p2, q2 = ref.apply(psi, g, "object"), ref.apply(prb, g, "probe")
    for sy, sx in ((0, 0), (5, 11), (22, 26)):
        a = prb[0] * psi[0, sy:sy + 8, sx:sx + 8]
        b = q2[0] * p2[0, sy:sy + 8, sx:sx + 8]
        ratio = b / a
        assert np.abs(np.abs(ratio) - 1).max() < 1e-12 and np.abs(ratio - ratio[0, 0, 0]).max() < 1e-12


# ---- the index logic of csrc/k_gauge.hpp, built for the host --------------------------------------------------------------
@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    program = host_build.build("host_gauge", tmp_path_factory.mktemp("gauge"))

    def walk(scan, nprb, nz, n):
        text = "%d %d %d %d %d\n%s\n" % (scan.shape[0], scan.shape[1], nprb, nz, n,
                                         " ".join(str(int(v)) for v in scan.view(np.uint32).ravel()))
        return [int(v) for v in program(stdin=text).stdout.split()]
    return walk


def expected_visits(scan, nprb, nz, n):
    total = skipped = 0
    for py, px in scan.reshape(-1, 2):
        (vy, sy, _), (vx, sx, _) = ref.split(py), ref.split(px)
        if not (vy and vx):
            skipped += 1
            continue
        for a in (0, 1):
            for b in (0, 1):
                total += max(0, min(nprb, nz - sy - a)) * max(0, min(nprb, n - sx - b))
    return total, skipped


@pytest.mark.parametrize("case", ["a", "b", "c"])
def test_host_walk_visits_every_contribution_once(host_walk, case):
    if case == "c":                                                   # 300 positions: three chunks, a one-tile object
        rng = np.random.default_rng(6)
        scan, nz, n, nprb = rng.uniform(-2, 20, (1, 300, 2)).astype(np.float32), 13, 50, 9
    else:
        scan, nz, n, nprb = ref.case_a_scan() if case == "a" else ref.case_b_scan()
    errors, visits, skipped = host_walk(scan, nprb, nz, n)
    want, want_skipped = expected_visits(scan, nprb, nz, n)
    assert errors == 0
    assert (visits, skipped) == (want, want_skipped) and visits > 0


# ---- argument checks --------------------------------------------------------------------------------------------------
def test_gauge_symbols_are_declared_and_exported(nat):
    text = open(os.path.join(ROOT, "include", "ptycho_hip.h")).read()
    for name in ("ptycho_illumination", "ptycho_gauge_fit", "ptycho_gauge_apply"):
        assert "int %s(" % name in text
        assert name in nat.SYMBOLS and hasattr(nat.lib, name)
    assert "#define PTYCHO_GAUGE_WORK_PER_ANGLE %d\n" % nat.GAUGE_WORK_PER_ANGLE in text


def test_gauge_abi_rejects_bad_arguments_without_a_gpu(nat):
    d = ctypes.c_void_p(0x1000)              # never dereferenced: every rejection comes before any HIP call
    # ptycho_illumination(out, scan, probe, ptheta, nscan, nmodes, nprb, nz, n, stream)
    for args in ((None, d, d), (d, None, d), (d, d, None)):
        assert nat.illumination(*args, 1, 4, 1, 16, 64, 64, None) == 1
        assert b"null" in nat.last_error()
    for sizes in ((0, 4, 1, 16, 64, 64), (1, 0, 1, 16, 64, 64), (1, 4, 1, 0, 64, 64), (1, 4, 1, 16, 0, 64),
                  (1, 4, 1, 16, 64, 0)):
        assert nat.illumination(d, d, d, *sizes, None) == 1
        assert b"positive" in nat.last_error()
    for nmodes in (0, -1):
        assert nat.illumination(d, d, d, 1, 4, nmodes, 16, 64, 64, None) == 1
        assert b"nmodes" in nat.last_error()
    assert nat.illumination(d, d, d, 65536, 4, 1, 16, 64, 64, None) == 1
    assert b"ptheta" in nat.last_error()
    for sizes in ((1, 4, 1, 16, 16 * 65535 + 1, 64), (1, 4, 1, 16, 64, 2 ** 30 + 1), (1, 2 ** 31, 1, 16, 64, 64),
                  (1, 4, 1, 2 ** 30 + 1, 64, 64)):
        assert nat.illumination(d, d, d, *sizes, None) == 1
        assert b"too large" in nat.last_error()
    # ptycho_gauge_fit(gauge, psi, ref, weight, ptheta, nz, n, work, stream): ref and weight may be null
    for args in ((None, d, None, None, 1, 8, 8, d), (d, None, None, None, 1, 8, 8, d), (d, d, d, d, 1, 8, 8, None)):
        assert nat.gauge_fit(*args, None) == 1
        assert b"null" in nat.last_error()
    for sizes in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert nat.gauge_fit(d, d, None, None, *sizes, d, None) == 1
        assert b"positive" in nat.last_error()
    assert nat.gauge_fit(d, d, None, None, 65536, 8, 8, d, None) == 1
    assert nat.gauge_fit(d, d, None, None, 1, 2 ** 30 + 1, 8, d, None) == 1
    assert b"too large" in nat.last_error()
    # ptycho_gauge_apply(x, gauge, ptheta, ny, nx, which, stream)
    assert nat.gauge_apply(None, d, 1, 8, 8, 0, None) == 1
    assert nat.gauge_apply(d, None, 1, 8, 8, 0, None) == 1
    assert b"null" in nat.last_error()
    for sizes in ((0, 8, 8), (1, 0, 8), (1, 8, 0)):
        assert nat.gauge_apply(d, d, *sizes, 0, None) == 1
    for which in (-1, 2):
        assert nat.gauge_apply(d, d, 1, 8, 8, which, None) == 1
        assert b"which" in nat.last_error()
    assert nat.gauge_apply(d, d, 65536, 8, 8, 0, None) == 1
    assert nat.gauge_apply(d, d, 1, 2 ** 30, 2 ** 12, 1, None) == 1    # more workgroups than one grid axis holds
    assert b"too large" in nat.last_error()


def arrays(**over):
    a = {"scan": np.zeros((2, 5, 2), np.float32), "probe": np.zeros((2, 3, 8, 8), np.complex64),
         "psi": np.zeros((2, 20, 24), np.complex64), "weight": np.zeros((2, 20, 24), np.float32),
         "ref": np.zeros((2, 20, 24), np.complex64), "gauge": np.zeros((2, 6), np.float64)}
    a.update(over)
    return a


def test_checkers_accept_the_documented_shapes(lib):
    import torch
    a = arrays()
    assert lib.check_illumination(a["scan"], a["probe"], 20, 24) == (2, 5, 3, 8, 20, 24)
    assert lib.check_illumination(a["scan"], a["probe"][:, 0], 20, 24, np.zeros((2, 20, 24), np.float32))[2] == 1
    assert lib.check_fit(a["psi"], a["weight"], a["ref"]) == (2, 20, 24)
    assert lib.check_fit(a["psi"][0]) == (1, 20, 24)
    assert lib.check_apply(a["psi"], a["gauge"]) == (2, 1, 20, 24, 0)
    assert lib.check_apply(a["psi"][0], a["gauge"][0], "object") == (1, 1, 20, 24, 0)
    assert lib.check_apply(a["probe"], a["gauge"], "probe") == (2, 3, 8, 8, 1)
    assert lib.check_apply(a["probe"][:, 0], a["gauge"], "probe") == (2, 1, 8, 8, 1)
    assert lib.check_fix(a["psi"], a["scan"], a["probe"], 0.25, a["ref"]) == (2, 20, 24)
    assert lib.check_fix(a["psi"], a["scan"], a["probe"], 0, None) == (2, 20, 24)
    t = {k: torch.from_numpy(v) for k, v in a.items()}              # torch tensors on the host check alike
    assert lib.check_fix(t["psi"], t["scan"], t["probe"], 1.0, t["ref"]) == (2, 20, 24)
    assert lib.check_apply(t["probe"], t["gauge"], "probe") == (2, 3, 8, 8, 1)


@pytest.mark.parametrize("fn, over, exc, match", [
    ("illumination", {"scan": np.zeros((2, 5, 2), np.float64)}, TypeError, "scan must be float32"),
    ("illumination", {"probe": np.zeros((2, 3, 8, 8), np.complex128)}, TypeError, "probe must be complex64"),
    ("illumination", {"scan": [[0.0, 0.0]]}, TypeError, "scan must be an array"),
    ("illumination", {"scan": np.zeros((5, 2), np.float32)}, ValueError, "scan"),
    ("illumination", {"scan": np.zeros((2, 5, 3), np.float32)}, ValueError, "nscan, 2"),
    ("illumination", {"scan": np.zeros((2, 0, 2), np.float32)}, ValueError, "non-empty"),
    ("illumination", {"probe": np.zeros((8, 8), np.complex64)}, ValueError, "probe"),
    ("illumination", {"probe": np.zeros((2, 3, 8, 9), np.complex64)}, ValueError, "square"),
    ("illumination", {"probe": np.zeros((3, 3, 8, 8), np.complex64)}, ValueError, "ptheta"),
    ("illumination", {"nz": 0}, ValueError, "nz"),
    ("illumination", {"n": 2.5}, ValueError, "n must"),
    ("illumination", {"out": np.zeros((2, 20, 25), np.float32)}, ValueError, "out must be"),
    ("illumination", {"out": np.zeros((2, 20, 24), np.float64)}, TypeError, "out must be float32"),
    ("fit", {"psi": np.zeros((2, 20, 24), np.complex128)}, TypeError, "psi must be complex64"),
    ("fit", {"psi": np.zeros((24,), np.complex64)}, ValueError, "psi"),
    ("fit", {"weight": np.zeros((2, 20, 24), np.float64)}, TypeError, "weight must be float32"),
    ("fit", {"weight": np.zeros((2, 20, 23), np.float32)}, ValueError, "weight must have"),
    ("fit", {"ref": np.zeros((2, 20, 24), np.float32)}, TypeError, "ref must be complex64"),
    ("fit", {"ref": np.zeros((1, 20, 24), np.complex64)}, ValueError, "ref must have"),
    ("apply", {"which": "both"}, ValueError, "which"),
    ("apply", {"psi": np.zeros((2, 20, 24), np.float32)}, TypeError, "x must be complex64"),
    ("apply", {"psi": np.zeros((2, 2, 20, 24), np.complex64)}, ValueError, "x must have"),
    ("apply", {"psi": np.zeros((8, 8), np.complex64), "which": "probe"}, ValueError, "x must have"),
    ("apply", {"gauge": np.zeros((2, 6), np.float32)}, TypeError, "gauge must be float64"),
    ("apply", {"gauge": np.zeros((3, 6), np.float64)}, ValueError, "gauge must be"),
    ("apply", {"gauge": np.zeros((2, 5), np.float64)}, ValueError, "gauge must be"),
    ("apply", {"gauge": np.zeros((6,), np.float64)}, ValueError, "gauge must be"),
    ("fix", {"floor": -0.1}, ValueError, "floor"),
    ("fix", {"floor": 1.5}, ValueError, "floor"),
    ("fix", {"floor": float("nan")}, ValueError, "floor"),
    ("fix", {"floor": "0.1"}, ValueError, "floor"),
    ("fix", {"scan": np.zeros((3, 5, 2), np.float32), "probe": np.zeros((3, 8, 8), np.complex64)}, ValueError, "ptheta"),
    ("fix", {"ref": np.zeros((2, 20, 20), np.complex64)}, ValueError, "ref must have"),
    ("fix", {"probe": np.zeros((2, 3, 8, 8), np.complex128)}, TypeError, "probe must be complex64"),
])
def test_bad_arguments_raise_before_device_use(lib, fn, over, exc, match):
    import torch
    import libtike.hipfft as pt
    a = arrays(nz=20, n=24, out=None, which="object", floor=0.1)
    a.update(over)
    calls = {
        "illumination": (lib.check_illumination, pt.illumination, lambda v: (v["scan"], v["probe"], v["nz"], v["n"], v["out"])),
        "fit": (lib.check_fit, pt.fit_gauge, lambda v: (v["psi"], v["weight"], v["ref"])),
        "apply": (lib.check_apply, pt.apply_gauge, lambda v: (v["psi"], v["gauge"], v["which"])),
        "fix": (lib.check_fix, pt.fix_gauge, lambda v: (v["psi"], v["scan"], v["probe"], v["floor"], v["ref"])),
    }
    checker, public, pick = calls[fn]
    as_torch = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in a.items()}
    for values in (a, as_torch):
        with pytest.raises(exc, match=match):
            checker(*pick(values))
        with pytest.raises(exc, match=match):                         # the public function checks first
            public(*pick(values))


def test_host_operands_are_refused(lib):
    import torch
    a = {k: torch.from_numpy(v) for k, v in arrays().items()}
    with pytest.raises(ValueError, match="device tensors"):
        lib.illumination(a["scan"], a["probe"], 20, 24)
    with pytest.raises(ValueError, match="device tensors"):
        lib.fit_gauge(a["psi"])
    with pytest.raises(ValueError, match="device tensors"):
        lib.apply_gauge(a["psi"], a["gauge"])


def test_gauge_functions_are_exported_with_their_documented_signatures():
    import libtike.hipfft as pt
    import libtike.cufft as alias
    want = {"illumination": ["scan", "probe", "nz", "n", "out"], "fit_gauge": ["psi", "weight", "ref"],
            "apply_gauge": ["x", "gauge", "which"], "fix_gauge": ["psi", "scan", "probe", "floor", "ref"]}
    for name, params in want.items():
        assert getattr(pt, name) is getattr(alias, name)
        assert list(inspect.signature(getattr(pt, name)).parameters) == params
    sig = inspect.signature(pt.fix_gauge).parameters
    assert sig["floor"].default == 0.1 and sig["ref"].default is None
    assert inspect.signature(pt.apply_gauge).parameters["which"].default == "object"
    assert inspect.signature(pt.illumination).parameters["out"].default is None
