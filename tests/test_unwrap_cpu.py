"""Phase unwrapping, host side: the NumPy restatement of tests/unwrap_ref.py held against a sparse direct solve and its
own planted truth, the conditions that the cases of tests/test_hip_unwrap.py rely on, the tile / halo index logic of
csrc/k_unwrap.hpp built with the host compiler and walked as the kernels walk it, and the argument checks of the C ABI
and of ``libtike.hipfft.unwrap``.  No GPU needed."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_build  # noqa: E402
import unwrap_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libtike-cufft_amd", "csrc")
TWO_PI = 2.0 * np.pi


@pytest.fixture(scope="module")
def lib():
    import libtike.hipfft.unwrap as lib
    return lib


@pytest.fixture(scope="module")
def nat():
    from libtike.hipfft import _native
    return _native


def ellipse(nz=67, n=129):
    y, x = np.meshgrid(np.arange(nz), np.arange(n), indexing="ij")
    return (((y - 33) / 30.0) ** 2 + ((x - 64) / 60.0) ** 2 < 1).astype(np.float32)


def noisy(sigma=0.6):
    truth = ref.make_truth(67, 129, 25)
    return truth, ref.wrap(truth + np.random.default_rng(11).normal(0, sigma, truth.shape)).astype(np.float32)


# ---- the restatement ------------------------------------------------------------------------------------------------------
def components(w):
    """Labels of the 4-connected regions of positive weight (0: none), by flood fill over the weighted edges."""
    lab = np.zeros(w.shape, np.int64)
    cur = 0
    for y0, x0 in zip(*np.nonzero(w > 0)):
        if lab[y0, x0]:
            continue
        cur += 1
        lab[y0, x0] = cur
        stack = [(y0, x0)]
        while stack:
            y, x = stack.pop()
            for yy, xx in ((y, x - 1), (y, x + 1), (y - 1, x), (y + 1, x)):
                if 0 <= yy < w.shape[0] and 0 <= xx < w.shape[1] and w[yy, xx] > 0 and not lab[yy, xx]:
                    lab[yy, xx] = cur
                    stack.append((yy, xx))
    return lab


@pytest.mark.parametrize("case", ["plain", "ellipse", "two regions", "ragged weights"])
def test_restatement_solves_the_normal_equations(case):
    """PCG at a tight tolerance against ``spsolve`` on the same ``L``, ``b`` with one pixel pinned per component, both
    after removal of the weighted mean per component."""
    from scipy.sparse.linalg import spsolve
    import scipy.sparse as sp
    rng = np.random.default_rng(5)
    nz, n = 23, 37
    phase = ref.wrap(ref.make_truth(nz, n, 9.0) + rng.normal(0, 0.5, (nz, n))).astype(np.float32)
    weight = {"plain": None, "ellipse": ellipse(67, 129)[22:45, 46:83].copy(),
              "two regions": np.ones((nz, n), np.float32), "ragged weights": rng.uniform(0.1, 3.0, (nz, n)).astype(np.float32)}[case]
    if case == "two regions":
        weight[:, 17:19] = 0
    if case == "ragged weights":
        weight[rng.uniform(size=(nz, n)) < 0.1] = 0
    wx, dx, wy, dy = ref.edges(phase, weight)
    b = ref.rhs(wx, dx, wy, dy)
    x, info = ref.pcg(wx, wy, b, tol=1e-13, maxiter=5000)
    assert info["converged"]
    L = ref.system(wx, wy)
    assert np.allclose(L @ np.ones(nz * n), 0, atol=1e-12)              # constants are in the null space
    assert np.allclose((L @ x.ravel()).reshape(nz, n), ref.apply_L(x, wx, wy), atol=1e-11)
    D = ref.diagonal(wx, wy)
    assert np.array_equal(L.diagonal().reshape(nz, n), D)
    lab = components(ref.effective_weight(weight, (nz, n)) * (D > 0))
    ncomp = lab.max()
    assert ncomp >= {"plain": 1, "ellipse": 1, "two regions": 2, "ragged weights": 1}[case]
    free = np.ones(nz * n, bool)
    free[~(D > 0).ravel()] = False
    for c in range(1, ncomp + 1):
        free[np.flatnonzero(lab.ravel() == c)[0]] = False                 # pin one pixel of the component to 0
    keep = np.flatnonzero(free)
    sol = np.zeros(nz * n)
    sol[keep] = spsolve(sp.csc_matrix(L[keep][:, keep]), b.ravel()[keep])
    sol = sol.reshape(nz, n)
    w = ref.effective_weight(weight, (nz, n))
    for c in range(1, ncomp + 1):
        m = lab == c
        a_ = x[m] - np.average(x[m], weights=w[m])
        b_ = sol[m] - np.average(sol[m], weights=w[m])
        assert np.abs(a_ - b_).max() <= 1e-9 * max(1.0, np.abs(b_).max())
    assert (x[~(D > 0)] == 0).all()


@pytest.mark.parametrize("shape, amp", [((67, 129), 25.0), ((67, 129), 12.0), ((67, 129), -18.0), ((65, 257), 20.0),
                                        ((17, 65), 6.0), ((2, 2), 1.0), ((2, 300), 1.0), ((300, 2), 1.0)])
def test_restatement_recovers_the_truth_up_to_one_integer(shape, amp):
    truth = ref.make_truth(shape[0], shape[1], amp)
    assert max(np.abs(np.diff(truth, axis=0)).max(), np.abs(np.diff(truth, axis=1)).max()) < 2.0
    phi = ref.wrap(truth).astype(np.float32)
    for dtype in (np.float64, np.float32):
        out = ref.unwrap(phi, dtype=dtype)
        assert out["converged"] and out["residues"] == 0 and out["phase"].dtype == np.float32
        k = (out["phase"].astype(np.float64) - truth) / TWO_PI
        assert np.ptp(np.rint(k)) == 0
        assert np.abs(k - np.rint(k)).max() * TWO_PI <= np.spacing(np.float32(np.abs(out["phase"]).max()))
    if shape == (67, 129) and amp == 25.0:
        assert np.ptp(truth) > 7 * TWO_PI and np.abs(np.diff(truth, axis=1)).max() <= 1.5


def test_only_multiples_of_two_pi_are_changed_and_smooth_mode_is_not_congruent():
    truth, phi = noisy()
    con, smooth = ref.unwrap(phi, tol=1e-6), ref.unwrap(phi, tol=1e-6, congruent=False)
    k = (con["phase"].astype(np.float64) - phi) / TWO_PI
    assert np.abs(k - np.rint(k)).max() < 1e-6 and np.ptp(np.rint(k)) >= 7
    assert np.abs(ref.wrap(smooth["phase"].astype(np.float64) - phi)).max() > 0.1


# ---- the conditions of the GPU cases, for the restatement alone -------------------------------------------------------------
def test_case_conditions_hold_for_the_restatement():
    # case 2: a weighted support in noise; garbage outside changes nothing inside
    truth = ref.make_truth(67, 129, 25)
    w = ellipse()
    rng = np.random.default_rng(2)
    a = np.where(w > 0, ref.wrap(truth), rng.uniform(-np.pi, np.pi, truth.shape)).astype(np.float32)
    b = np.where(w > 0, ref.wrap(truth), rng.uniform(-np.pi, np.pi, truth.shape)).astype(np.float32)
    off = np.flatnonzero(w.ravel() == 0)[::max(1, (w == 0).sum() // 20)][:20]
    b.ravel()[off[::2]], b.ravel()[off[1::2]] = np.nan, np.inf
    oa, ob = ref.unwrap(a, w), ref.unwrap(b, w)
    assert oa["converged"] and oa["iterations"] == ob["iterations"] and oa["residual"] == ob["residual"]
    m = w > 0
    assert (oa["D"] > 0)[m].all() and not (oa["D"] > 0)[~m].any()
    assert np.array_equal(oa["phase"][m], ob["phase"][m]) and np.array_equal(ob["phase"][~m], b[~m], equal_nan=True)
    k = (oa["phase"].astype(np.float64) - truth)[m] / TWO_PI
    assert np.ptp(np.rint(k)) == 0
    # case 3: residues inside, at most 2 % of the pixels within 0.01 of a half-integer
    _, phi = noisy()
    r64, r32 = ref.unwrap(phi, tol=1e-6), ref.unwrap(phi, tol=1e-6, dtype=np.float32)
    frac = np.abs(r64["k"] - np.floor(r64["k"]) - 0.5) < 0.01
    assert frac.mean() <= 0.02
    assert r64["residues"] == r32["residues"] > 0 and r64["converged"] and r32["converged"]
    assert abs(r64["iterations"] - r32["iterations"]) <= 2
    # case 4: two regions, each flat against the truth in least-squares mode
    w2 = np.ones(truth.shape, np.float32)
    w2[:, 60:63] = 0
    phi2 = np.where(w2 > 0, ref.wrap(truth), rng.uniform(-np.pi, np.pi, truth.shape)).astype(np.float32)
    out = ref.unwrap(phi2, w2, congruent=False, tol=1e-6)
    for cols in (slice(0, 60), slice(63, None)):
        d = out["phase"].astype(np.float64)[:, cols] - truth[:, cols]
        assert np.ptp(d) < 1e-3
    # case 5: a vortex pair
    y, x = np.meshgrid(np.arange(67.0), np.arange(129.0), indexing="ij")
    vort = (np.arctan2(y - 20.5, x - 40.5) - np.arctan2(y - 45.5, x - 90.5)).astype(np.float32)
    charge, count = ref.residues(vort, dtype=np.float32)
    assert count == 2 and charge[20, 40] == 1 and charge[45, 90] == -1 and np.abs(charge).sum() == 2
    wv = np.ones(vort.shape, np.float32)
    wv[43:48, 88:93] = 0
    charge, count = ref.residues(vort, wv, dtype=np.float32)
    assert count == 1 and charge[45, 90] == 0 and charge[20, 40] == 1


def test_weights_that_are_not_positive_and_finite_count_as_zero():
    truth = ref.make_truth(17, 33, 6.0)
    phi = ref.wrap(truth).astype(np.float32)
    w0 = np.ones(phi.shape, np.float32)
    w0[4:7, 5:9] = 0
    w1 = w0.copy()
    w1[4:7, 5:9] = np.array([-1.0, np.nan, np.inf, -np.inf], np.float32)
    a, b = ref.unwrap(phi, w0), ref.unwrap(phi, w1)
    assert np.array_equal(a["phase"], b["phase"]) and a["iterations"] == b["iterations"]
    zero = ref.unwrap(phi, np.zeros_like(phi))
    assert zero["iterations"] == 0 and zero["converged"] and np.array_equal(zero["phase"], phi) and zero["offset"] == 0.0
    flat = ref.unwrap(np.full((9, 12), 0.75, np.float32))
    assert flat["iterations"] == 0 and flat["converged"] and np.array_equal(flat["phase"], np.full((9, 12), 0.75, np.float32))
    five = ref.unwrap(phi, maxiter=5)
    assert five["iterations"] == 5 and five["status"] == 3 and not five["converged"]


# ---- the tile / halo index logic of csrc/k_unwrap.hpp, built for the host ---------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    program = host_build.build("host_unwrap", tmp_path_factory.mktemp("unwrap"))
    return lambda *args: program(*args).stdout


def test_host_walk_owns_every_pixel_once_and_visits_every_edge_from_both_ends(host, nat):
    text = host()
    assert "host_unwrap: 0 errors" in text and int(text.split()[3]) == 48 * 192   # nz 2 .. 49, n 2 .. 193
    for nz, n in ((67, 129), (65, 257), (17, 65), (2, 2), (2, 300), (300, 2), (96, 160), (64, 128), (1000, 3)):
        errors, tiles, owned, visits = (int(v) for v in host(nz, n).split())
        assert errors == 0 and owned == nz * n and visits == 2 * (nz * (n - 1) + (nz - 1) * n)
        assert tiles == -(-nz // 16) * -(-n // 64)
        assert nat.unwrap_work_words(3, nz, n) == 3 * tiles * 2            # the library plans as the host build does
        assert nat.unwrap_buffer_floats(3, nz, n) == 3 * 6 * nz * n


# ---- argument checks ------------------------------------------------------------------------------------------------------
NAMES = {"ptycho_unwrap_work_words": "size_t", "ptycho_unwrap_buffer_floats": "size_t", "ptycho_unwrap_begin": "int",
         "ptycho_unwrap_iterate": "int", "ptycho_unwrap_finish": "int", "ptycho_unwrap_residues": "int"}


def test_unwrap_symbols_are_declared_and_exported(nat):
    text = open(os.path.join(ROOT, "include", "ptycho_hip.h")).read()
    for name, res in NAMES.items():
        assert "%s %s(" % (res, name) in text
        assert name in nat.SYMBOLS and hasattr(nat.lib, name)
    assert "#define PTYCHO_UNWRAP_STATE_WORDS 16" in text and nat.UNWRAP_STATE_WORDS == 16
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_unwrap.hpp" in make and "host_unwrap.hpp" in make and "host_unwrap:" in make


def test_unwrap_abi_rejects_bad_arguments_without_a_gpu(nat):
    d = ctypes.c_void_p(0x1000)              # never dereferenced: every rejection comes before any HIP call
    calls = {
        "begin": (nat.unwrap_begin, dict(buf=d, state=d, phase=d, weight=None, ptheta=1, nz=8, n=8, work=d), ("buf", "state", "phase", "work")),
        "iterate": (nat.unwrap_iterate, dict(buf=d, state=d, weight=None, ptheta=1, nz=8, n=8, niter=1, maxiter=4, tol=1e-4, work=d),
                    ("buf", "state", "work")),
        "finish": (nat.unwrap_finish, dict(out=d, state=d, buf=d, phase=d, weight=None, congruent=1, ptheta=1, nz=8, n=8, work=d),
                   ("out", "state", "buf", "phase", "work")),
        "residues": (nat.unwrap_residues, dict(charge=None, count=d, phase=d, weight=None, ptheta=1, nz=8, n=8), ("count", "phase")),
    }
    for fn, ok, required in calls.values():
        call = lambda **over: fn(*{**ok, **over}.values(), None)   # noqa: E731
        for name in required:
            assert call(**{name: None}) == 1
            assert b"null" in nat.last_error()
        for over in (dict(nz=1), dict(n=1), dict(nz=0), dict(n=0)):
            assert call(**over) == 1
            assert b"at least 2" in nat.last_error()
        for over in (dict(nz=2 ** 16, n=2 ** 15), dict(nz=2 ** 31, n=2), dict(nz=2, n=2 ** 40)):
            assert call(**over) == 1
            assert b"2^31" in nat.last_error()
        for bad in (0, 65536):
            assert call(ptheta=bad) == 1
            assert b"ptheta" in nat.last_error()
    fn, ok, _ = calls["iterate"]
    call = lambda **over: fn(*{**ok, **over}.values(), None)   # noqa: E731
    for over in (dict(niter=-1), dict(maxiter=-1)):
        assert call(**over) == 1
        assert b"negative" in nat.last_error()
    for bad in (-1e-3, float("nan"), float("inf"), -float("inf")):
        assert call(tol=bad) == 1
        assert b"tol" in nat.last_error()
    for sizes in ((0, 8, 8), (65536, 8, 8), (1, 1, 8), (1, 8, 1), (1, 2 ** 16, 2 ** 15)):
        assert nat.unwrap_work_words(*sizes) == 0 and nat.unwrap_buffer_floats(*sizes) == 0
    assert nat.unwrap_work_words(1, 2304, 2304) == 36 * 144 * 2
    assert nat.unwrap_buffer_floats(65535, 2, 2 ** 30 - 1) == 65535 * 6 * 2 * (2 ** 30 - 1)


def arrays(**over):
    a = {"x": np.zeros((2, 9, 12), np.float32), "weight": np.ones((2, 9, 12), np.float32), "congruent": True, "tol": 1e-4,
         "maxiter": None, "check_every": 256, "out": None}
    a.update(over)
    return a


def test_checker_accepts_the_documented_shapes(lib):
    import torch
    assert lib.check_unwrap(**arrays()) == (2, 9, 12, 96)
    assert lib.check_unwrap(np.zeros((40, 7), np.complex64), np.ones((40, 7), bool), False, 0.0, 0, 1) == (1, 40, 7, 0)
    assert lib.check_unwrap(np.zeros((2, 2), np.float64), maxiter=np.int64(3)) == (1, 2, 2, 3)
    t = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in arrays().items()}
    t["out"] = torch.zeros((2, 9, 12))
    assert lib.check_unwrap(**t) == (2, 9, 12, 96)


@pytest.mark.parametrize("over, exc, match", [
    ({"x": [[0.0]]}, TypeError, "x must be an array"),
    ({"x": np.zeros((2, 9, 12), np.int32)}, TypeError, "x must be .*got int32"),
    ({"x": np.zeros((12,), np.float32)}, ValueError, r"x must be \[nz, n\] or \[ptheta, nz, n\]"),
    ({"x": np.zeros((1, 2, 9, 12), np.float32)}, ValueError, r"x must be \[nz, n\] or \[ptheta, nz, n\]"),
    ({"x": np.zeros((2, 1, 12), np.float32), "weight": None}, ValueError, "nz >= 2, n >= 2"),
    ({"x": np.zeros((0, 9, 12), np.float32), "weight": None}, ValueError, "ptheta in"),
    ({"weight": np.ones((2, 9, 12), np.float64)}, TypeError, "weight must be float32 or bool, got float64"),
    ({"weight": np.ones((9, 12), np.float32)}, ValueError, r"weight must have x's shape \(2, 9, 12\)"),
    ({"weight": 1.0}, TypeError, "weight must be an array"),
    ({"congruent": 1}, TypeError, "congruent must be a bool"),
    ({"tol": -1e-3}, ValueError, "tol must be"),
    ({"tol": float("nan")}, ValueError, "tol must be"),
    ({"tol": float("inf")}, ValueError, "tol must be"),
    ({"tol": "tight"}, ValueError, "tol must be"),
    ({"maxiter": -1}, ValueError, "maxiter must be"),
    ({"maxiter": 10.0}, ValueError, "maxiter must be"),
    ({"maxiter": True}, ValueError, "maxiter must be"),
    ({"check_every": 0}, ValueError, "check_every must be"),
    ({"check_every": 2.5}, ValueError, "check_every must be"),
    ({"out": np.zeros((2, 9, 12), np.float64)}, TypeError, "out must be float32"),
    ({"out": np.zeros((9, 12), np.float32)}, ValueError, r"out must have x's shape"),
])
def test_bad_arguments_raise_before_device_use(lib, over, exc, match):
    import torch
    import libtike.hipfft as pt
    a = arrays(**over)
    as_torch = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in a.items()}
    for v in (a, as_torch):
        with pytest.raises(exc, match=match):
            lib.check_unwrap(**v)
        with pytest.raises(exc, match=match):                             # the public function checks first
            pt.unwrap_phase(**v)
    if set(over) <= {"x", "weight"}:
        with pytest.raises(exc, match=match):
            pt.phase_residues(a["x"], a["weight"])


def test_host_tensors_are_refused(lib):
    import torch
    with pytest.raises(ValueError, match="device tensors or NumPy arrays"):
        lib.unwrap_phase(torch.zeros((8, 8), dtype=torch.float32))
    with pytest.raises(ValueError, match="device tensors or NumPy arrays"):
        lib.phase_residues(np.zeros((8, 8), np.float32), torch.ones((8, 8), dtype=torch.float32))


def test_unwrap_functions_are_exported_with_their_documented_signatures(lib):
    import libtike.hipfft as pt
    assert pt.unwrap_phase is lib.unwrap_phase and pt.phase_residues is lib.phase_residues
    assert lib.__all__ == ["unwrap_phase", "phase_residues", "check_unwrap"]
    sig = inspect.signature(pt.unwrap_phase).parameters
    assert list(sig) == ["x", "weight", "congruent", "tol", "maxiter", "check_every", "out"]
    assert [sig[k].default for k in list(sig)[1:]] == [None, True, 1e-4, None, 256, None]
    assert inspect.signature(lib.check_unwrap) == inspect.signature(pt.unwrap_phase)
    sig = inspect.signature(pt.phase_residues).parameters
    assert list(sig) == ["x", "weight"] and sig["weight"].default is None
