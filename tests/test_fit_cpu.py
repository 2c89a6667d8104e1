"""Fit residuals, host side: the NumPy restatement of tests/fit_ref.py held to its identities, the partition of
csrc/k_fit.hpp built with the host compiler and walked as the kernels walk it, and the argument checks of the C ABI and
of ``libtike.hipfft.fit``.  No GPU needed."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_build  # noqa: E402
import fit_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    import libtike.hipfft.fit as lib
    return lib


@pytest.fixture(scope="module")
def nat():
    from libtike.hipfft import _native
    return _native


# ---- the restatement --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["A", "B", "C", "F"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_restatement_identities(name, dtype):
    g, data = ref.make_case(name)
    mask = ref.make_mask(data.shape[-1])
    for m in (None, mask):
        plain = ref.frames_pixels(g, data, m, None, dtype)
        ab = (plain["frames"][..., 2].sum(), plain["frames"][..., 0].sum())
        for out in (plain, ref.frames_pixels(g, data, m, ab, dtype)):
            f, p = out["frames"], out["pixels"]
            assert f.shape == data.shape[:2] + (8,) and p.shape == (data.shape[0], 4) + data.shape[2:]
            assert f.dtype == np.float64 and p.dtype == np.float64 and np.isfinite(f).all() and np.isfinite(p).all()
            # half the Poisson deviance of a frame is not negative: x - d ln x has its minimum at x = d
            assert (f[..., 4] - f[..., 5] >= -16 * ref.ULP * (out["frames_mag"][..., 4] + out["frames_mag"][..., 5])).all()
            for col, mp in ((0, 0), (1, 1), (3, 3)):   # the same terms summed over pixels first or over frames first
                assert np.allclose(p[:, mp].sum((-2, -1)), f[..., col].sum(1), rtol=1e-12, atol=0)
            slack = 1 + 1e-6                                           # float32 terms: (sqrt I)^2 may round above I
            assert (np.abs(f) <= out["frames_mag"] * slack).all() and (np.abs(p) <= out["pixels_mag"] * slack).all()
            if m is not None:
                assert (p[:, :, m == 0] == 0).all()


def test_restatement_planted_frames_and_scale():
    g, data = ref.make_case("C")
    out = ref.frames_pixels(g, data)
    f = out["frames"]
    assert (f[0, 1] == 0).all()                                        # g = 0, d = 0: every term is 0
    assert f[0, 2, 1] == 0 and f[0, 2, 0] > 0 and f[0, 2, 3] == pytest.approx(f[0, 2, 0])   # d = 0: cost = sum I
    a, b = f[..., 2].sum(), f[..., 0].sum()
    scaled = ref.frames_pixels(g, data, None, (a, b))["frames"]
    assert scaled[..., 0].sum() == pytest.approx(b * (a / b) ** 2, rel=1e-12)
    assert scaled[..., 3].sum() < f[..., 3].sum()                      # a / b minimises the gaussian cost over scales
    f32 = ref.frames_pixels(g, data, None, (a, b), np.float32)
    err = np.abs(f32["frames"] - scaled) / (ref.ULP * ref.frames_pixels(g, data, None, (a, b))["frames_mag"] + 1e-300)
    assert err.max() < 1.0, err.max()                                  # float32 terms: well inside 2^-23 of the magnitudes


def test_unmeasured_pixels_may_hold_anything_in_the_restatement():
    g, data = ref.make_case("B")
    mask = ref.make_mask(data.shape[-1])
    want = ref.frames_pixels(g, data, mask)
    bad_d, bad_g = data.copy(), g.copy()
    bad_d[..., mask == 0] = np.nan
    bad_g[..., mask == 0] = np.inf
    got = ref.frames_pixels(bad_g, bad_d, mask)
    assert np.array_equal(got["frames"], want["frames"]) and np.array_equal(got["pixels"], want["pixels"])


# ---- the partition of csrc/k_fit.hpp, built for the host ------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_walk(tmp_path_factory):
    program = host_build.build("host_fit", tmp_path_factory.mktemp("fit"))
    return lambda ptheta, nscan, npix: [int(v) for v in program(ptheta, nscan, npix).stdout.split()]


WALK_SHAPES = [(pt_, ns, nd * nd) for pt_, ns, nd, _ in ref.CASES.values()] + [
    (1, 4096, 65536), (1, 1, 4), (3, 5, 1_048_576),
    (1, 129, 513), (2, 100_000, 49), (1, 257, 2049), (7, 300, 2048), (1, 40_000, 9)]


@pytest.mark.parametrize("shape", WALK_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_host_walk_visits_every_pair_and_every_word_once(host_walk, nat, shape):
    errors, words, cap, nranges, nwt = host_walk(*shape)
    assert errors == 0
    assert words <= cap == max(1 << 20, shape[0] * shape[1] * shape[2]) // 8
    assert words == nat.fit_work_words(*shape)                         # the library plans as the host build does
    assert nwt == -(-shape[2] // 512) and 1 <= nranges <= max(1, -(-shape[1] // 128))


def test_the_cases_reach_the_paths_they_are_named_for(host_walk):
    plan = {k: host_walk(v[0], v[1], v[2] * v[2])[3:] for k, v in ref.CASES.items()}
    assert plan["A"] == [1, 1] and plan["B"] == [1, 1] and plan["F"] == [1, 1]
    assert plan["C"][0] > 1 and plan["C"][1] > 4                       # frame ranges; wave tiles of two workgroups
    assert plan["D"] == [1, 32] and plan["E"][0] > 2 and plan["E"][1] == 2
    assert host_walk(1, 4096, 65536)[3] * (65536 // 2048) >= 4 * 256   # the flagship grid: four workgroups per compute unit


# ---- argument checks --------------------------------------------------------------------------------------------------
def test_fit_symbols_are_declared_and_exported(nat):
    text = open(os.path.join(ROOT, "include", "ptycho_hip.h")).read()
    for name, res in (("ptycho_fit_accumulate", "int"), ("ptycho_fit_work_words", "size_t"), ("ptycho_fit_frames", "int")):
        assert "%s %s(" % (res, name) in text
        assert name in nat.SYMBOLS and hasattr(nat.lib, name)


def test_fit_abi_rejects_bad_arguments_without_a_gpu(nat):
    d = ctypes.c_void_p(0x1000)              # never dereferenced: every rejection comes before any HIP call
    # ptycho_fit_accumulate(inten, g, count, add, stream)
    for args in ((None, d, 8), (d, None, 8)):
        assert nat.fit_accumulate(*args, 0, None) == 1
        assert b"null" in nat.last_error()
    assert nat.fit_accumulate(d, d, 0, 0, None) == 1
    assert b"positive" in nat.last_error()
    assert nat.fit_accumulate(d, d, 2 ** 60, 1, None) == 1
    assert b"too large" in nat.last_error()
    # ptycho_fit_frames(frames, pixels, inten, g, data, mask, ab, ptheta, nscan, npix, work, stream): pixels, mask, ab and
    # one of inten / g may be null
    ok = dict(frames=d, pixels=None, inten=None, g=d, data=d, mask=None, ab=None, ptheta=1, nscan=4, npix=256, work=d)
    call = lambda **over: nat.fit_frames(*{**ok, **over}.values(), None)   # noqa: E731
    for name in ("frames", "data", "work"):
        assert call(**{name: None}) == 1
        assert b"null" in nat.last_error()
    assert call(g=None) == 1
    assert b"both" in nat.last_error()
    for name in ("ptheta", "nscan", "npix"):
        assert call(**{name: 0}) == 1
        assert b"positive" in nat.last_error()
    assert call(ptheta=65536) == 1
    assert b"ptheta" in nat.last_error()
    for over in (dict(nscan=2 ** 31), dict(npix=2 ** 31), dict(ptheta=65535, nscan=2 ** 30, npix=2 ** 30),
                 dict(nscan=2 ** 31 - 1, npix=2 ** 31 - 1)):
        assert call(**over) == 1
        assert b"too large" in nat.last_error()
    # ptycho_fit_work_words: 0 for the same sizes
    for sizes in ((0, 4, 256), (1, 0, 256), (1, 4, 0), (65536, 4, 256), (1, 2 ** 31, 4), (1, 4, 2 ** 31),
                  (65535, 2 ** 30, 2 ** 30)):
        assert nat.fit_work_words(*sizes) == 0
    assert nat.fit_work_words(1, 4, 256) == 0                          # one wave tile, one range: nothing to fold
    assert nat.fit_work_words(1, 4096, 65536) == 4096 * 128 * 8 + 32 * 4 * 65536


def arrays(**over):
    shape = (2, 5, 12, 12)
    a = {"data": np.zeros(shape, np.float32), "farplane": np.zeros(shape, np.complex64),
         "intensity": np.zeros(shape, np.float32), "mask": np.ones((12, 12), np.uint8), "ab": np.ones(2, np.float64)}
    a.update(over)
    return a


def test_checker_accepts_the_documented_shapes(lib):
    import torch
    a = arrays()
    assert lib.check_fit_frames(a["data"], a["farplane"]) == (2, 5, 12)
    assert lib.check_fit_frames(a["data"], None, a["intensity"]) == (2, 5, 12)
    assert lib.check_fit_frames(a["data"], a["farplane"], a["intensity"], a["mask"], a["ab"]) == (2, 5, 12)
    assert lib.check_fit_frames(a["data"], a["farplane"], mask=a["mask"].astype(bool)) == (2, 5, 12)
    t = {k: torch.from_numpy(v) for k, v in a.items()}                # torch tensors on the host check alike
    assert lib.check_fit_frames(t["data"], t["farplane"], t["intensity"], t["mask"], t["ab"]) == (2, 5, 12)


@pytest.mark.parametrize("over, exc, match", [
    ({"data": np.zeros((2, 5, 12, 12), np.float64)}, TypeError, "data must be float32"),
    ({"data": [[0.0]]}, TypeError, "data must be an array"),
    ({"data": np.zeros((5, 12, 12), np.float32)}, ValueError, r"data must have 4 .*\(5, 12, 12\)"),
    ({"data": np.zeros((2, 5, 12, 13), np.float32)}, ValueError, r"ndet, ndet\], got \(2, 5, 12, 13\)"),
    ({"data": np.zeros((2, 0, 12, 12), np.float32)}, ValueError, "non-empty"),
    ({"farplane": None, "intensity": None}, ValueError, "at least one of farplane and intensity"),
    ({"farplane": np.zeros((2, 5, 12, 12), np.complex128)}, TypeError, "farplane must be complex64"),
    ({"farplane": np.zeros((2, 4, 12, 12), np.complex64)}, ValueError, r"farplane must have data's shape .*\(2, 4, 12, 12\)"),
    ({"intensity": np.zeros((2, 5, 12, 12), np.float64)}, TypeError, "intensity must be float32"),
    ({"intensity": np.zeros((1, 5, 12, 12), np.float32)}, ValueError, r"intensity must have data's shape .*\(1, 5, 12, 12\)"),
    ({"mask": [[1]]}, TypeError, "mask must be an array"),
    ({"mask": np.ones((2, 12, 12), np.uint8)}, ValueError, r"mask must be \(12, 12\), got shape \(2, 12, 12\)"),
    ({"mask": np.ones((12, 11), np.uint8)}, ValueError, r"mask must be \(12, 12\)"),
    ({"ab": np.ones(2, np.float32)}, TypeError, "ab must be float64"),
    ({"ab": np.ones(3, np.float64)}, ValueError, r"ab must hold .*\(3,\)"),
    ({"ab": np.ones((1, 2), np.float64)}, ValueError, "ab must have 1"),
])
def test_bad_arguments_raise_before_device_use(lib, over, exc, match):
    import torch
    import libtike.hipfft as pt
    a = arrays(**over)
    as_torch = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in a.items()}
    for v in (a, as_torch):
        args = (v["data"], v["farplane"], v["intensity"], v["mask"], v["ab"])
        with pytest.raises(exc, match=match):
            lib.check_fit_frames(*args)
        with pytest.raises(exc, match=match):                         # the public function checks first
            pt.fit_frames(*args)


def test_host_operands_are_refused(lib):
    import torch
    a = {k: torch.from_numpy(v) for k, v in arrays().items()}
    with pytest.raises(ValueError, match="device tensors"):
        lib.fit_frames(a["data"], a["farplane"])
    with pytest.raises(ValueError, match="device tensors"):
        lib.accumulate_intensity(a["farplane"])
    with pytest.raises(TypeError, match="farplane must be complex64"):
        lib.accumulate_intensity(a["data"])
    with pytest.raises(ValueError, match="out must have farplane's shape"):
        lib.accumulate_intensity(a["farplane"], out=a["intensity"][:1])


# ---- flag_frames (plain torch: it runs on host tensors as it does on the device) ------------------------------------------
def test_flag_frames_follows_the_median_rule(lib):
    import torch
    rng = np.random.default_rng(5)
    v = rng.normal(100.0, 1.0, (3, 41))
    v[0, [4, 17]] = [130.0, 60.0]
    v[2, 40] = 107.0
    got = lib.flag_frames(torch.from_numpy(v)).numpy()
    assert got.dtype == bool and got.shape == v.shape
    assert np.array_equal(got, ref.flag(v)) and sorted(np.flatnonzero(got[0])) == [4, 17] and not got[1].any()
    assert got[2, 40] and got[2].sum() == 1
    assert np.array_equal(lib.flag_frames(torch.from_numpy(v), nsigma=2.0).numpy(), ref.flag(v, 2.0))
    even = torch.tensor([[1.0, 2.0, 3.0, 50.0]], dtype=torch.float64)      # lower median 2, MAD 1
    assert lib.flag_frames(even, 6.0).tolist() == [[False, False, False, True]]
    flat = torch.tensor([[5.0, 5.0, 5.0, 5.0, 5.0000001, 4.0]], dtype=torch.float64)   # MAD = 0: every v != median
    assert lib.flag_frames(flat).tolist() == [[False, False, False, False, True, True]]
    for bad in (torch.zeros(4), torch.zeros((2, 0)), torch.zeros((2, 3), dtype=torch.int32), np.zeros((2, 3))):
        with pytest.raises(ValueError, match="values must be"):
            lib.flag_frames(bad)
    for bad in (-1.0, float("nan"), "6", True):
        with pytest.raises(ValueError, match="nsigma"):
            lib.flag_frames(even, bad)


def test_planted_frames_stand_far_from_the_clean_ones():
    """The input of tests/test_hip_fit.py's flag test, on the restatement: three frames' data times 3."""
    g, data = ref.make_case("C", plant=False)
    data[0, [5, 64, 129]] *= 3
    cost = ref.frames_pixels(g, data)["frames"][..., 3]
    flagged = ref.flag(cost)
    assert sorted(np.flatnonzero(flagged[0])) == [5, 64, 129]
    med = np.median(cost)
    spread = 1.4826 * np.median(np.abs(cost - med))
    clean = np.delete(cost[0], [5, 64, 129])
    assert np.abs(clean - med).max() < 4 * spread                      # clean frames: inside 4 sigma
    assert np.abs(cost[0, [5, 64, 129]] - med).min() > 50 * spread     # planted frames: beyond 50 sigma


def test_fit_functions_are_exported_with_their_documented_signatures():
    import libtike.hipfft as pt
    import libtike.cufft as alias
    want = {"fit_frames": ["data", "farplane", "intensity", "mask", "ab", "pixels"],
            "accumulate_intensity": ["farplane", "out"], "flag_frames": ["values", "nsigma"]}
    for name, params in want.items():
        assert getattr(pt, name) is getattr(alias, name)
        assert list(inspect.signature(getattr(pt, name)).parameters) == params
    sig = inspect.signature(pt.fit_frames).parameters
    assert [sig[k].default for k in ("farplane", "intensity", "mask", "ab", "pixels")] == [None, None, None, None, True]
    assert inspect.signature(pt.flag_frames).parameters["nsigma"].default == 6.0
    assert inspect.signature(pt.accumulate_intensity).parameters["out"].default is None
    res = inspect.signature(pt.PtychoHIP.residuals).parameters
    assert list(res) == ["self", "data", "psi", "scan", "probe", "mask", "rescale"]
    assert res["mask"].default is None and res["rescale"].default is False
    assert pt.CGPtychoSolver.residuals is pt.PtychoHIP.residuals
