"""Frame preparation, host side: the NumPy restatement of tests/prepare_ref.py held to its identities, the partition and
the crop / shift index map of csrc/k_prepare.hpp built with the host compiler and walked as the kernels walk them, and
the argument checks of the C ABI and of ``libtike.hipfft.prepare``.  No GPU needed."""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_build  # noqa: E402
import prepare_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libtike-cufft_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    import libtike.hipfft.prepare as lib
    return lib


@pytest.fixture(scope="module")
def nat():
    from libtike.hipfft import _native
    return _native


_cases = {}


def case(name):
    if name not in _cases:
        raw, kw = ref.make_case(name)
        _cases[name] = (raw, kw, ref.prepare(raw, **kw))
    return _cases[name]


# ---- the restatement --------------------------------------------------------------------------------------------------
def test_defaults_are_the_ifftshift_of_the_float32_frames():
    raw, kw, out = case("A")
    assert kw == {"ndet": 16}
    assert np.array_equal(out["data"][0], np.fft.ifftshift(raw.astype(np.float32), axes=(-2, -1)))
    assert out["mask"].all() and out["data"].dtype == np.float32 and out["mask"].dtype == np.uint8
    assert out["data"][0, 0, 0, 0] == raw[0, 8, 8]                       # centred pixel ndet // 2 lands at [0, 0]


def test_restatement_equals_the_host_chain_of_io_bitwise():
    """Even ndet, bin 1, a probe of maximum modulus 2: ``from_record`` + ``solver_inputs`` divide by 4."""
    from libtike.hipfft.io import PtychoDataset, solver_inputs
    rng = np.random.default_rng(3)
    raw = rng.integers(0, 65536, (6, 32, 32), dtype=np.uint16)
    probe = np.zeros((1, 8, 8), np.complex64)
    probe[0, 3, 4] = 2j
    pos = np.stack([np.arange(6), np.arange(6)[::-1]], 1).astype(np.float32)
    rec = {"data": raw, "positions_0": pos, "positions_1": pos, "initprobe": probe, "recprobe": probe,
           "detector_pixel_size": 1.0, "detector_distance": 1.0, "incident_wavelength": 8e10, "rotation_angle": 0.0}
    ds = PtychoDataset.from_record(rec, view_dims=(64, 64))
    host = solver_inputs(ds, (64, 64))["data"]
    assert host.shape == (1, 6, 32, 32)                                  # every position kept, in order
    mine = ref.prepare(raw, 32, scale=0.25)["data"]
    assert np.array_equal(mine.view(np.uint32), host.view(np.uint32))


def test_binning_keeps_the_frame_sums():
    rng = np.random.default_rng(4)
    raw = rng.integers(0, 4000, (3, 32, 32), dtype=np.uint16)            # integer sums below 2^24: exact in float32
    one, two = ref.prepare(raw, 32), ref.prepare(raw, 16, bin=2)
    assert np.array_equal(one["frames"][..., 0], two["frames"][..., 0])
    assert np.array_equal(two["centred"], raw.astype(np.float32).reshape(1, 3, 16, 2, 16, 2).sum((3, 5)))
    four = ref.prepare(raw, 8, bin=4)
    assert np.array_equal(one["frames"][..., 0], four["frames"][..., 0])


@pytest.mark.parametrize("name", ["C", "E", "H"])
def test_unmeasured_pixels_are_zero_whatever_they_hold(name):
    raw, kw, out = case(name)
    off = out["mask"] == 0
    assert off.any() and not off.all()
    assert (out["data"][..., off] == 0).all() and (out["pixels"][..., off] == 0).all()
    assert np.isfinite(out["data"]).all() and np.isfinite(out["frames"]).all()
    if name == "C":                                                    # other garbage under the bad pixels: the same bits
        raw2, dark2, gain2 = raw.copy(), kw["dark"].copy(), kw["gain"].copy()
        ys, xs = np.nonzero(kw["bad"])
        raw2[:, ys, xs], dark2[ys, xs], gain2[ys, xs] = 1e30, np.inf, np.nan
        again = ref.prepare(raw2, **{**kw, "dark": dark2, "gain": gain2})
        for key in ("data", "frames", "pixels"):
            assert np.array_equal(again[key], out[key])


@pytest.mark.parametrize("name", list(ref.CASES))
def test_frame_and_pixel_sums_agree_when_totalled(name):
    raw, kw, out = case(name)
    f, p = out["frames"], out["pixels"]
    ptheta, nscan, ndet = ref.CASES[name]
    assert out["data"].shape == (ptheta, nscan, ndet, ndet) and f.shape == (ptheta, nscan, 4) and p.shape == (ptheta, 4, ndet, ndet)
    for col in (0, 1):
        assert np.allclose(p[:, col].sum((-2, -1)), f[..., col].sum(1), rtol=1e-12, atol=0)
    assert np.array_equal(f[..., 0], out["data"].astype(np.float64).sum((-2, -1)))
    assert (np.abs(f[..., :2]) <= out["frames_mag"]).all() and (np.abs(p[:, :2]) <= out["pixels_mag"]).all()
    assert f[..., 2].max() == p[:, 2].max() == out["data"].max()      # the largest value, whichever way it is found
    assert p[:, 3].sum() <= f[..., 3].sum()                              # frames per pixel against raw pixels per frame


def test_the_cases_exercise_what_they_are_named_for():
    raw, kw, out = case("B")
    assert raw.dtype == np.int32 and raw.shape[-2] != raw.shape[-1] and (raw < 0).any()
    idx = kw["index"]
    assert idx[0, 0] == idx[0, 1] and ((idx < 0) | (idx >= raw.shape[1])).sum() == 2
    assert np.array_equal(out["data"][0, 0], out["data"][0, 1]) and out["data"][0, 1].any()
    for t, j in ((0, 2), (1, 1)):
        assert not out["data"][t, j].any() and not out["frames"][t, j].any()
    raw, kw, out = case("C")
    plain = ref.prepare(raw, **{**kw, "clip": False})
    assert (plain["data"] < 0).any() and (out["data"] >= 0).all() and not np.array_equal(plain["data"], out["data"])
    assert np.isnan(raw).any() and np.isinf(raw).any() and np.isnan(kw["dark"]).any() and np.isinf(kw["gain"]).any()
    assert 0 < (out["mask"] == 0).sum() <= 5
    raw, kw, out = case("D")
    assert raw.dtype == np.uint32 and (raw.astype(np.float32).astype(np.float64) != raw).any()   # the conversion rounds
    fft = np.fft.fftshift(out["centred"], axes=(-2, -1))
    assert not np.array_equal(fft, out["data"]) and out["data"][0, 0, 0, 0] == np.float32(2 ** 32 - 1)
    raw, kw, out = case("E")
    y0, x0 = ref.window_origin(raw.shape, kw["ndet"], kw["center"], kw["bin"])
    assert y0 < 0 and x0 + kw["ndet"] * kw["bin"] > raw.shape[-1] and y0 + kw["ndet"] * kw["bin"] <= raw.shape[-2]
    assert out["frames"][0, :, 3].tolist() == [2, 0, 1] and (raw >= 60000).sum() == 5 and out["pixels"][0, 3].sum() == 2   # two in one bin
    assert out["measured"][:11].sum() == 0 and out["measured"][11:, :18].all() and not out["measured"][:, 18:].any()
    raw, kw, out = case("F")
    assert ref.window_origin(raw.shape, 64, kw["center"])[1] % 2 == 1 and raw.shape[-1] % 4 and out["mask"].all()
    raw, kw, out = case("G")
    assert ref.window_origin(raw.shape, 24, kw["center"], 4) == (-8, -4) and not out["measured"][:2].any()
    assert out["measured"][2:18, 1:17].all() and out["measured"].sum() == 256 and out["frames"][..., 3].sum() > 0
    raw, kw, out = case("H")
    assert (out["data"] < 0).any() and out["frames"][..., 3].sum() > 0 and (out["mask"] == 0).sum() == 2


# ---- the partition and the index map of csrc/k_prepare.hpp, built for the host ---------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    program = host_build.build("host_prepare", tmp_path_factory.mktemp("prepare"))
    return lambda *args: program(*args).stdout


WALK_SHAPES = list(ref.CASES.values()) + [(1, 4096, 256), (1, 1, 1), (3, 5, 2), (1, 129, 3), (2, 1000, 33), (1, 257, 45),
                                          (7, 300, 32), (1, 40_000, 3)]


@pytest.mark.parametrize("shape", WALK_SHAPES, ids=lambda s: "%dx%dx%d" % s)
def test_host_walk_visits_every_pair_and_every_word_once(host, nat, shape):
    errors, words, nranges, nwt = (int(v) for v in host("walk", *shape).split())
    npix = shape[2] ** 2
    assert errors == 0
    assert words == nat.prepare_work_words(shape[0], shape[1], npix)    # the library plans as the host build does
    assert nwt == -(-npix // 256) and 1 <= nranges <= max(1, -(-shape[1] // 128))
    assert words == (shape[0] * shape[1] * nwt * 4 if nwt > 1 else 0) + (shape[0] * nranges * 4 * npix if nranges > 1 else 0)


def test_the_cases_reach_the_plans_they_are_named_for(host):
    plan = {k: [int(x) for x in host("walk", *v).split()][2:] for k, v in ref.CASES.items()}
    assert plan["A"] == [1, 1]                                           # exactly one wave tile, one range: no fold
    assert plan["B"] == [1, 3] and 24 * 24 % 256 != 0                    # three wave tiles, the last one partial
    assert plan["C"][1] == 1 and plan["C"][0] == 3 and 290 % -(-290 // 3) != 0   # three ranges, the last one shorter
    assert plan["D"] == [1, 1] and 15 * 15 < 256                         # a partial wave tile
    assert plan["E"] == [1, 4] and plan["F"] == [1, 16]                  # one and four workgroups of four waves
    assert [int(x) for x in host("walk", 1, 4096, 256).split()][2:] == [32, 256]   # the flagship: 64 x 32 workgroups
    assert "host_prepare: 0 errors" in host()                            # the program's own list of shapes


def numpy_map(ndet, bin, H, W, y0, x0):
    oy, ox = np.meshgrid(np.arange(ndet), np.arange(ndet), indexing="ij")
    oy, ox = np.fft.ifftshift(oy), np.fft.ifftshift(ox)                  # data[r][c] holds centred pixel (oy, ox)[r][c]
    rows = []
    for by, bx in ((0, 0), (bin - 1, bin - 1)):
        y, x = y0 + oy * bin + by, x0 + ox * bin + bx
        rows.append(np.where((y >= 0) & (y < H) & (x >= 0) & (x < W), y * W + x, -1))
    return np.stack([oy, ox] + rows, -1).reshape(-1, 4)


MAP_GEOMS = []
for _name in ref.CASES:
    _raw, _kw = ref.make_case(_name)
    MAP_GEOMS.append((_kw["ndet"], _kw.get("bin", 1)) + _raw.shape[-2:]
                     + ref.window_origin(_raw.shape, _kw["ndet"], _kw.get("center"), _kw.get("bin", 1)))
MAP_GEOMS += [(1, 1, 5, 7, 2, 3), (2, 4, 5, 7, 2, 3), (3, 2, 9, 9, 8, -1), (2, 1, 4, 4, -1, -1), (3, 1, 3, 3, 0, 0),
              (1, 4, 2, 2, 0, 0), (256, 2, 512, 512, 0, 0)]


@pytest.mark.parametrize("geom", MAP_GEOMS, ids=lambda g: "n%d-b%d-%dx%d-%d-%d" % g)
def test_crop_and_shift_index_map_is_numpys(host, geom):
    got = np.array([[int(v) for v in line.split()] for line in host("map", *geom).splitlines()])
    ndet, bin, H, W, y0, x0 = geom
    assert np.array_equal(got[:, :4], numpy_map(*geom))
    aligned = ndet % 8 == 0 and W % 4 == 0 and x0 % 4 == 0
    assert (got[:, 4] == int(aligned)).all()


def test_the_cases_cover_both_load_paths(host):
    aligned = {}
    for name, geom in zip(ref.CASES, MAP_GEOMS):
        aligned[name] = int(host("map", *geom).split()[4])
    assert aligned == {"A": 1, "B": 0, "C": 1, "D": 0, "E": 0, "F": 0, "G": 1, "H": 1}


# ---- argument checks --------------------------------------------------------------------------------------------------
def test_prepare_symbols_are_declared_and_exported(nat):
    text = open(os.path.join(ROOT, "include", "ptycho_hip.h")).read()
    for name, res in (("ptycho_prepare_work_words", "size_t"), ("ptycho_prepare_frames", "int")):
        assert "%s %s(" % (res, name) in text
        assert name in nat.SYMBOLS and hasattr(nat.lib, name)
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_prepare.hpp" in make and "host_prepare.hpp" in make and "host_prepare:" in make


def test_prepare_abi_rejects_bad_arguments_without_a_gpu(nat):
    d = ctypes.c_void_p(0x1000)              # never dereferenced: every rejection comes before any HIP call
    ok = dict(data=d, mask=d, frames=d, pixels=None, raw=d, dtype=0, index=None, dark=None, gain=None, bad=None, ptheta=1,
              nraw=4, nscan=4, H=32, W=32, y0=0, x0=0, bin=1, ndet=16, saturation=float("nan"), scale=1.0, clip=1, work=d)
    call = lambda **over: nat.prepare_frames(*{**ok, **over}.values(), None)   # noqa: E731
    for name in ("data", "mask", "frames", "raw", "work"):
        assert call(**{name: None}) == 1
        assert b"null" in nat.last_error()
    for name in ("ptheta", "nraw", "nscan", "H", "W", "ndet"):
        assert call(**{name: 0}) == 1
        assert b"positive" in nat.last_error()
    for bad in (0, 3, 8, -1):
        assert call(bin=bad) == 1
        assert b"bin" in nat.last_error()
    for bad in (-1, 4, 100):
        assert call(dtype=bad) == 1
        assert b"dtype" in nat.last_error()
    assert call(ptheta=65536, index=d) == 1
    assert b"ptheta" in nat.last_error()
    assert call(nraw=5) == 1                                           # no index: frame j is raw frame j
    assert b"nraw" in nat.last_error()
    for over in (dict(nscan=2 ** 31, index=d), dict(nraw=2 ** 31, index=d), dict(ndet=32769), dict(H=2 ** 16, W=2 ** 15),
                 dict(ptheta=65535, nscan=2 ** 30, nraw=2 ** 30, ndet=32768), dict(y0=2 ** 30 + 1), dict(x0=-2 ** 30 - 1),
                 dict(ptheta=65535, nraw=2 ** 30, nscan=1, index=d, H=2 ** 15, W=2 ** 15)):
        assert call(**over) == 1
        assert b"too large" in nat.last_error()
    for sizes in ((0, 4, 256), (1, 0, 256), (1, 4, 0), (65536, 4, 256), (1, 2 ** 31, 4), (1, 4, 2 ** 30 + 1),
                  (65535, 2 ** 30, 2 ** 30)):
        assert nat.prepare_work_words(*sizes) == 0
    assert nat.prepare_work_words(1, 4, 256) == 0                       # one wave tile, one range: nothing to fold
    assert nat.prepare_work_words(1, 4096, 65536) == 4096 * 256 * 4 + 32 * 4 * 65536


def arrays(**over):
    a = {"raw": np.zeros((2, 5, 20, 24), np.uint16), "ndet": 8, "center": None, "bin": 2, "dark": np.zeros((20, 24), np.float32),
         "gain": np.ones((20, 24), np.float32), "bad": np.zeros((20, 24), np.uint8), "index": np.zeros((2, 3), np.int64),
         "saturation": 60000, "scale": 1.0, "out": None}
    a.update(over)
    return a


def test_checker_accepts_the_documented_shapes(lib):
    import torch
    a = arrays()
    assert lib.check_prepare(**a) == (2, 5, 3, 20, 24, 10 - 8, 12 - 8)
    assert lib.check_prepare(a["raw"][0], 9, center=(3, 30), bin=4) == (1, 5, 5, 20, 24, 3 - 16, 30 - 16)
    assert lib.check_prepare(a["raw"][0], 8, index=np.zeros(7, np.int64), bad=np.zeros((20, 24), bool))[:3] == (1, 5, 7)
    for dt in (np.uint16, np.uint32, np.int32, np.float32):
        assert lib.check_prepare(np.zeros((3, 4, 4), dt), 1)[:3] == (1, 3, 3)
    t = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in a.items()}
    t["out"] = torch.zeros((2, 3, 8, 8))
    assert lib.check_prepare(**t) == (2, 5, 3, 20, 24, 2, 4)


@pytest.mark.parametrize("over, exc, match", [
    ({"raw": [[0]]}, TypeError, "raw must be an array"),
    ({"raw": np.zeros((2, 5, 20, 24), np.float64)}, TypeError, "raw must be uint16, uint32, int32 or float32, got float64"),
    ({"raw": np.zeros((2, 5, 20, 24), np.int16)}, TypeError, "got int16"),
    ({"raw": np.zeros((20, 24), np.uint16)}, ValueError, r"raw must be \[nraw, H, W\] or .*\(20, 24\)"),
    ({"raw": np.zeros((2, 0, 20, 24), np.uint16)}, ValueError, "non-empty"),
    ({"raw": np.zeros((2, 5, 20, 48), np.uint16)[..., ::2]}, ValueError, "raw must be contiguous"),
    ({"ndet": 0}, ValueError, "ndet must be an integer"),
    ({"ndet": 8.0}, ValueError, "ndet must be an integer"),
    ({"ndet": 32769}, ValueError, "ndet must be an integer"),
    ({"bin": 3}, ValueError, "bin must be 1, 2 or 4, got 3"),
    ({"bin": True}, ValueError, "bin must be 1, 2 or 4"),
    ({"center": (1.5, 2)}, ValueError, "center must be two integers"),
    ({"center": 7}, ValueError, "center must be two integers"),
    ({"dark": np.zeros((20, 24), np.float64)}, TypeError, "dark must be float32"),
    ({"dark": np.zeros((24, 20), np.float32)}, ValueError, r"dark must be \(20, 24\)"),
    ({"gain": np.ones((1, 20, 24), np.float32)}, ValueError, r"gain must be \(20, 24\)"),
    ({"bad": [[0]]}, TypeError, "bad must be an array"),
    ({"bad": np.zeros((20, 23), np.uint8)}, ValueError, r"bad must be \(20, 24\)"),
    ({"index": np.zeros((2, 3), np.int32)}, TypeError, "index must be int64"),
    ({"index": np.zeros(3, np.int64)}, ValueError, r"index must be \[2, nscan\]"),
    ({"index": np.zeros((1, 3), np.int64)}, ValueError, r"index must be \[2, nscan\]"),
    ({"saturation": "high"}, ValueError, "saturation must be a number"),
    ({"scale": None}, ValueError, "scale must be a number"),
    ({"out": np.zeros((2, 3, 8, 8), np.float64)}, TypeError, "out must be float32"),
    ({"out": np.zeros((2, 5, 8, 8), np.float32)}, ValueError, r"out must be \(2, 3, 8, 8\)"),
])
def test_bad_arguments_raise_before_device_use(lib, over, exc, match):
    import torch
    import libtike.hipfft as pt
    a = arrays(**over)
    as_torch = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) and v.flags["C_CONTIGUOUS"] else v for k, v in a.items()}
    for v in (a, as_torch):
        with pytest.raises(exc, match=match):
            lib.check_prepare(**v)
        with pytest.raises(exc, match=match):                         # the public function checks first
            pt.prepare_frames(**v)


def test_host_tensors_and_bad_probe_arguments_are_refused(lib):
    import torch
    with pytest.raises(ValueError, match="device tensor or a NumPy array"):
        lib.prepare_frames(torch.zeros((2, 8, 8), dtype=torch.float32), 4)
    for args, exc, match in ((([[1.0]], 1), TypeError, "pattern must be an array"),
                             ((np.zeros((8, 8)), 4), ValueError, "pattern must be"),
                             ((np.zeros((1, 8, 6)), 4), ValueError, "pattern must be"),
                             ((np.zeros((1, 8, 8), np.complex64), 4), TypeError, "pattern must be real"),
                             ((np.zeros((1, 8, 8)), 9), ValueError, "nprb must be"),
                             ((np.zeros((1, 8, 8)), 0), ValueError, "nprb must be"),
                             ((np.zeros((1, 8, 8)), 4, -1.0), ValueError, "power must be")):
        with pytest.raises(exc, match=match):
            lib.initial_probe(*args)


def test_prepare_functions_are_exported_with_their_documented_signatures():
    import libtike.hipfft as pt
    import libtike.cufft as alias
    want = {"prepare_frames": ["raw", "ndet", "center", "bin", "dark", "gain", "bad", "index", "saturation", "scale", "clip",
                               "pixels", "out"],
            "initial_probe": ["pattern", "nprb", "power"]}
    for name, params in want.items():
        assert getattr(pt, name) is getattr(alias, name)
        assert list(inspect.signature(getattr(pt, name)).parameters) == params
    sig = inspect.signature(pt.prepare_frames).parameters
    assert [sig[k].default for k in list(sig)[2:]] == [None, 1, None, None, None, None, None, 1.0, True, True, None]
    assert inspect.signature(pt.initial_probe).parameters["power"].default is None
