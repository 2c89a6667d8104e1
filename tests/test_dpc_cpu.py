"""First look, host side: the index logic of csrc/k_dpc.hpp built with the host compiler and walked as the kernels walk
it, the NumPy restatement of tests/dpc_ref.py run on the scenario of DESIGN.md section 18 with the float64 oracle forward,
and the argument checks of the C ABI and of ``libtike.hipfft.dpc``.  No GPU needed.

The bounds of the scenario (phase weighted relative rms <= 0.09, amplitude correlation >= 0.99, starting cost <= 0.25 of
the cost of ``psi = 1``) rest on the values measured for seed 3 with the float64 oracle: 0.043, 0.9990 and 0.039 (the
probe's own centre as reference) to 0.044 (the mean-frame reference), i.e. 2x to 6x margin; another seed moves the jitter
of the raster and with it these figures in the third digit.
"""
import ctypes
import inspect
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_build  # noqa: E402
import dpc_ref as ref  # noqa: E402
import gauge_ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libtike-cufft_amd", "csrc")


@pytest.fixture(scope="module")
def lib():
    import libtike.hipfft.dpc as lib
    return lib


@pytest.fixture(scope="module")
def nat():
    from libtike.hipfft import _native
    return _native


# ---- the index logic of csrc/k_dpc.hpp, built for the host --------------------------------------------------------------------
@pytest.fixture(scope="module")
def host(tmp_path_factory):
    program = host_build.build("host_dpc", tmp_path_factory.mktemp("dpc"))
    return lambda *args, stdin=None: program(*args, stdin=stdin).stdout


def test_host_sweep_is_clean(host):
    text = host()
    assert "host_dpc: 0 errors" in text and int(text.split()[3]) > 1000


@pytest.mark.parametrize("ptheta, nscan, ndet", [(1, 1, 1), (2, 33, 2), (1, 5, 15), (1, 1, 16), (2, 33, 18), (1, 130, 48),
                                                 (1, 600, 32), (1, 7, 128)])
def test_every_pixel_of_a_frame_is_visited_once_with_its_frequencies(host, nat, ptheta, nscan, ndet):
    errors, nwt, nranges, words, sky2, skx2, skykx = (int(v) for v in host("moments", ptheta, nscan, ndet).split())
    k = (np.fft.fftfreq(ndet) * ndet).round().astype(np.int64)          # stated without dpc_ref
    assert np.array_equal(ref.moment_k(ndet), k)
    assert errors == 0 and nwt == -(-ndet * ndet // 512)
    assert sky2 == skx2 == ndet * int((k * k).sum()) and skykx == int(k.sum()) ** 2
    assert nat.frame_moments_work_words(ptheta, nscan, ndet) == words == (ptheta * nscan * nwt * 8 if nwt > 1 else 0)


def map_case(rng, ptheta, nscan, nprb, nz, n):
    scan = (rng.uniform(0, 1, (ptheta, nscan, 2)) * np.array([nz - nprb + 6, n - nprb + 6])).astype(np.float32)
    scan[0, 0] = (nz - nprb + 0.5, n - nprb + 0.5)          # the +1 taps leave the object
    scan[0, 1 % nscan] = (-2.5, 3.0)
    scan[-1, 2 % nscan] = (np.nan, 4.0)
    scan[-1, 3 % nscan] = (7.0, 9.0)                         # a whole-pixel position
    keep = rng.uniform(size=(ptheta, nscan)) > 0.2
    return scan, keep


@pytest.mark.parametrize("ptheta, nscan, nprb, nz, n, nval", [(2, 9, 5, 37, 70, 1), (1, 130, 16, 37, 70, 4), (1, 300, 5, 64, 128, 2)])
def test_every_map_contribution_is_visited_once(host, ptheta, nscan, nprb, nz, n, nval):
    scan, keep = map_case(np.random.default_rng(7), ptheta, nscan, nprb, nz, n)
    text = "%d %d %d %d %d %d\n" % (ptheta, nscan, nprb, nz, n, nval)
    text += " ".join(str(int(v)) for v in scan.view(np.uint32).ravel()) + "\n" + " ".join(str(int(v)) for v in keep.ravel())
    errors, visits, skipped = (int(v) for v in host("map", stdin=text).split())
    valid = keep & np.array([[gauge_ref.split(p[0])[0] and gauge_ref.split(p[1])[0] for p in row] for row in scan])
    assert errors == 0 and skipped == (~valid).sum() and skipped >= 2
    want = 0                                                             # contributions that land inside the object
    for t, j in zip(*np.nonzero(valid)):
        sy, sx = gauge_ref.split(scan[t, j, 0])[1], gauge_ref.split(scan[t, j, 1])[1]
        for a in (0, 1):
            for b in (0, 1):
                want += max(0, min(nprb, nz - sy - a)) * max(0, min(nprb, n - sx - b))
    assert visits == want * nval


@pytest.mark.parametrize("nz, n", [(17, 130), (64, 64), (2, 2), (96, 112), (33, 257)])
def test_every_edge_gets_its_difference_once_from_each_end(host, nz, n):
    errors, tiles, visits = (int(v) for v in host("edges", nz, n).split())
    assert errors == 0 and tiles == -(-nz // 16) * -(-n // 64) and visits == 2 * (nz * (n - 1) + (nz - 1) * n)


# ---- the restatement on the scenario ----------------------------------------------------------------------------------------
_memo = {}


def probe_center(op, sc):
    """The documented recipe for the reference of a known probe: the centre of the pattern of the probe alone."""
    one = op.fwd(np.ones_like(sc["psi"]), np.array([[[8.0, 8.0]]], np.float32), sc["probe"], sc["ndet"], "double")
    return tuple(ref.centers(ref.frame_moments((np.abs(one) ** 2).astype(np.float32))[0])[0, 0])


def scenario_look(reference="probe"):
    """The scenario with data from the float64 oracle forward and the restatement's first looks, computed once."""
    if not _memo:
        from oracle import ptycho_oracle as op
        sc = ref.scenario()
        far = op.fwd(sc["psi"], sc["scan"], sc["probe"], sc["ndet"], "double")
        data = (np.abs(far) ** 2).astype(np.float32)
        args = (data, sc["scan"], sc["probe"], sc["nz"], sc["n"])
        _memo.update(sc=sc, data=data, op=op, mean=ref.first_look(*args),
                     probe=ref.first_look(*args, reference=probe_center(op, sc)))
    return _memo["sc"], _memo["data"], _memo[reference], _memo["op"]


def gaussian_cost(op, psi, sc, data):
    far = op.fwd(psi, sc["scan"], sc["probe"], sc["ndet"], "double")
    return float(((np.abs(far) - np.sqrt(data.astype(np.float64))) ** 2).sum())


def test_scenario_is_the_documented_one():
    sc = ref.scenario()
    assert sc["scan"].shape == (1, 864, 2) and sc["psi"].shape == (1, 96, 112) and sc["probe"].shape == (1, 16, 16)
    assert 7.6 < np.ptp(sc["phi"]) < 7.8


def test_zeroth_moment_is_the_exit_wave_power():
    sc, data, look, op = scenario_look("mean")
    near = op.nearplane(sc["psi"], sc["scan"], sc["probe"], sc["ndet"], "double")
    power = (np.abs(near) ** 2).sum(axis=(-2, -1))
    ndet = sc["ndet"]                                # nearplane carries c = 1 / ndet and the transform is unnormalised:
    assert np.allclose(look["moments"][..., 0], ndet * ndet * power, rtol=1e-6)      # sum I = sum |P psi|^2 exactly
    exit_wave = op.patches(sc["psi"], sc["scan"], sc["nprb"], "double") * sc["probe"][:, None]
    assert np.allclose(look["moments"][..., 0], (np.abs(exit_wave) ** 2).sum(axis=(-2, -1)), rtol=1e-6)


@pytest.mark.parametrize("reference", ["probe", "mean"])
def test_restatement_recovers_the_object_of_the_scenario(reference):
    """With the probe's own centre as the reference the phase is the truth as it stands (measured: 0.043); the mean-frame
    reference removes a ramp from it, which is gauge, so there the ramp of the difference is taken out first."""
    sc, data, look, op = scenario_look(reference)
    lit = look["illumination"][0] > 0.05 * look["illumination"][0].max()
    w = np.where(lit, look["illumination"][0], 0)
    assert np.array_equal(lit, look["lit"][0]) and look["converged"][0]
    rms = ref.weighted_rms_error(look["phase"][0], sc["phi"], w, ramp=reference == "mean")
    corr = ref.weighted_correlation(look["phase"][0], sc["phi"], w)
    acorr = ref.weighted_correlation(np.sqrt(np.maximum(look["transmission"][0], 0)), sc["amp"], w)
    print("first look, restatement, reference %s: phase rms %.4f, phase correlation %.5f, amplitude correlation %.5f, "
          "%d iterations" % (reference, rms, corr, acorr, look["iterations"][0]))
    assert rms <= 0.09 and acorr >= 0.99
    assert corr >= (0.99 if reference == "probe" else 0.95)


@pytest.mark.parametrize("reference", ["probe", "mean"])
def test_restatement_object_starts_at_a_quarter_of_the_cost(reference):
    sc, data, look, op = scenario_look(reference)
    flat = gaussian_cost(op, np.ones_like(sc["psi"]), sc, data)
    start = gaussian_cost(op, ref.initial_object(look), sc, data)
    print("first look, restatement, reference %s: cost %.1f from psi = 1, %.1f from the data (ratio %.4f)"
          % (reference, flat, start, start / flat))
    assert start <= 0.25 * flat


def test_restatement_pieces():
    rng = np.random.default_rng(1)
    # a mask drops what lies under it, NaN included; NaN at a measured pixel stays in its frame
    data = rng.uniform(0, 5, (1, 3, 6, 6)).astype(np.float32)
    mask = rng.uniform(size=(6, 6)) > 0.3
    dirty = data.copy()
    dirty[:, :, ~mask] = np.nan
    a, bound = ref.frame_moments(data, mask, 1.5)
    b, _ = ref.frame_moments(dirty, mask, 1.5)
    assert np.array_equal(a, b) and (bound >= 0).all() and (a[..., 7] == 0).all()
    assert np.allclose(a[..., 6], (data * (mask & (ref.moment_k(6)[:, None] ** 2 + ref.moment_k(6)[None] ** 2 > 2.25))).sum((-2, -1)))
    dirty[0, 1][np.nonzero(mask)[0][0], np.nonzero(mask)[1][0]] = np.nan
    c, _ = ref.frame_moments(dirty, mask)
    assert np.isnan(c[0, 1, 0]) and np.isfinite(c[0, [0, 2]]).all()
    # a constant goes through the map unchanged; keep equals the call on the subset
    probe = gauge_ref.random_probe(rng, 1, 2, 5)
    scan = (rng.uniform(0, 1, (1, 40, 2)) * np.array([30, 60])).astype(np.float32)
    keep = rng.uniform(size=(1, 40)) > 0.3
    vals = rng.normal(size=(1, 40, 2)).astype(np.float32)
    vals[..., 1] = 2.5
    w, out, _ = ref.scan_map(vals, scan, probe, 37, 70, keep)
    w2, out2, _ = ref.scan_map(vals[:, keep[0]], scan[:, keep[0]], probe, 37, 70)
    assert np.array_equal(w, w2) and np.array_equal(out, out2)
    assert np.array_equal(w, gauge_ref.illumination(scan[:, keep[0]], probe, 37, 70, np.float32))
    assert np.abs(out[0, 1][w[0] > 0] - 2.5).max() <= 2.5e-6 and (out[0, :, w[0] == 0] == 0).all()
    # the analytic gradient of a quadratic is exact under the trapezoid rule: the surface comes back
    y, x = np.meshgrid(np.arange(17.0), np.arange(30.0), indexing="ij")
    s = (0.01 * x * x - 0.2 * x + 1) * (0.05 * y - 0.3)
    gy, gx = (0.01 * x * x - 0.2 * x + 1) * 0.05, (0.02 * x - 0.2) * (0.05 * y - 0.3)
    got = ref.integrate(gy.astype(np.float32), gx.astype(np.float32), tol=1e-10)
    assert got["converged"] and np.abs(got["phase"] - (s - s.mean())).max() < 1e-5


# ---- argument checks --------------------------------------------------------------------------------------------------------
NAMES = {"ptycho_frame_moments_work_words": "size_t", "ptycho_frame_moments": "int", "ptycho_scan_map": "int",
         "ptycho_integrate_begin": "int", "ptycho_integrate_finish": "int"}


def test_dpc_symbols_are_declared_and_exported(nat):
    text = open(os.path.join(ROOT, "include", "ptycho_hip.h")).read()
    for name, res in NAMES.items():
        assert "%s %s(" % (res, name) in text
        assert name in nat.SYMBOLS and hasattr(nat.lib, name)
    make = open(os.path.join(CSRC, "Makefile")).read()
    assert "k_dpc.hpp" in make and "host_dpc.hpp" in make and "host_dpc:" in make


def test_dpc_abi_rejects_bad_arguments_without_a_gpu(nat):
    d = ctypes.c_void_p(0x1000)              # never dereferenced: every rejection comes before any HIP call

    def rejects(fn, ok, over, word):
        assert fn(*{**ok, **over}.values(), None) == 1, over
        assert word in nat.last_error(), (over, nat.last_error())

    ok = dict(moments=d, data=d, mask=None, darkfield=-1.0, ptheta=1, nscan=4, ndet=16, work=d)
    for name in ("moments", "data", "work"):
        rejects(nat.frame_moments, ok, {name: None}, b"null")
    for name in ("ptheta", "nscan", "ndet"):
        rejects(nat.frame_moments, ok, {name: 0}, b"positive")
    rejects(nat.frame_moments, ok, dict(ptheta=65536), b"ptheta")
    rejects(nat.frame_moments, ok, dict(ndet=46341), b"too large")
    rejects(nat.frame_moments, ok, dict(nscan=2 ** 31), b"too large")
    for bad in (float("nan"), float("inf")):
        rejects(nat.frame_moments, ok, dict(darkfield=bad), b"darkfield")
    assert nat.frame_moments_work_words(0, 4, 16) == 0 and nat.frame_moments_work_words(1, 4, 46341) == 0
    assert nat.frame_moments_work_words(1, 4096, 256) == 4096 * 128 * 8 and nat.frame_moments_work_words(1, 4, 16) == 0

    ok = dict(weight=d, out=d, values=d, keep=None, scan=d, probe=d, ptheta=1, nscan=4, nval=4, nmodes=1, nprb=8, nz=32,
              n=32, raw=0, work=None)
    for name in ("weight", "out", "values", "scan", "probe"):
        rejects(nat.scan_map, ok, {name: None}, b"null")
    rejects(nat.scan_map, ok, dict(keep=d), b"work")
    for name in ("ptheta", "nscan", "nprb", "nz", "n"):
        rejects(nat.scan_map, ok, {name: 0}, b"positive")
    for bad in (0, 5, -1):
        rejects(nat.scan_map, ok, dict(nval=bad), b"nval")
    rejects(nat.scan_map, ok, dict(nmodes=0), b"nmodes")
    rejects(nat.scan_map, ok, dict(ptheta=65536), b"ptheta")
    for over in (dict(nz=2 ** 30 + 1), dict(n=2 ** 30 + 1), dict(nz=16 * 65535 + 1), dict(nscan=2 ** 31)):
        rejects(nat.scan_map, ok, over, b"too large")

    begin = dict(buf=d, state=d, gy=d, gx=d, weight=None, ptheta=1, nz=8, n=8, work=d)
    finish = dict(out=d, state=d, buf=d, weight=None, ptheta=1, nz=8, n=8, work=d)
    for fn, ok, required in ((nat.integrate_begin, begin, ("buf", "state", "gy", "gx", "work")),
                             (nat.integrate_finish, finish, ("out", "state", "buf", "work"))):
        for name in required:
            rejects(fn, ok, {name: None}, b"null")
        for over in (dict(nz=1), dict(n=1), dict(nz=0)):
            rejects(fn, ok, over, b"at least 2")
        rejects(fn, ok, dict(nz=2 ** 16, n=2 ** 15), b"2^31")
        for bad in (0, 65536):
            rejects(fn, ok, dict(ptheta=bad), b"ptheta")


def arrays(**over):
    a = {"data": np.zeros((2, 6, 8, 8), np.float32), "scan": np.zeros((2, 6, 2), np.float32),
         "probe": np.zeros((2, 1, 4, 4), np.complex64), "nz": 20, "n": 24}
    a.update(over)
    return a


@pytest.mark.parametrize("over, exc, match", [
    ({"data": np.zeros((2, 6, 8, 8), np.float64)}, TypeError, "data must be float32"),
    ({"data": np.zeros((2, 6, 8, 9), np.float32)}, ValueError, r"data must be \[ptheta, nscan, ndet, ndet\]"),
    ({"data": np.zeros((6, 8, 8), np.float32)}, ValueError, "data must have 4"),
    ({"mask": np.ones((8, 9), bool)}, ValueError, "mask must be"),
    ({"mask": 1}, TypeError, "mask must be an array"),
    ({"darkfield": -1.0}, ValueError, "darkfield must be"),
    ({"darkfield": float("nan")}, ValueError, "darkfield must be"),
    ({"darkfield": "wide"}, ValueError, "darkfield must be"),
    ({"scan": np.zeros((2, 6, 3), np.float32)}, ValueError, "scan must be"),
    ({"scan": np.zeros((2, 7, 2), np.float32)}, ValueError, "values must be|differ"),
    ({"probe": np.zeros((3, 1, 4, 4), np.complex64)}, ValueError, "differ in ptheta"),
    ({"probe": np.zeros((2, 1, 4, 5), np.complex64)}, ValueError, "probe must be square"),
    ({"nz": 0}, ValueError, "nz must be a positive integer"),
    ({"nz": 1}, ValueError, "nz >= 2"),
    ({"keep": np.ones((2, 5), bool)}, ValueError, "keep must be"),
    ({"keep": np.ones((2, 6), np.float32)}, TypeError, "keep must be bool or uint8"),
    ({"reference": "median"}, ValueError, "reference must be"),
    ({"reference": (1.0, 2.0, 3.0)}, ValueError, "reference must be"),
    ({"reference": (np.nan, 0.0)}, ValueError, "reference must be"),
    ({"floor": 1.5}, ValueError, "floor must be"),
    ({"floor": True}, ValueError, "floor must be"),
    ({"tol": -1.0}, ValueError, "tol must be"),
    ({"maxiter": 2.5}, ValueError, "maxiter must be"),
])
def test_first_look_refuses_bad_arguments_before_device_use(lib, over, exc, match):
    import torch
    a = arrays(**over)
    as_torch = {k: torch.from_numpy(v) if isinstance(v, np.ndarray) else v for k, v in a.items()}
    for v in (a, as_torch):
        with pytest.raises(exc, match=match):
            lib.check_first_look(**v)
        with pytest.raises(exc, match=match):                             # the public function checks first
            lib.first_look(**v)


@pytest.mark.parametrize("fn, args, exc, match", [
    ("frame_moments", (np.zeros((1, 2, 4, 4), np.int32),), TypeError, "data must be float32"),
    ("scan_map", (np.zeros((1, 3, 5), np.float32), np.zeros((1, 3, 2), np.float32), np.zeros((1, 4, 4), np.complex64), 9, 9),
     None, None),
    ("scan_map", (np.zeros((1, 4), np.float32), np.zeros((1, 3, 2), np.float32), np.zeros((1, 4, 4), np.complex64), 9, 9),
     ValueError, "values must be"),
    ("scan_map", (np.zeros((1, 3), np.float64), np.zeros((1, 3, 2), np.float32), np.zeros((1, 4, 4), np.complex64), 9, 9),
     TypeError, "values must be float32"),
    ("integrate_gradient", (np.zeros((4, 5), np.float32), np.zeros((4, 6), np.float32)), ValueError, "gx must have gy's shape"),
    ("integrate_gradient", (np.zeros((4, 5), np.float64), np.zeros((4, 5), np.float64)), TypeError, "gy must be float32"),
    ("integrate_gradient", (np.zeros((1, 5), np.float32), np.zeros((1, 5), np.float32)), ValueError, "nz >= 2"),
    ("integrate_gradient", (np.zeros((4, 5), np.float32), np.zeros((4, 5), np.float32), np.ones((4, 4), np.float32)), ValueError,
     "weight must have"),
    ("initial_object", ({"phase": 1},), ValueError, "look must be"),
])
def test_the_pieces_refuse_bad_arguments_before_device_use(lib, fn, args, exc, match):
    checker = {"frame_moments": lib.check_frame_moments, "scan_map": lib.check_scan_map,
               "integrate_gradient": lib.check_integrate}.get(fn)
    if exc is None:                                                       # five channels are fine: Python splits them
        assert checker(*args) == (1, 3, 5, 1, 4, 9, 9)
        return
    for call in filter(None, (checker, getattr(lib, fn))):
        with pytest.raises(exc, match=match):
            call(*args)


def test_dpc_functions_are_exported_with_their_documented_signatures(lib):
    import libtike.hipfft as pt
    for name in ("frame_moments", "scan_map", "integrate_gradient", "first_look", "initial_object"):
        assert getattr(pt, name) is getattr(lib, name) and name in lib.__all__
    sig = inspect.signature(pt.first_look).parameters
    assert list(sig) == ["data", "scan", "probe", "nz", "n", "mask", "reference", "keep", "floor", "darkfield", "tol", "maxiter"]
    assert [sig[k].default for k in list(sig)[5:]] == [None, "mean", None, 0.05, None, 1e-4, None]
    assert inspect.signature(lib.check_first_look) == inspect.signature(pt.first_look)
    assert list(inspect.signature(pt.frame_moments).parameters) == ["data", "mask", "darkfield"]
    sig = inspect.signature(pt.scan_map).parameters
    assert list(sig) == ["values", "scan", "probe", "nz", "n", "keep", "normalize"] and sig["normalize"].default is True
    sig = inspect.signature(pt.integrate_gradient).parameters
    assert list(sig) == ["gy", "gx", "weight", "tol", "maxiter", "check_every", "out"]
    assert [sig[k].default for k in list(sig)[2:]] == [None, 1e-4, None, 256, None]
    assert list(inspect.signature(pt.initial_object).parameters) == ["look", "amplitude"]
