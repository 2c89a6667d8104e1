"""Measured-pixel mask of the CG reconstruction, host side: the NumPy reference with a mask (tests/cg_reference.py), the C ABI's
argument checks, the solver signature and the I/O adapters.  No GPU needed."""
import inspect
import os
import sys
import warnings

import numpy as np
import pytest

from libtike.hipfft import io
from libtike.hipfft import synthetic as syn
from oracle import cg_oracle as cg

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from cg_reference import ReferenceSolver, detector_mask, random_mask  # noqa: E402


def problem(nmodes, ndet=16, seed=3):
    p = syn.make_problem(4, 4, 4, ndet, ndet, seed=seed)
    probe = syn.hermite_modes(ndet, nmodes) if nmodes > 1 else p["probe"][:, None].copy()
    rng = np.random.default_rng(seed + 100)
    probe = (probe * np.exp(2j * np.pi * rng.random(probe.shape[-2:]))).astype(np.complex64)
    ora = cg.OracleSolver(p["nscan"], ndet, ndet, 1, p["nz"], p["n"])
    data = np.zeros((1, p["nscan"], ndet, ndet), np.float32)
    for k in range(nmodes):
        data += np.abs(ora.fwd(p["psi"], p["scan"], probe[:, k])) ** 2
    return p, probe, data


def run(cls, p, probe, data, mask=None, piter=5, recover=True):
    ndet = data.shape[-1]
    slv = cls(p["nscan"], ndet, ndet, 1, p["nz"], p["n"])
    kw = {} if cls is cg.OracleSolver else {"mask": mask}
    scan = p["scan"].copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = slv.run(data.copy(), np.ones_like(p["psi"]), scan, probe.copy().swapaxes(2, 3),
                      piter=piter, recover_prb=recover, **kw)
    return res, scan, slv.history


@pytest.mark.parametrize("nmodes", [1, 2])
def test_all_ones_mask_is_the_oracle_bitwise(nmodes):
    p, probe, data = problem(nmodes)
    want, wscan, whist = run(cg.OracleSolver, p, probe, data)
    got, gscan, ghist = run(ReferenceSolver, p, probe, data, mask=np.ones(data.shape[-2:], np.float32))
    assert np.array_equal(got["psi"], want["psi"])
    assert np.array_equal(got["probe"], want["probe"])
    assert np.array_equal(gscan, wscan)
    assert ghist == whist


@pytest.mark.parametrize("garbage", [np.nan, -1.0, 1e30])
def test_masked_reference_ignores_unmeasured_data(garbage):
    p, probe, data = problem(1)
    mask = detector_mask(data.shape[-1], beamstop=2, gap=1, dead=0.05, seed=4)
    assert 0 < (mask == 0).sum() < mask.size
    zero = np.where(mask != 0, data, 0).astype(np.float32)
    bad = np.where(mask != 0, data, garbage).astype(np.float32)
    want, wscan, whist = run(ReferenceSolver, p, probe, zero, mask=mask, piter=4)
    got, gscan, ghist = run(ReferenceSolver, p, probe, bad, mask=mask, piter=4)
    assert np.isfinite(got["psi"]).all()
    assert np.array_equal(got["psi"], want["psi"]) and np.array_equal(got["probe"], want["probe"])
    assert np.array_equal(gscan, wscan) and ghist == whist


def test_masked_reference_differs_from_unmasked():
    """The mask changes the sums: a random 30 % mask on consistent data moves the cost and the trajectory."""
    p, probe, data = problem(1)
    mask = random_mask(data.shape[-1])
    a, _, ha = run(ReferenceSolver, p, probe, data, mask=mask, piter=3)
    b, _, hb = run(ReferenceSolver, p, probe, data, piter=3)
    assert ha[0][3] < hb[0][3]
    assert not np.array_equal(a["psi"], b["psi"])


def test_masked_reference_rejects_bad_masks():
    p, probe, data = problem(1)
    with pytest.raises(ValueError):
        run(ReferenceSolver, p, probe, data, mask=np.ones((8, 8)), piter=1)
    with pytest.raises(ValueError):
        run(ReferenceSolver, p, probe, data, mask=np.zeros(data.shape[-2:]), piter=1)


def test_test_masks_layout():
    m = detector_mask(64)
    assert m.dtype == np.uint8 and m.shape == (64, 64)
    assert m[0, 0] == 0 and m[-1, -1] == 0 and m[0, -1] == 0   # beamstop at DC = the corners in memory
    assert 0.75 < m.mean() < 0.97
    r = random_mask(64)
    assert 0.6 < r.mean() < 0.8


@pytest.fixture(scope="module")
def nat():
    import __graft_entry__ as ge
    ge.build_native()
    from libtike.hipfft import _native
    return _native


def test_set_mask_abi_without_gpu(nat):
    assert "ptycho_set_mask" in nat.SYMBOLS and hasattr(nat.lib, "ptycho_set_mask")
    assert nat.set_mask(None, None, None) == 1
    assert b"null handle" in nat.last_error()
    assert nat.get(None, nat.GET_MASK) == -1


def test_run_takes_a_mask_keyword():
    import libtike.hipfft as pt
    params = list(inspect.signature(pt.CGPtychoSolver.run).parameters)
    assert params[:9] == ["self", "data", "psi", "scan", "probe", "piter", "model", "recover_prb", "ortho_prb"]
    assert params[9] == "mask"
    assert inspect.signature(pt.CGPtychoSolver.run).parameters["mask"].default is None


def record(rng, nscan=6, ndet=16):
    data = rng.random((nscan, ndet, ndet)).astype(np.float32)
    pos_m = np.stack([rng.uniform(-2e-6, 2e-6, nscan), rng.uniform(-1e-6, 3e-6, nscan)], axis=1)
    return {"data": data, "positions_0": pos_m, "positions_1": pos_m,
            "initprobe": (rng.random((1, ndet, ndet)) + 0j).astype(np.complex64),
            "recprobe": (rng.random((1, ndet, ndet)) + 0j).astype(np.complex64),
            "detector_pixel_size": 75e-6, "detector_distance": 2.0, "incident_wavelength": 1.4,
            "rotation_angle": 0.0}


def test_from_record_reads_and_shifts_the_mask(tmp_path):
    rng = np.random.default_rng(5)
    rec = record(rng)
    centred = (rng.random((16, 16)) > 0.2).astype(np.uint8)
    rec["mask"] = centred
    ds = io.PtychoDataset.from_record(rec, view_dims=(64, 64))
    assert np.array_equal(ds.mask, np.fft.fftshift(centred))
    assert np.array_equal(io.solver_inputs(ds, (64, 64))["mask"], ds.mask)
    ds0 = io.PtychoDataset.from_record(rec, view_dims=(64, 64), data_fftshift=False)
    assert np.array_equal(ds0.mask, centred)
    path = tmp_path / "scan_1_2.npz"
    np.savez(path, **rec)
    assert np.array_equal(io.PtychoDataset.from_npz(path, view_dims=(64, 64)).mask, np.fft.fftshift(centred))
    rec["mask"] = centred[:8]
    with pytest.raises(ValueError):
        io.PtychoDataset.from_record(rec, view_dims=(64, 64))


def test_records_without_mask_are_unchanged():
    rng = np.random.default_rng(6)
    rec = record(rng)
    ds = io.PtychoDataset.from_record(rec, view_dims=(64, 64))
    assert ds.mask is None
    inp = io.solver_inputs(ds, (64, 64))
    assert sorted(inp) == ["data", "probe", "psi", "scan"]
