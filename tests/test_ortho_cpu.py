"""Orthogonal probe modes, host side: the NumPy reference of tests/ortho_modes.py and tests/cg_reference.py held to its
defining properties, the Jacobi solve of csrc/k_modes.hpp built with the host compiler against numpy.linalg.eigh, and
the C ABI's argument checks.  No GPU needed."""
import ctypes
import os
import sys
import warnings

import numpy as np
import pytest

from libtike.hipfft import synthetic as syn
from oracle import cg_oracle as cg
from oracle import ptycho_oracle as op

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import host_build  # noqa: E402
import ortho_modes as om  # noqa: E402
from cg_reference import ReferenceSolver  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


mixed_probe = om.mixed_probe


@pytest.mark.parametrize("nmodes", [2, 3, 5, 8])
def test_reference_modes_are_orthogonal_and_sorted(nmodes):
    probe = mixed_probe(nmodes)
    new, _, powers, v = om.orthogonalize(probe)
    g = om.gram(new)
    for t in range(probe.shape[0]):
        off = g[t] - np.diag(np.diag(g[t]))
        assert np.abs(off).max() <= 1e-12 * np.abs(np.diag(g[t])).max()
        assert np.all(np.diff(powers[t]) < 0)
        assert np.allclose(np.diag(g[t]).real, powers[t], rtol=1e-12, atol=0)
        assert abs(powers[t].sum() - np.sum(np.abs(probe[t].astype(np.complex128)) ** 2)) <= 1e-12 * powers[t].sum()
        assert np.allclose(v[t].conj().T @ v[t], np.eye(nmodes), atol=1e-13)
        # phase convention: the largest component of every column is real and positive
        for j in range(nmodes):
            k = np.argmax(np.abs(v[t][:, j]))
            assert v[t][k, j].imag == 0 and v[t][k, j].real > 0


def test_reference_is_idempotent():
    probe = mixed_probe(4, seed=1)
    once = om.orthogonalize(probe)[0]
    twice = om.orthogonalize(once)[0]
    assert np.abs(twice - once).max() <= 1e-12 * np.abs(once).max()


def test_reference_reverses_ascending_modes():
    probe = syn.hermite_modes(32, 4)[:, ::-1].copy()        # orthogonal by symmetry, weakest first
    probe[:, 1] *= 0.9                                       # 0.25, 0.45, 0.5, 1: distinct powers
    new, _, powers, v = om.orthogonalize(probe)
    assert np.all(np.diff(powers[0]) < 0)
    assert np.abs(new[0] - probe[0, ::-1]).max() <= 1e-6 * np.abs(probe).max()


def test_reference_leaves_one_mode_unchanged():
    probe = mixed_probe(1, seed=2)
    new, (c,), powers, v = om.orthogonalize(probe, probe * 2)
    assert np.array_equal(v, np.ones((2, 1, 1)))
    assert np.array_equal(new.astype(np.complex64), probe) and np.array_equal(c.astype(np.complex64), probe * 2)


def test_reference_keeps_the_summed_farplane_intensity():
    p = syn.make_problem(4, 4, 4, 16, 16, seed=3)
    probe = mixed_probe(3, nprb=16, ptheta=1, seed=3)
    new = om.orthogonalize(probe)[0]

    def inten(modes):
        return sum(np.abs(op.fwd(p["psi"].astype(np.complex128), p["scan"], modes[:, k], 16, "double")) ** 2
                   for k in range(modes.shape[1]))
    before, after = inten(probe.astype(np.complex128)), inten(new)
    assert np.abs(after - before).max() <= 1e-12 * before.max()


def test_reference_rotates_companions_by_the_same_v():
    probe = mixed_probe(3, seed=4)
    d, g0 = mixed_probe(3, seed=5), mixed_probe(3, seed=6)
    _, (d2, g2), _, v = om.orthogonalize(probe, d, g0)
    for t in range(2):
        want = (d[t].reshape(3, -1).T.astype(np.complex128) @ v[t]).T.reshape(d[t].shape)
        assert np.abs(d2[t] - want).max() <= 1e-12 * np.abs(want).max()
    assert np.abs(g2 - om.rotate(g0, v)).max() == 0


# ---- the host build of k_modes.hpp's Jacobi solve ----------------------------------------------------------------------
@pytest.fixture(scope="module")
def host_jacobi(tmp_path_factory):
    program = host_build.build("host_jacobi", tmp_path_factory.mktemp("jacobi"))

    def solve(mats):
        text = []
        for g in mats:
            text.append(str(g.shape[0]))
            text.extend("%.17g %.17g" % (z.real, z.imag) for z in g.ravel())
        words = program(stdin="\n".join(text) + "\n").stdout.split()
        res, pos = [], 0
        for g in mats:
            m = g.shape[0]
            sweeps = int(words[pos])
            lam = np.array([float(w) for w in words[pos + 1:pos + 1 + m]])
            vals = np.array([float(w) for w in words[pos + 1 + m:pos + 1 + m + 2 * m * m]])
            res.append((sweeps, lam, (vals[0::2] + 1j * vals[1::2]).reshape(m, m)))
            pos += 1 + m + 2 * m * m
        return res
    return solve


def random_hermitian(m, rng):
    a = rng.standard_normal((m, m)) + 1j * rng.standard_normal((m, m))
    return a @ a.conj().T                                   # positive semi-definite, like a Gram matrix


@pytest.mark.parametrize("m", list(range(2, 17)))
def test_host_jacobi_matches_eigh(host_jacobi, m):
    rng = np.random.default_rng(100 + m)
    mats = [random_hermitian(m, rng) for _ in range(4)]
    mats.append(om.gram(mixed_probe(m, nprb=8, ptheta=1, seed=m))[0])
    for g, (sweeps, lam, v) in zip(mats, host_jacobi(mats)):
        lam_ref, v_ref = om.mode_eig(g)
        scale = np.abs(lam_ref).max()
        assert sweeps < 40
        assert np.abs(lam - lam_ref).max() <= 1e-12 * scale, (lam, lam_ref)
        for j in range(m):                                   # distinct eigenvalues: each column is unique
            gap = np.min(np.abs(np.delete(lam_ref, j) - lam_ref[j])) / scale
            assert gap > 1e-9
            assert np.abs(v[:, j] - v_ref[:, j]).max() <= 1e-13 / gap, (j, gap, np.abs(v[:, j] - v_ref[:, j]).max())
        assert np.allclose(v.conj().T @ v, np.eye(m), atol=1e-13)


@pytest.mark.parametrize("m", [2, 3, 4, 8, 12, 16])
def test_host_jacobi_rank_deficient(host_jacobi, m):
    rng = np.random.default_rng(200 + m)
    p = rng.standard_normal((5, m)) + 1j * rng.standard_normal((5, m))
    p[:, m // 2] = 0                                          # a zero mode, and rank <= 5 < m for m > 5
    zero_mode = p.conj().T @ p
    mats = [zero_mode, np.zeros((m, m), complex), np.eye(m, dtype=complex) * 3.0]
    for g, (sweeps, lam, v) in zip(mats, host_jacobi(mats)):
        lam_ref = np.linalg.eigvalsh(g)[::-1]
        scale = max(np.abs(lam_ref).max(), 1e-300)
        assert np.abs(lam - lam_ref).max() <= 1e-12 * scale
        assert np.all(np.diff(lam) <= 0)
        assert np.allclose(v.conj().T @ v, np.eye(m), atol=1e-13)
        assert np.abs(v @ np.diag(lam) @ v.conj().T - g).max() <= 1e-12 * scale


def test_host_jacobi_diagonal_input_is_a_permutation(host_jacobi):
    g = np.diag([1.0, 4.0, 2.0, 4.0]).astype(complex)    # an exact tie: stable by index
    (_, lam, v), = host_jacobi([g])
    assert list(lam) == [4.0, 4.0, 2.0, 1.0]
    assert np.array_equal(v, np.eye(4)[:, [1, 3, 2, 0]])


# ---- the CG reference with ortho_prb --------------------------------------------------------------------------------------
def cg_problem(nmodes, ndet=16, seed=3):
    p = syn.make_problem(4, 4, 4, ndet, ndet, seed=seed)
    probe = syn.hermite_modes(ndet, nmodes)
    ora = ReferenceSolver(p["nscan"], ndet, ndet, 1, p["nz"], p["n"])
    data = np.zeros((1, p["nscan"], ndet, ndet), np.float32)
    for k in range(nmodes):
        data += np.abs(ora.fwd(p["psi"], p["scan"], probe[:, k])) ** 2
    rng = np.random.default_rng(seed)
    start = (probe * np.exp(1j * rng.random(probe.shape[-2:]))).astype(np.complex64)
    return p, start, data


def cg_run(cls, p, start, data, **kw):
    ndet = data.shape[-1]
    slv = cls(p["nscan"], ndet, ndet, 1, p["nz"], p["n"], precision="double")
    scan = p["scan"].copy()
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = slv.run(data.copy(), np.ones_like(p["psi"]), scan, start.copy(), piter=3, **{"recover_prb": True, **kw})
    return res, slv


@pytest.mark.parametrize("model", ["gaussian", "poisson_ml"])
def test_cg_reference_returns_orthogonal_modes(model):
    p, start, data = cg_problem(3)
    res, slv = cg_run(ReferenceSolver, p, start, data, ortho_prb=True, model=model)
    plain, pslv = cg_run(ReferenceSolver, p, start, data, ortho_prb=False, model=model)
    g = om.gram(res["probe"])[0]
    d = np.diag(g).real
    assert np.abs(g - np.diag(np.diag(g))).max() <= 1e-5 * d.max()
    assert np.all(np.diff(d) < 0)
    assert np.allclose(slv.mode_powers[0], d, rtol=1e-5)
    assert slv.history[0] == pslv.history[0]                  # the first rotation comes after the first cost
    assert not np.array_equal(res["probe"], plain["probe"])


def test_cg_reference_without_ortho_is_the_oracle():
    """ortho_prb=False is the oracle's loop bit for bit, and so is ortho_prb=True where it does not act (one mode, or no
    probe recovery)."""
    for nmodes, recover, ortho in [(2, True, False), (1, True, False), (3, True, False), (1, False, False),
                                   (3, False, False), (1, True, True), (3, False, True)]:
        p, start, data = cg_problem(nmodes)
        a, sa = cg_run(ReferenceSolver, p, start, data, ortho_prb=ortho, recover_prb=recover)
        b, sb = cg_run(cg.OracleSolver, p, start, data, recover_prb=recover)
        assert np.array_equal(a["probe"], b["probe"]) and np.array_equal(a["psi"], b["psi"]), (nmodes, recover, ortho)
        assert sa.history == sb.history, (nmodes, recover, ortho)


@pytest.mark.parametrize("model", ["gaussian", "poisson_ml"])
def test_cg_reference_all_ones_mask_is_no_mask_bitwise(model):
    p, start, data = cg_problem(3)
    a, sa = cg_run(ReferenceSolver, p, start, data, ortho_prb=True, model=model)
    b, sb = cg_run(ReferenceSolver, p, start, data, ortho_prb=True, model=model, mask=np.ones(data.shape[-2:], np.float32))
    assert np.array_equal(a["probe"], b["probe"]) and np.array_equal(a["psi"], b["psi"]) and sa.history == sb.history
    assert np.array_equal(sa.mode_powers, sb.mode_powers)


# ---- C ABI ------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def nat():
    from libtike.hipfft import _native
    return _native


def test_orthogonalize_symbol_is_declared_and_exported(nat):
    text = open(os.path.join(ROOT, "include", "ptycho_hip.h")).read()
    assert "int ptycho_orthogonalize_modes(" in text
    assert "ptycho_orthogonalize_modes" in nat.SYMBOLS and hasattr(nat.lib, "ptycho_orthogonalize_modes")


def test_orthogonalize_rejects_bad_arguments_without_a_gpu(nat):
    dummy = ctypes.c_void_p(0x1000)         # never dereferenced: every rejection comes before any HIP call
    powers = (ctypes.c_double * 32)()
    v = ctypes.c_void_p(0x2000)
    for nmodes in (0, -1, 17):
        assert nat.orthogonalize_modes(dummy, None, None, 1, nmodes, 64, v, powers, None) == 1
        assert b"nmodes" in nat.last_error()
    assert nat.orthogonalize_modes(None, None, None, 1, 2, 64, v, powers, None) == 1            # null prb
    assert nat.orthogonalize_modes(dummy, None, None, 1, 2, 0, v, powers, None) == 1            # npix == 0
    assert nat.orthogonalize_modes(dummy, None, None, 0, 2, 64, v, powers, None) == 1           # ptheta == 0
    assert nat.orthogonalize_modes(dummy, None, None, 1, 2, 64, None, powers, None) == 1        # v_out
    assert nat.orthogonalize_modes(dummy, None, None, 1, 2, 64, v, None, None) == 1             # powers


def test_orthogonalize_modes_wants_a_device_tensor():
    import libtike.hipfft as pt
    with pytest.raises(TypeError):
        pt.orthogonalize_modes(np.zeros((1, 2, 4, 4), np.complex64))
