"""NumPy reference of the CG loop with orthogonal probe modes (``CGPtychoSolver.run(..., ortho_prb=True)``).

``OrthoOracleSolver.run`` is the loop of ``tests/masked_cg.py`` (``model="gaussian"``) or ``tests/poisson_cg.py``
(``model="poisson_ml"``), mask rules included, plus one step at the end of every iteration's probe step, after every mode
has been updated: with ``recover_prb=True``, ``ortho_prb=True`` and two or more modes, the probe is replaced by its
orthogonalised modes (``tests/ortho_modes.py``: ``P V`` with ``V`` the eigenvectors of ``P^H P``, descending powers),
and ``dprb`` and ``gradprb0`` are rotated by the same ``V`` so that the per-mode Dai-Yuan directions stay in the new
basis.  ``gradprb`` is overwritten before it is read and is not rotated.  ``ortho_prb=False`` is the plain loop.
The powers of the last orthogonalisation are kept in ``self.mode_powers``.
"""
import numpy as np

from oracle.cg_oracle import line_search_sqr, register_translation_batch

from ortho_modes import orthogonalize
from poisson_cg import PoissonOracleSolver, poisson_cost, poisson_residual

__all__ = ["OrthoOracleSolver"]


class OrthoOracleSolver(PoissonOracleSolver):
    mode_powers = None

    def run(self, data, psi, scan, probe, piter, model="gaussian",
            recover_prb=False, ortho_prb=False, verbose=False, mask=None):
        if not ortho_prb:
            return super().run(data, psi, scan, probe, piter, model=model, recover_prb=recover_prb,
                               verbose=verbose, mask=mask)
        assert probe.ndim == 4 and model in ("gaussian", "poisson_ml")
        if mask is None:
            mask = np.ones((self.ndet, self.ndet), dtype=bool)
        mask = np.asarray(mask) != 0

        def keep(x):
            return np.where(mask, x, np.zeros((), dtype=x.dtype))

        data = keep(np.asarray(data))
        nmodes = probe.shape[1]

        def minf(x):
            x = keep(x)
            if model == "gaussian":
                return np.linalg.norm(np.sqrt(np.abs(x)) - np.sqrt(data)) ** 2
            return poisson_cost(x, data)

        def residual(f, inten):
            if model == "gaussian":
                return keep(f - np.sqrt(data) * f / (np.sqrt(inten) + 1e-32))
            return keep(poisson_residual(f, inten, data))

        def intensity(obj):
            acc = data * 0
            for k in range(nmodes):
                acc += np.abs(self.fwd(obj, scan, probe[:, k])) ** 2
            return keep(acc)

        prb_scale = nmodes if model == "gaussian" else 1
        dpsi = gradpsi0 = 0
        dprb = gradprb0 = 0
        gammaprb = 0
        for i in range(piter):
            absfpsi = intensity(psi)
            a = np.sum(np.sqrt(absfpsi * data))
            b = np.sum(absfpsi)
            probe *= (a / b)
            absfpsi *= (a / b) ** 2
            gradpsi = np.zeros([self.ptheta, self.nz, self.n], dtype="complex64")
            for k in range(nmodes):
                fpsi = self.fwd(psi, scan, probe[:, k]) * (b / a)
                gradpsi += self.adj(residual(fpsi, absfpsi), scan, probe[:, k]) / (np.max(np.abs(probe[:, k])) ** 2)
            if i == 0:
                dpsi = -gradpsi
            else:
                dpsi = -gradpsi + (
                    np.linalg.norm(gradpsi) ** 2
                    / (np.sum(np.conj(dpsi) * (gradpsi - gradpsi0))) * dpsi)
            gradpsi0 = gradpsi
            p1, p2, p3 = data * 0, data * 0, data * 0
            for k in range(nmodes):
                t1 = self.fwd(psi, scan, probe[:, k])
                t2 = self.fwd(dpsi, scan, probe[:, k])
                p1 += np.abs(t1) ** 2
                p2 += np.abs(t2) ** 2
                p3 += 2 * (t1.real * t2.real + t1.imag * t2.imag)
            gammapsi = 0.5 * line_search_sqr(minf, p1, p2, p3)
            if i > 0:
                ones = probe[:, 0] * 0 + 1
                t1 = self.fwd(psi, scan, ones)[0]
                t2 = self.fwd(psi + gammapsi * dpsi, scan, ones)[0]
                shifts = register_translation_batch(t1, t2, upsample_factor=100, space="fourier")
                scan[0, :] += shifts
            psi = psi + gammapsi * dpsi

            if recover_prb:
                if i == 0:
                    gradprb = probe * 0
                    gradprb0 = probe * 0
                    dprb = probe * 0
                for m in range(nmodes):
                    fprb = self.fwd(psi, scan, probe[:, m])
                    absfprb = intensity(psi)
                    gradprb[:, m] = self.adj_probe(residual(fprb, absfprb), scan, psi,
                                                   ) / np.max(np.abs(psi)) ** 2 / self.nscan * prb_scale
                    if i == 0:
                        dprb[:, m] = -gradprb[:, m]
                    else:
                        dprb[:, m] = -gradprb[:, m] + (
                            np.linalg.norm(gradprb[:, m]) ** 2
                            / (np.sum(np.conj(dprb[:, m]) * (gradprb[:, m] - gradprb0[:, m])))
                            * dprb[:, m])
                    gradprb0[:, m] = gradprb[:, m]
                    p1 = intensity(psi)
                    t1 = self.fwd(psi, scan, probe[:, m])
                    t2 = self.fwd(psi, scan, dprb[:, m])
                    p2 = np.abs(t2) ** 2
                    p3 = 2 * (t1.real * t2.real + t1.imag * t2.imag)
                    gammaprb = 0.5 * line_search_sqr(minf, p1, p2, p3, step_length=1)
                    probe[:, m] = probe[:, m] + gammaprb * dprb[:, m]
                if nmodes > 1:                  # orthogonal modes, and the CG memory in their basis
                    new, (d_new, g0_new), powers, _ = orthogonalize(probe, dprb, gradprb0)
                    probe[:] = new.astype(probe.dtype)
                    dprb[:] = d_new.astype(dprb.dtype)
                    gradprb0[:] = g0_new.astype(gradprb0.dtype)
                    self.mode_powers = powers

            cost = float(minf(absfpsi))
            self.history.append((i, float(gammapsi), float(gammaprb), cost))
            if verbose and i % 32 == 0:
                print("%4d, %.3e, %.3e, %.7e" % self.history[-1])
        return {"psi": psi, "probe": probe}
