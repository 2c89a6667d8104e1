"""NumPy reference of the CG loop with the Poisson maximum-likelihood model (``CGPtychoSolver.run(..., model="poisson_ml")``).

``PoissonOracleSolver.run`` with ``model="poisson_ml"`` is the reference's ``model="poisson"`` branch (``ptycho.py:308-313,
357-363, 436-441``) with its one defect removed: ``fpsi`` is ``fwd(psi, probe_k) * (b / a)`` as in the gaussian branch.
Per iteration:

* probe rescale: ``a = sum sqrt(I d)``, ``b = sum I``, ``probe *= a / b``, ``I *= (a / b)^2`` (unchanged);
* object residual of mode k: ``fpsi - d fpsi / (I + 1e-32)``; ``gradpsi = sum_k adj(r_k, probe_k) / max|probe_k|^2``;
* probe residual: ``fprb - d fprb / (I + 1e-32)``; ``gradprb = adj_probe(.) / max|psi|^2 / nscan`` (no ``* nmodes``);
* cost, logged and in every line-search trial: ``f(I) = sum (|I| - d ln(|I| + 1e-32))``.

Dai-Yuan, ``line_search_sqr``, the registration and the history format are the oracle's own.  ``mask=`` follows the rules
of ``tests/masked_cg.py``: data, the intensities, the cost's argument and the residuals are selected to 0 at unmeasured
pixels, so every term of ``f`` there is exactly 0.  Every other model goes to ``MaskedOracleSolver.run`` (``"poisson"``
raises ``UnboundLocalError`` there, as in the reference).
"""
import numpy as np

from oracle.cg_oracle import line_search_sqr, register_translation_batch

from masked_cg import MaskedOracleSolver

__all__ = ["PoissonOracleSolver", "poisson_cost", "poisson_residual"]


def poisson_cost(x, data):
    """``sum (|x| - d ln(|x| + 1e-32))`` in the precision of its arguments."""
    return np.sum(np.abs(x) - data * np.log(np.abs(x) + 1e-32))


def poisson_residual(fp, inten, data):
    """``fp - d fp / (I + 1e-32)``: the farplane whose adjoint is half the gradient of ``poisson_cost(|fp|^2)``."""
    return fp - data * fp / (inten + 1e-32)


class PoissonOracleSolver(MaskedOracleSolver):
    def run(self, data, psi, scan, probe, piter, model="gaussian",
            recover_prb=False, ortho_prb=False, verbose=False, mask=None):
        if model != "poisson_ml":
            return super().run(data, psi, scan, probe, piter, model=model, recover_prb=recover_prb,
                               ortho_prb=ortho_prb, verbose=verbose, mask=mask)
        assert probe.ndim == 4, "probe needs 4 dimensions, not %d" % probe.ndim
        if mask is None:
            def keep(x):
                return x
        else:
            mask = np.asarray(mask) != 0
            if mask.shape != (self.ndet, self.ndet):
                raise ValueError("mask shape")
            if not mask.any():
                raise ValueError("mask has no measured pixel")

            def keep(x):
                return np.where(mask, x, np.zeros((), dtype=x.dtype))

        data = keep(np.asarray(data))
        nmodes = probe.shape[1]

        def minf(x):
            return poisson_cost(keep(x), data)

        def intensity(obj):
            acc = data * 0
            for k in range(nmodes):
                acc += np.abs(self.fwd(obj, scan, probe[:, k])) ** 2
            return keep(acc)

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
                gradpsi += self.adj(keep(poisson_residual(fpsi, absfpsi, data)),
                                    scan, probe[:, k]) / (np.max(np.abs(probe[:, k])) ** 2)
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
                    gradprb[:, m] = self.adj_probe(
                        keep(poisson_residual(fprb, absfprb, data)), scan, psi,
                    ) / np.max(np.abs(psi)) ** 2 / self.nscan
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

            cost = float(minf(absfpsi))
            self.history.append((i, float(gammapsi), float(gammaprb), cost))
            if verbose and i % 32 == 0:
                print("%4d, %.3e, %.3e, %.7e" % self.history[-1])
        return {"psi": psi, "probe": probe}
