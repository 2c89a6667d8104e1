"""NumPy reference of the CG loop with every option of ``CGPtychoSolver.run``: the measured-pixel mask, the Poisson
maximum-likelihood model and orthogonal probe modes.

``ReferenceSolver.run`` is ``oracle.cg_oracle.OracleSolver.run`` (operators, ``line_search_sqr``, the registration and the
history format are the oracle's own) plus:

* ``mask=``: every sum over detector pixels is restricted to the measured pixels (``mask != 0``).  ``data`` is selected
  to 0 at unmeasured pixels before it enters any arithmetic, and so are the intensities, the argument of the cost (the
  logged cost and every line-search trial) and the object and probe residuals.  A select, never a product, so NaN / Inf
  in unmeasured data cannot leak; with an all-ones mask every select returns its input.  ``mask=None`` selects nothing.
* ``model="poisson_ml"``: the reference's ``model="poisson"`` branch (``ptycho.py:308-313, 357-363, 436-441``) with its
  one defect removed, ``fpsi`` is ``fwd(psi, probe_k) * (b / a)`` as in the gaussian branch.  Object residual of mode k
  ``fpsi - d fpsi / (I + 1e-32)``, probe residual ``fprb - d fprb / (I + 1e-32)`` with no ``* nmodes`` on the probe
  gradient, cost ``f(I) = sum (|I| - d ln(|I| + 1e-32))``; at an unmeasured pixel every term of ``f`` is exactly 0.
  ``model="poisson"`` itself raises ``UnboundLocalError`` at its first iteration, as in the reference.
* ``ortho_prb=True``: with ``recover_prb=True`` and two or more modes, after every mode has been updated the probe is
  replaced by its orthogonalised modes (``tests/ortho_modes.py``: ``P V`` with ``V`` the eigenvectors of ``P^H P``,
  descending powers), and ``dprb`` and ``gradprb0`` are rotated by the same ``V`` so that the per-mode Dai-Yuan
  directions stay in the new basis.  ``gradprb`` is overwritten before it is read and is not rotated.  The powers of the
  last orthogonalisation are kept in ``self.mode_powers``.

With every option off the result is the bits of ``OracleSolver.run``.
"""
import numpy as np

from oracle.cg_oracle import OracleSolver, line_search_sqr, register_translation_batch

from ortho_modes import orthogonalize

__all__ = ["ReferenceSolver", "poisson_cost", "poisson_residual", "detector_mask", "random_mask"]


def poisson_cost(x, data):
    """``sum (|x| - d ln(|x| + 1e-32))`` in the precision of its arguments."""
    return np.sum(np.abs(x) - data * np.log(np.abs(x) + 1e-32))


def poisson_residual(fp, inten, data):
    """``fp - d fp / (I + 1e-32)``: the farplane whose adjoint is half the gradient of ``poisson_cost(|fp|^2)``."""
    return fp - data * fp / (inten + 1e-32)


def detector_mask(ndet, beamstop=None, gap=2, dead=0.02, seed=0):
    """Mask of a detector frame in memory layout (DC at [0, 0]): a beamstop disc over the central beam (the four
    corners in memory), a ``gap``-pixel cross of module gaps through the centre of the centred frame, and a fraction
    ``dead`` of random dead pixels.  uint8, 1 = measured."""
    beamstop = max(2, ndet // 16) if beamstop is None else beamstop
    c = np.arange(ndet) - ndet // 2
    m = np.ones((ndet, ndet), dtype=bool)
    m &= (c[:, None] ** 2 + c[None, :] ** 2) > beamstop ** 2
    h = ndet // 2 + ndet // 5                     # module gaps off the centre line, through the centred frame
    m[h:h + gap, :] = False
    m[:, h:h + gap] = False
    m &= np.random.default_rng(seed).random((ndet, ndet)) >= dead
    return np.fft.ifftshift(m).astype(np.uint8)


def random_mask(ndet, fraction=0.3, seed=1):
    """A fraction ``fraction`` of the pixels unmeasured, at random.  uint8, 1 = measured."""
    return (np.random.default_rng(seed).random((ndet, ndet)) >= fraction).astype(np.uint8)


def dai_yuan(grad, grad0, d):
    """The next direction from the gradient, the previous gradient and the previous direction (complex beta, as in
    the reference)."""
    return -grad + (np.linalg.norm(grad) ** 2 / (np.sum(np.conj(d) * (grad - grad0))) * d)


class ReferenceSolver(OracleSolver):
    mode_powers = None

    def run(self, data, psi, scan, probe, piter, model="gaussian",
            recover_prb=False, ortho_prb=False, verbose=False, mask=None):
        assert probe.ndim == 4, "probe needs 4 dimensions, not %d" % probe.ndim
        assert model in ("gaussian", "poisson", "poisson_ml"), model
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
        gaussian = model == "gaussian"

        def minf(x):
            x = keep(x)
            if gaussian:
                return np.linalg.norm(np.sqrt(np.abs(x)) - np.sqrt(data)) ** 2
            return poisson_cost(x, data)

        def residual(f, inten):
            if gaussian:
                return keep(f - np.sqrt(data) * f / (np.sqrt(inten) + 1e-32))
            return keep(poisson_residual(f, inten, data))

        def intensity(obj):
            acc = data * 0
            for k in range(nmodes):
                acc += np.abs(self.fwd(obj, scan, probe[:, k])) ** 2
            return keep(acc)

        prb_scale = nmodes if gaussian else 1
        gammaprb = 0
        for i in range(piter):
            # object step
            absfpsi = intensity(psi)
            a = np.sum(np.sqrt(absfpsi * data))
            b = np.sum(absfpsi)
            probe *= (a / b)
            absfpsi *= (a / b) ** 2
            gradpsi = np.zeros([self.ptheta, self.nz, self.n], dtype="complex64")
            for k in range(nmodes):
                if model != "poisson":                  # reference bug kept: its poisson branch never assigns fpsi
                    fpsi = self.fwd(psi, scan, probe[:, k]) * (b / a)
                gradpsi += self.adj(residual(fpsi, absfpsi), scan, probe[:, k]) / (np.max(np.abs(probe[:, k])) ** 2)
            dpsi = -gradpsi if i == 0 else dai_yuan(gradpsi, gradpsi0, dpsi)
            gradpsi0 = gradpsi
            p1, p2, p3 = data * 0, data * 0, data * 0
            for k in range(nmodes):
                t1 = self.fwd(psi, scan, probe[:, k])
                t2 = self.fwd(dpsi, scan, probe[:, k])
                p1 += np.abs(t1) ** 2
                p2 += np.abs(t2) ** 2
                p3 += 2 * (t1.real * t2.real + t1.imag * t2.imag)
            gammapsi = 0.5 * line_search_sqr(minf, p1, p2, p3)
            if i > 0:                                   # position correction: does not read data
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
                    dprb[:, m] = -gradprb[:, m] if i == 0 else dai_yuan(gradprb[:, m], gradprb0[:, m], dprb[:, m])
                    gradprb0[:, m] = gradprb[:, m]
                    p1 = intensity(psi)
                    t1 = self.fwd(psi, scan, probe[:, m])
                    t2 = self.fwd(psi, scan, dprb[:, m])
                    p2 = np.abs(t2) ** 2
                    p3 = 2 * (t1.real * t2.real + t1.imag * t2.imag)
                    gammaprb = 0.5 * line_search_sqr(minf, p1, p2, p3, step_length=1)
                    probe[:, m] = probe[:, m] + gammaprb * dprb[:, m]
                if ortho_prb and nmodes > 1:            # orthogonal modes, and the CG memory in their basis
                    new, (d_new, g0_new), powers, _ = orthogonalize(probe, dprb, gradprb0)
                    probe[:] = new.astype(probe.dtype)
                    dprb[:] = d_new.astype(dprb.dtype)
                    gradprb0[:] = g0_new.astype(gradprb0.dtype)
                    self.mode_powers = powers

            cost = float(minf(absfpsi))      # start-of-iteration value
            self.history.append((i, float(gammapsi), float(gammaprb), cost))
            if verbose and i % 32 == 0:
                print("%4d, %.3e, %.3e, %.7e" % self.history[-1])
        return {"psi": psi, "probe": probe}
