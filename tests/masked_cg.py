"""NumPy reference of the CG loop with a measured-pixel mask (``CGPtychoSolver.run(..., mask=)``).

``MaskedOracleSolver.run`` is ``oracle.cg_oracle.OracleSolver.run`` with every sum over detector pixels restricted to the
measured pixels (``mask != 0``): ``data`` is selected to 0 at unmeasured pixels before it enters any arithmetic, and so
are the intensities, the argument of the gaussian cost (the logged cost and every line-search trial) and the object and
probe residuals.  A select, never a product, so NaN / Inf in unmeasured data cannot leak; with an all-ones mask every
select returns its input and the result is the bits of ``OracleSolver.run``.  Operators, ``line_search_sqr`` and the
registration are the oracle's own.
"""
import numpy as np

from oracle.cg_oracle import OracleSolver, line_search_sqr, register_translation_batch

__all__ = ["MaskedOracleSolver", "detector_mask", "random_mask"]


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


class MaskedOracleSolver(OracleSolver):
    def run(self, data, psi, scan, probe, piter, model="gaussian",
            recover_prb=False, ortho_prb=False, verbose=False, mask=None):
        assert probe.ndim == 4, "probe needs 4 dimensions, not %d" % probe.ndim
        if mask is None:
            mask = np.ones((self.ndet, self.ndet), dtype=bool)
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
            x = keep(x)
            if model == "gaussian":
                return np.linalg.norm(np.sqrt(np.abs(x)) - np.sqrt(data)) ** 2
            elif model == "poisson":
                return np.sum(np.abs(x) - data * np.log(np.abs(x) + 1e-32))

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
            if model == "gaussian":
                for k in range(nmodes):
                    fpsi = self.fwd(psi, scan, probe[:, k]) * (b / a)
                    gradpsi += self.adj(
                        keep(fpsi - np.sqrt(data) * fpsi / (np.sqrt(absfpsi) + 1e-32)),
                        scan, probe[:, k]) / (np.max(np.abs(probe[:, k])) ** 2)
            elif model == "poisson":
                for k in range(nmodes):
                    gradpsi += self.adj(
                        keep(fpsi - data * fpsi / (absfpsi + 1e-32)),   # noqa: F821 (reference bug kept)
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
                    if model == "gaussian":
                        gradprb[:, m] = self.adj_probe(
                            keep(fprb - np.sqrt(data) * fprb / (np.sqrt(absfprb) + 1e-32)),
                            scan, psi,
                        ) / np.max(np.abs(psi)) ** 2 / self.nscan * nmodes
                    elif model == "poisson":
                        gradprb[:, m] = self.adj_probe(
                            keep(fprb - data * fprb / (absfprb + 1e-32)), scan, psi,
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
