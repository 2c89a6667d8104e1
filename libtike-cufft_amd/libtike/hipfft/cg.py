"""CG solver (ptycho.py:250-488): ``CGPtychoSolver``, its driver choice and the statement-by-statement loop."""
import warnings

import numpy as np
import torch

from . import _native as nat
from .cg_device import DeviceDrivers
from .modes import orthogonalize_modes
from .operators import PtychoHIP, _dy_direction
from .registration import register_translation_batch


class CGPtychoSolver(DeviceDrivers, PtychoHIP):
    """Solve the ptychography problem with Dai-Yuan conjugate gradients.

    ``group``: optional ``torch.distributed`` process group; when given, the scan
    positions (``data``, ``scan``) are this rank's shard, ``psi`` / ``probe`` are
    replicated, and the object / probe gradients and every global scalar are
    all-reduced (RCCL over xGMI on MI355X).
    """

    def __init__(self, nscan, probe_shape, detector_shape, ntheta, nz, n, group=None):
        super().__init__(nscan, probe_shape, detector_shape, ntheta, nz, n)
        self.group = group
        self.history = []      # (iteration, gammapsi, gammaprb, cost) per logged iteration
        self.verbose = True
        self.log_every = 32    # the reference prints every 32 iterations (ptycho.py:475)
        self.fused = True      # gaussian loops through the fused CG-stage kernels
        self.native = True     # single-mode loop sequenced by the native stage calls (no host round trips)
        self._nscan_all = None
        self.reproducible = True  # fused CG loops use the deterministic adjoints (same trajectory every run)
        self.share_ones = True    # native loop: the position correction's column passes share the object step's patch gathers
        self.ls_two_pass = None  # native line search with few collectives (<= 16, 32, 80 step lengths); None: with a group only

    def _allreduce(self, t):
        if self.group is not None:
            import torch.distributed as dist
            if torch.is_complex(t):
                dist.all_reduce(torch.view_as_real(t), group=self.group)
            else:
                dist.all_reduce(t, group=self.group)
        return t

    def _nscan_total(self):
        """Positions over all ranks (ptycho.py:431 divides the probe gradient by nscan); one collective
        per solver, not per run."""
        if self.group is None:
            return self.nscan
        if getattr(self, "_nscan_all", None) is None:
            import torch.distributed as dist
            t = torch.tensor([float(self.nscan)], device=self._device)
            dist.all_reduce(t, group=self.group)
            self._nscan_all = int(t.item())
        return self._nscan_all

    @staticmethod
    def line_search_sqr(f, p1, p2, p3, step_length=1, step_shrink=0.5):
        """Backtracking on the closed-form quadratic (``ptycho.py:253-281``)."""
        assert step_shrink > 0 and step_shrink < 1
        m = 0
        fp1 = f(p1)
        while f(p1 + step_length ** 2 * p2 + step_length * p3) > fp1 + step_shrink * m:
            if step_length < 1e-32:
                warnings.warn("Line search failed for conjugate gradient.")
                return 0
            step_length *= step_shrink
        return step_length

    def _log_header(self):
        if self.verbose:
            print("# congujate gradient parameters\niteration, step size object, step size probe, function min")

    def _log(self, i, gammapsi, gammaprb, cost):
        self.history.append((i, gammapsi, gammaprb, cost))
        if self.verbose:
            print("%4d, %.3e, %.3e, %.7e" % self.history[-1])

    def _log_state(self, i, st):
        """``_log`` from a snapshot of the device state vector (the cost summed over the ranks)."""
        snap = st[:nat.ST_LS_FAILED + 1].clone()
        self._allreduce(snap[nat.ST_COST:nat.ST_COST + 1])
        snap = snap.cpu()
        self._log(i, float(snap[nat.ST_GAMMA_PSI]), float(snap[nat.ST_GAMMA_PRB]), float(snap[nat.ST_COST].to(torch.float32)))

    def _replay_ls_failures(self, st):
        """The device-resident loops count failed line searches; warn once per failure, as the reference does."""
        failed = int(st[nat.ST_LS_FAILED].item())
        if failed:
            st[nat.ST_LS_FAILED] = 0.0
            for _ in range(failed):
                warnings.warn("Line search failed for conjugate gradient.")

    @staticmethod
    def _result(psi, probe, powers):
        return {"psi": psi, "probe": probe, **({} if powers is None else {"mode_powers": powers})}

    def _mask_operand(self, mask, device):
        """``mask`` (NumPy array or tensor, any dtype, nonzero = measured) -> uint8 ``[ndet, ndet]`` on ``device``."""
        if mask is None:
            return None
        m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask))
        if tuple(m.shape) != (self.ndet, self.ndet):
            raise ValueError("mask: shape %s != expected %s" % (tuple(m.shape), (self.ndet, self.ndet)))
        m = m != 0
        if not bool(m.any()):
            raise ValueError("mask has no measured pixel (the probe rescale a / b would be 0 / 0)")
        return m.to(device=device, dtype=torch.uint8).contiguous()

    def run(self, data, psi, scan, probe, piter, model="gaussian", recover_prb=False, ortho_prb=False, mask=None):
        """Conjugate gradients for ptychography (``ptycho.py:283-488``).

        ``probe`` and ``scan`` are updated in place, like in the reference.

        ``mask``: measured-pixel mask, shape ``[ndet, ndet]`` in the layout of ``data`` (un-fftshifted, DC at
        ``[0, 0]``); any nonzero value means "measured".  A bool / integer / float NumPy array or tensor; the same mask
        applies to every position and angle.  With a mask every sum over detector pixels runs over the measured pixels
        only: the probe rescale ``a = sum sqrt(I d)``, ``b = sum I``, the gaussian cost ``sum (sqrt I - sqrt d)^2`` (the
        logged cost and every line-search trial), and the object and probe residuals are exactly 0 at unmeasured pixels.
        What ``data`` holds at an unmeasured pixel never matters (NaN and Inf included), and an all-ones mask gives the
        bits of ``mask=None``.  The position correction does not read ``data`` and is unchanged.  ``ValueError`` for a
        mask of the wrong shape or one with no measured pixel.

        ``model``: the noise model of the cost.

        * ``"gaussian"`` (default): least squares on amplitudes, ``f(I) = sum (sqrt|I| - sqrt d)^2``.
        * ``"poisson_ml"``: Poisson maximum likelihood, ``f(I) = sum (|I| - d ln(|I| + 1e-32))``, for photon-counting
          data at low dose.  It is the reference's ``"poisson"`` branch (``ptycho.py:308-313, 357-363, 436-441``) with
          ``fpsi`` defined as in the gaussian branch: object residual ``fpsi - d fpsi / (I + 1e-32)`` per mode, probe
          residual ``fprb - d fprb / (I + 1e-32)``, and a probe gradient that is not multiplied by the number of modes.
          The probe rescale, the Dai-Yuan directions, ``line_search_sqr``, the position correction and the mask rules
          are those of ``"gaussian"``.  The line-search trials are priced minus the per-pixel constant
          ``d - d ln(d + 1e-32)``, which cancels in every comparison and keeps the float32 sums small; the logged
          cost is ``f`` itself.
        * ``"poisson"``: kept exactly as the reference has it, which reads ``fpsi`` before assigning it and so raises
          ``UnboundLocalError`` on its first iteration.  Results of this solver are compared with the reference's, so
          its branches are not changed; ``"poisson_ml"`` is the working form.

        ``ortho_prb``: keep the incoherent probe modes orthogonal (``orthogonalize_modes``).  At the end of every
        iteration's probe step, after every mode has been updated, the modes of each angle are replaced by ``P V``,
        with ``P^H P = V diag(lam) V^H``: mode 0 is then the strongest, ``P^H P = diag(lam)`` with ``lam`` descending
        and ``sum(lam) = sum_k |P_k|^2``.  The summed intensity ``sum_k |F(psi P_k)|^2`` does not change under this
        unitary mixing, so neither do the cost and the next iteration's rescale ``a / b`` (which keeps the modes
        orthogonal).  The probe's CG direction and previous gradient are rotated by the same ``V``, so the per-mode
        Dai-Yuan directions stay in the new basis.  The returned probe is orthogonal and sorted by power, and the
        result gains ``"mode_powers"``: ``lam`` of the last orthogonalisation, a ``[ptheta, M]`` float64 device tensor.
        Nothing happens with ``recover_prb=False`` (the reference placed it inside the probe step) or with one mode.
        Works with ``mask=``, ``"gaussian"`` and ``"poisson_ml"``, ``run_batch`` and a process group (the probe is
        replicated and the kernels are deterministic, so every rank computes the same ``V``).  ``ValueError`` for more
        than 16 modes.
        """
        assert probe.ndim == 4, "probe needs 4 dimensions, not %d" % probe.ndim
        ortho = bool(ortho_prb) and bool(recover_prb) and probe.shape[1] > 1
        if ortho_prb and probe.shape[1] > nat.ORTHO_MAX_MODES:
            raise ValueError("ortho_prb: %d probe modes, supported up to %d" % (probe.shape[1], nat.ORTHO_MAX_MODES))
        mask = self._mask_operand(mask, data.device)
        with self._options(*([(b"model", nat.MODEL_POISSON_ML, nat.MODEL_GAUSSIAN)] if model == "poisson_ml" else []), mask=mask):
            return self._run(data, psi, scan, probe, piter, model, recover_prb, None if mask is None else mask.bool(), ortho)

    def _run(self, data, psi, scan, probe, piter, model, recover_prb, mask, ortho=False):
        nmodes = probe.shape[1]
        pow2 = self._stockham_size()
        # several modes: the compact slot layout runs its line search over position ranges, which needs the windowed
        # column pass (ndet <= 512); larger detectors take the statement-by-statement loop
        if self.fused and model in ("gaussian", "poisson_ml") and pow2 and nmodes <= 8 and (nmodes == 1 or self.ndet <= 512):
            # The fused loops run on the deterministic adjoints unless told otherwise: with float atomics (the
            # reference's kernels.cu:73-80) two runs of the same problem take different line-search paths -- near a
            # flat start the accept / reject decisions sit on the last float32 digit of the cost -- and differ by
            # +-10 % in time (tools/cg_variance.py).  In the loop the fixed-point scale comes from the projection
            # stage, so this costs no extra pass.
            det = self.reproducible and not self._det and self.ndet <= 512 and int(nat.get(self._h, nat.GET_WINDOW)) == 1
            with self._options(*([(b"deterministic", 1, 0)] if det else [])):
                if nmodes == 1:
                    zoom = self._native_ready()
                    if zoom is not None:
                        return self._run_native(data, psi, scan, probe, piter, recover_prb, zoom)
                    return self._run_fused(data, psi, scan, probe, piter, recover_prb)
                return self._run_fused_multi(data, psi, scan, probe, piter, recover_prb,   # one pair of work slots per mode
                                             model, ortho)
        nscan_total = self._nscan_total()
        if mask is not None:
            # measured pixels only: data, the intensities, the line-search terms and the residuals are selected to 0
            # elsewhere (a select, not a product: unmeasured data may be NaN / Inf)
            zero = torch.zeros((), dtype=data.dtype, device=data.device)
            data = torch.where(mask, data, zero)
            keep = lambda x: torch.where(mask, x, torch.zeros((), dtype=x.dtype, device=x.device))  # noqa: E731
        else:
            keep = lambda x: x  # noqa: E731

        def minf(fpsi):
            fpsi = keep(fpsi)
            if model == "gaussian":
                f = torch.sum((torch.sqrt(torch.abs(fpsi)) - torch.sqrt(data)) ** 2)
            elif model in ("poisson", "poisson_ml"):
                f = torch.sum(torch.abs(fpsi) - data * torch.log(torch.abs(fpsi) + 1e-32))
            return self._allreduce(f)

        if model == "poisson_ml":
            # line-search trials: minus the per-pixel constant d - d ln(d + 1e-32) (the term's value at I = d), which
            # cancels in every comparison of line_search_sqr and keeps the float32 sums near the size of the cost
            # differences (as the fused kernels do); the logged cost stays minf
            shift = data - data * torch.log(data + 1e-32)

            def minf_ls(fpsi):
                fpsi = keep(fpsi)
                f = torch.sum(torch.abs(fpsi) - data * torch.log(torch.abs(fpsi) + 1e-32) - shift)
                return self._allreduce(f)
        else:
            minf_ls = minf

        def residual(f, inten):
            if model == "gaussian":
                return keep(f - torch.sqrt(data) * f / (torch.sqrt(inten) + 1e-32))
            return keep(f - data * f / (inten + 1e-32))

        def intensity(obj):
            acc = torch.zeros_like(data)
            for k in range(nmodes):
                acc += torch.abs(self.fwd(obj, scan, probe[:, k])) ** 2
            return keep(acc)

        prb_scale = nmodes if model == "gaussian" else 1    # ptycho.py:431 (gaussian) / :441 (poisson)
        dprb = dpsi = gradprb0 = gradpsi0 = 0
        powers = None
        self._log_header()
        gammaprb = 0
        for i in range(piter):
            # 1) object retrieval subproblem with fixed probes -- :325-405
            absfpsi = intensity(psi)
            ab = torch.stack((torch.sum(torch.sqrt(absfpsi * data)), torch.sum(absfpsi)))
            self._allreduce(ab)
            a, b = ab[0], ab[1]
            probe *= (a / b)
            absfpsi *= (a / b) ** 2
            gradpsi = torch.zeros((self.ptheta, self.nz, self.n), dtype=torch.complex64,
                                  device=data.device)
            for k in range(nmodes):
                if model != "poisson":          # reference bug kept: its poisson branch reads fpsi and never assigns it
                    fpsi = self.fwd(psi, scan, probe[:, k]) * (b / a)
                gradpsi += self.adj(residual(fpsi, absfpsi), scan, probe[:, k]) / (torch.max(torch.abs(probe[:, k])) ** 2)
            self._allreduce(gradpsi)
            dpsi = _dy_direction(i, gradpsi, gradpsi0, dpsi)
            gradpsi0 = gradpsi
            p1, p2, p3 = torch.zeros_like(data), torch.zeros_like(data), torch.zeros_like(data)
            for k in range(nmodes):
                tmp1 = self.fwd(psi, scan, probe[:, k])
                tmp2 = self.fwd(dpsi, scan, probe[:, k])
                p1 += torch.abs(tmp1) ** 2
                p2 += torch.abs(tmp2) ** 2
                p3 += 2 * (tmp1.real * tmp2.real + tmp1.imag * tmp2.imag)
            gammapsi = 0.5 * self.line_search_sqr(minf_ls, p1, p2, p3)

            # position correction -- :398-403
            if i > 0:
                ones = probe[:, 0] * 0 + 1
                tmp1 = self.fwd(psi, scan, ones)[0]
                tmp2 = self.fwd(psi + gammapsi * dpsi, scan, ones)[0]
                shifts = register_translation_batch(tmp1, tmp2, upsample_factor=100,
                                                    space="fourier", op=self)
                scan[0, :] += shifts.to(scan.dtype)
            psi = psi + gammapsi * dpsi

            if recover_prb:                     # :409-465
                if i == 0:
                    gradprb = probe * 0
                    gradprb0 = probe * 0
                    dprb = probe * 0
                for m in range(nmodes):
                    fprb = self.fwd(psi, scan, probe[:, m])
                    absfprb = intensity(psi)
                    g = self.adj_probe(residual(fprb, absfprb), scan, psi)
                    self._allreduce(g)
                    gradprb[:, m] = g / torch.max(torch.abs(psi)) ** 2 / nscan_total * prb_scale
                    dprb[:, m] = _dy_direction(i, gradprb[:, m], gradprb0[:, m], dprb[:, m])
                    gradprb0[:, m] = gradprb[:, m]
                    p1 = intensity(psi)
                    tmp1 = self.fwd(psi, scan, probe[:, m])
                    tmp2 = self.fwd(psi, scan, dprb[:, m])
                    p2 = torch.abs(tmp2) ** 2
                    p3 = 2 * (tmp1.real * tmp2.real + tmp1.imag * tmp2.imag)
                    gammaprb = 0.5 * self.line_search_sqr(minf_ls, p1, p2, p3, step_length=1)
                    probe[:, m] = probe[:, m] + gammaprb * dprb[:, m]
                if ortho:                       # ortho_prb
                    powers = orthogonalize_modes(probe, dprb, gradprb0)

            # check convergence -- :475-482 (cost of the start-of-iteration intensity)
            if i % self.log_every == 0:
                cost = float(minf(absfpsi))
                self._log(i, float(gammapsi), float(gammaprb), cost)
        return self._result(psi, probe, powers)
