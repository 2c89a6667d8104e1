"""The device-side CG drivers of ``CGPtychoSolver`` (native stage loop, fused loop, fused multi-mode loop) and their glue."""
import ctypes
import warnings

import torch

from . import _native as nat
from .modes import orthogonalize_modes
from .operators import _dy_direction, _ptr, _stream
from .registration import (_finish_registration, _zoom_kernel_factors, _zoom_shifts_native, register_translation_batch)

# Line-search pass schedules: the ``pass`` codes of ``ptycho_cg_ls_next``; code p prices ``kLsNext[p]`` (csrc/host_cg.hpp) groups of 16
# step lengths, 4 only decides.  One GPU: 16 + 32 + 64 more step lengths in passes that return at once when resolved; with a
# process group every pass costs a collective: 32, then all 80 that are left (a second pass of all 112
# would save one more collective, but a search that ends at index 30-50 -- a quarter of the bench
# problem's iterations -- would then price 112 step lengths instead of 32: +2 ms per iteration at 4096
# positions; ls_two_pass = "all" selects it)
LS_SINGLE, LS_STAGED = (1, 2, 3), (1, 2, 3, 4)          # one GPU: passes that decide on their own totals / separate decisions
LS_TWO_PASS, LS_ONE_PASS = (6, 7, 4), (5, 4)            # with a process group: ls_two_pass = True / "all"
LS_MULTI_GROUPS = (1, 2, 4, 0)     # multi-mode loop: groups the NEXT pass prices (``ptycho_cg_ls_decide``), after the hint-sized first


class DeviceDrivers:
    """Mixin of ``CGPtychoSolver``: the CG loops that run on the fused HIP stages."""
    def _state(self, dev):
        """The float64 state vector of the native stages, made once per device with both line-search hints at 14.  The
        two step lengths are zeroed: a run without probe recovery logs step 0, as the reference prints."""
        st = self.__dict__.get("_cg_state")
        if st is None or st.device != dev:
            st = self._cg_state = torch.zeros(nat.ST_WORDS, dtype=torch.float64, device=dev)
            st[nat.ST_HINT:nat.ST_HINT + 2] = 14.0
        st[nat.ST_GAMMA_PSI:nat.ST_GAMMA_PRB + 1] = 0.0
        return st

    def _ones(self, probe):
        """The all-ones probe of the position correction (ptycho.py:399), made once per shape and device."""
        ones = self.__dict__.get("_ones_probe")
        if ones is None or ones.shape != probe[:, 0].shape or ones.device != probe.device:
            ones = self._ones_probe = torch.ones_like(probe[:, 0])
        return ones

    def _cg_operands(self, data, psi, scan, probe, contiguous=(), clone=False):
        """``data`` and ``psi`` (or a copy) checked and contiguous; ``scan`` checked; ``contiguous``: tensors used as they are."""
        data = self._operand(data, torch.float32, (self.ptheta, self.nscan, self.ndet, self.ndet), "data")
        psi = self._operand(psi, torch.complex64, (self.ptheta, self.nz, self.n), "psi")
        self._operand(scan, torch.float32, (self.ptheta, self.nscan, 2), "scan")
        assert probe.dtype == torch.complex64 and all(t.is_contiguous() for t in contiguous)
        return data, (psi.clone() if clone else psi)

    def _cg_fwd_cols(self, slot, obj, scan, prb):
        self._note_scan(scan)
        nat.check(nat.cg_fwd_cols(self._h, slot, _ptr(obj), _ptr(scan), _ptr(prb), _stream()))

    def _position_shifts(self, psi, dpsi, gammapsi, scan, probe):
        """Shifts of ptycho.py:398-403.  Fused form (one angle): column passes of
        fwd(psi, 1) and fwd(dpsi, 1), one row pass that forms u1 conj(u1 + gamma u2) and its
        inverse row DFT, one column pass with a fused arg-max; then the zoomed DFT."""
        ones = self._ones(probe)
        if not (self.fused and self.ptheta == 1):
            g32 = gammapsi.to(torch.float32) if isinstance(gammapsi, torch.Tensor) else gammapsi
            tmp1 = self.fwd(psi, scan, ones)[0]
            tmp2 = self.fwd(psi + g32 * dpsi, scan, ones)[0]
            return register_translation_batch(tmp1, tmp2, upsample_factor=100, space="fourier", op=self)
        self._cg_fwd_cols(0, psi, scan, ones)
        self._cg_fwd_cols(1, dpsi, scan, ones)
        # three or more probe modes (compact slot layout): the image product goes to work slot 2, which is
        # free here, instead of a farplane-sized tensor of its own
        in_slot = probe.shape[1] >= 3 and _zoom_kernel_factors(self.ndet, 100, psi.device) is not None
        ip = None if in_slot else torch.empty((self.nscan, self.ndet, self.ndet), dtype=torch.complex64, device=psi.device)
        if isinstance(gammapsi, torch.Tensor):      # the accepted step lives on the device (float64 word)
            nat.check(nat.cg_cross_dev(self._h, 0, 1, _ptr(gammapsi), _ptr(ip) if ip is not None else None, _stream()))
        else:
            nat.check(nat.cg_cross(self._h, 0, 1, float(gammapsi), _ptr(ip) if ip is not None else None, _stream()))
        best = torch.empty(self.nscan, dtype=torch.int64, device=psi.device)
        nat.check(nat.cg_argmax(self._h, 1, _ptr(best), _stream()))
        shifts = _zoom_shifts_native(self, ip, best, 100)
        if shifts is not None:
            return shifts
        idx = 0xffffffff - (best & 0xffffffff)
        maxima = torch.stack((idx // self.ndet, idx % self.ndet), dim=1)
        return _finish_registration(ip, maxima, 100)

    def _fused_line_search(self, data, ab, costs, which="psi"):
        """All trials of ``line_search_sqr`` (ptycho.py:253-281), up to 16 step lengths per
        pass over the two work buffers (p1, p2, p3 never leave registers); returns the
        accepted step length (0 on failure).  Every step length before the accepted one is
        still evaluated and rejected, as in the reference; only the number priced per pass
        adapts: the accepted index moves slowly from one iteration to the next, so a pass
        prices two more than the last accepted index of the same search (``which``) and a
        second pass continues from there if none is accepted.  Measured alternative:
        writing the terms out once and pricing 32 steps per pass from arrays is not faster
        -- each trial step costs ~0.06 ms of sqrt/FMA work at 4096 x 256^2 wherever it is
        evaluated."""
        hints = self.__dict__.setdefault("_ls_hint", {})
        ncand = min(16, max(2, hints.get(which, 14) + 2))
        gamma0 = 1.0
        tried = 0
        while True:
            costs.zero_()
            nat.check(nat.cg_linesearch(self._h, 0, 1, _ptr(data), _ptr(ab) if ab is not None else None,
                                        gamma0, ncand, _ptr(costs), _stream()))
            self._allreduce(costs)
            c = costs.to(torch.float32).cpu().numpy()      # the reference compares float32 costs
            step = gamma0
            for j in range(ncand):
                if not (c[j] > c[ncand]):
                    hints[which] = tried + j
                    return step
                if step < 1e-32:
                    warnings.warn("Line search failed for conjugate gradient.")
                    hints[which] = 14
                    return 0
                step *= 0.5
            gamma0 = step
            tried += ncand
            ncand = 16

    def _native_ready(self):
        """The native stage calls cover one probe mode, any number of angles per call (the position correction touches
        angle 0 only, like ptycho.py:399-403) and detector sizes the fused zoom kernel accepts."""
        return _zoom_kernel_factors(self.ndet, 100, self._device) if self.native else None

    def _run_native(self, data, psi, scan, probe, piter, recover_prb, zoom):
        """``CGPtychoSolver.run`` (ptycho.py:283-488), one probe mode, gaussian or poisson_ml model (option "model" of the
        handle; the probe gradient's mode factor is 1 either way).  Same kernels and
        the same arithmetic as ``_run_fused``, but every scalar of the iteration (a, b, the Dai-Yuan
        sums, the line-search costs, the accepted step lengths) stays in a float64 state vector on the
        device and the line search is decided there (C ABI ``ptycho_cg_obj_* / prb_* / ls_next``): an
        iteration is ~13 library calls and no device synchronisation; the host reads the state back only
        when it logs (every ``log_every`` iterations, as the reference prints every 32).  With a process
        group the scalar messages of a search and the two gradients are all-reduced in between."""
        dev = data.device
        data, psi = self._cg_operands(data, psi, scan, probe, contiguous=(probe, scan), clone=True)
        vt, lz, nc, _ = zoom
        st = self._state(dev)
        h = self._h
        sp, costs = _ptr(st), st[nat.ST_COSTS:nat.ST_COSTS + nat.ST_NCOSTS]
        ones = self._ones(probe)
        grad, grad0, dpsi = torch.empty_like(psi), torch.zeros_like(psi), torch.zeros_like(psi)
        if recover_prb:
            gprb, gprb0, dprb = (torch.zeros_like(probe[:, 0]) for _ in range(3))
        nscan_total = float(self._nscan_total())
        dist_on = self.group is not None
        two_pass = dist_on if self.ls_two_pass is None else self.ls_two_pass
        # one GPU: nothing is all-reduced between the stages, so a line-search pass decides on its own totals (no
        # decision kernel in between) and the gradient goes from the adjoint's fixed-point image straight into the
        # Dai-Yuan pass (no fold-in pass of its own); with a process group the stages stay separate
        single = not dist_on and not two_pass
        schedule = LS_ONE_PASS if two_pass == "all" else LS_TWO_PASS if two_pass else LS_SINGLE if single else LS_STAGED

        with self._options((b"ls_fused_decide", int(single), 0), (b"defer_finish", int(not dist_on), 0)):
            def line_search(which, use_ab, S):
                for p in schedule:
                    if dist_on:
                        self._allreduce(costs)
                    nat.check(nat.cg_ls_next(h, sp, which, p, _ptr(data), use_ab, S))

            # Sharing the patch gathers keeps FOUR farplane-sized work slots on the device (0, 1 and, for the two operands of
            # the position correction, 2 and 3) instead of two: 2 x ptheta x nscan x ndet^2 x 8 bytes more (4 GiB at configs[1],
            # 16 GiB at a configs[3] shard).  Where that does not fit next to what is already allocated the loop runs without
            # sharing (two more column passes per iteration: 8.33 -> 8.39 ms at 4096 x 256^2) and gives slots 2 / 3 back.
            share_fits = self.share_ones and self.ndet <= 512 and self.ptheta == 1 and piter > 1
            if share_fits:
                slot_bytes = (self.ptheta * self.nscan + 8) * self.ndet * self.ndet * 8
                need = sum(slot_bytes for s_ in (2, 3) if not self._slot_allocated(s_))
                if need:
                    free_b = torch.cuda.mem_get_info(dev)[0]
                    if free_b < need + (1 << 30):
                        torch.cuda.empty_cache()
                        free_b = torch.cuda.mem_get_info(dev)[0]
                    share_fits = free_b >= need + (1 << 30)
            if not share_fits:
                for s_ in (2, 3):
                    if self._slot_allocated(s_) and not (s_ == 2 and dist_on):   # (slot 2 serves cg_reg_prepare with a process group)
                        nat.check(nat.set_option(h, b"release_work", s_))

            def iteration(first, correct):
                """One CG iteration as a fixed sequence of launches on the current stream (no host decisions)."""
                S = _stream()
                # 1) object step (ptycho.py:325-405)
                # with the position correction on, its two operands (column passes of fwd(psi, 1) and fwd(dpsi, 1)) ride
                # along with the object step's own column passes: one patch gather per position serves both probes
                share = bool(correct) and share_fits
                # with a process group the column pass of fwd(psi, 1) is better spent under the gradient all-reduce (below)
                op_psi = _ptr(ones) if (share and not dist_on) else None
                op_dpsi = _ptr(ones) if share else None
                nat.check(nat.cg_obj_begin2(h, sp, _ptr(psi), _ptr(scan), _ptr(probe), op_psi, _ptr(data), S))
                if dist_on:
                    self._allreduce(st[nat.ST_A:nat.ST_A + 2])
                nat.check(nat.cg_obj_grad(h, sp, _ptr(scan), _ptr(probe), _ptr(data), _ptr(grad), S))
                if dist_on:
                    # the gradient all-reduce runs on the communicator's stream; the first operand of the position
                    # correction (column pass of fwd(psi, 1): depends on psi and scan only) is computed under it
                    import torch.distributed as dist
                    work = dist.all_reduce(torch.view_as_real(grad), group=self.group, async_op=True)
                    if correct:
                        nat.check(nat.cg_reg_prepare(h, sp, _ptr(psi), _ptr(scan), _ptr(ones), S))
                        correct = 2
                    work.wait()
                nat.check(nat.cg_obj_dir2(h, sp, first, _ptr(scan), _ptr(probe), op_dpsi, _ptr(data), _ptr(grad),
                                          _ptr(grad0), _ptr(dpsi), S))
                if share:
                    correct = 3
                line_search(0, 1, S)
                nat.check(nat.cg_obj_finish(h, sp, correct, _ptr(psi), _ptr(dpsi), _ptr(scan), _ptr(ones),
                                            _ptr(vt), _ptr(lz), nc, 150, 100.0, S))
                # 2) probe step (ptycho.py:409-465)
                if recover_prb:
                    nat.check(nat.cg_prb_grad(h, sp, _ptr(psi), _ptr(scan), _ptr(probe), _ptr(data), _ptr(gprb), S))
                    if dist_on:
                        self._allreduce(gprb)
                    nat.check(nat.cg_prb_dir(h, sp, first, nscan_total, 1.0, _ptr(psi), _ptr(scan), _ptr(data),
                                             _ptr(gprb), _ptr(gprb0), _ptr(dprb), S))
                    line_search(1, 0, S)
                    nat.check(nat.cg_prb_finish(h, sp, _ptr(probe), _ptr(dprb), S))

            self._log_header()
            try:
                for i in range(piter):
                    iteration(int(i == 0), int(i > 0))
                    if i % self.log_every == 0:
                        self._log_state(i, st)
            finally:
                # the native loop moved scan behind torch's back: forget what the operator calls knew about it
                self._scan_key = self._scan_trusted = None
                nat.check(nat.set_option(self._h, b"trust_order", 0))
        self._replay_ls_failures(st)
        return self._result(psi, probe, None)

    def _run_fused(self, data, psi, scan, probe, piter, recover_prb):
        """``CGPtychoSolver.run`` (ptycho.py:283-488) for one probe mode and the gaussian or
        poisson_ml model (option "model" of the handle), with every farplane-sized elementwise stage fused into the DFT row pass
        (C ABI ``ptycho_cg_*``).  Work buffer 0 holds the column pass of fwd(psi), which
        is shared by the intensity statistics, the gradient projection and the line
        search (the probe rescale ``a/b`` is linear and applied on the fly)."""
        dev = data.device
        data, psi = self._cg_operands(data, psi, scan, probe, contiguous=(probe,))
        nscan_total = self._nscan_total()
        sums = torch.zeros(2, dtype=torch.float64, device=dev)
        cost = torch.zeros(1, dtype=torch.float64, device=dev)
        costs = torch.zeros(33, dtype=torch.float64, device=dev)
        dpsi = gradpsi0 = None
        dprb = gradprb0 = None
        gammaprb = 0
        self._log_header()
        for i in range(piter):
            # 1) object step ----------------------------------------------------------
            self._cg_fwd_cols(0, psi, scan, probe[:, 0])
            sums.zero_()
            nat.check(nat.cg_stats(self._h, 0, _ptr(data), _ptr(sums), _stream()))
            self._allreduce(sums)
            ab32 = sums.to(torch.float32)
            probe *= (ab32[0] / ab32[1])                                    # :344
            cost.zero_()
            nat.check(nat.cg_project(self._h, 0, 1, _ptr(data), _ptr(sums), _ptr(cost), _stream()))
            gradpsi = torch.zeros((self.ptheta, self.nz, self.n), dtype=torch.complex64, device=dev)
            nat.check(nat.cg_adj_cols(self._h, 1, _ptr(gradpsi), _ptr(scan), _ptr(probe[:, 0]), 0, _stream()))
            gradpsi /= (torch.max(torch.abs(probe[:, 0])) ** 2)
            self._allreduce(gradpsi)
            dpsi = _dy_direction(i, gradpsi, gradpsi0, dpsi)
            gradpsi0 = gradpsi
            self._cg_fwd_cols(1, dpsi, scan, probe[:, 0])
            gammapsi = 0.5 * self._fused_line_search(data, sums, costs)

            if i > 0:                                                       # :398-403
                scan[0, :] += self._position_shifts(psi, dpsi, gammapsi, scan, probe).to(scan.dtype)
            psi = psi + gammapsi * dpsi

            # 2) probe step ------------------------------------------------------------
            if recover_prb:
                if i == 0:
                    gradprb0 = probe * 0
                    dprb = probe * 0
                cost2 = torch.zeros(1, dtype=torch.float64, device=dev)
                self._cg_fwd_cols(0, psi, scan, probe[:, 0])
                nat.check(nat.cg_project(self._h, 0, 1, _ptr(data), None, _ptr(cost2), _stream()))
                g = torch.zeros((self.ptheta, self.nprb, self.nprb), dtype=torch.complex64, device=dev)
                nat.check(nat.cg_adj_cols(self._h, 1, _ptr(psi), _ptr(scan), _ptr(g), 1, _stream()))
                self._allreduce(g)
                gradprb = (g / torch.max(torch.abs(psi)) ** 2 / nscan_total * 1)[:, None]
                dprb = _dy_direction(i, gradprb, gradprb0, dprb)
                gradprb0 = gradprb
                self._cg_fwd_cols(1, psi, scan, dprb[:, 0].contiguous())
                gammaprb = 0.5 * self._fused_line_search(data, None, costs, which="prb")
                probe[:, 0] = probe[:, 0] + gammaprb * dprb[:, 0]

            if i % self.log_every == 0:
                c = cost.clone()
                self._allreduce(c)
                self._log(i, float(gammapsi), float(gammaprb), float(c.to(torch.float32)))
        return self._result(psi, probe, None)

    def _run_fused_multi(self, data, psi, scan, probe, piter, recover_prb, model="gaussian", ortho=False):
        """``CGPtychoSolver.run`` (ptycho.py:283-488), gaussian or poisson_ml model (option "model" of the handle),
        2..8 incoherent probe modes.

        Work slots (one farplane each), compact layout: slot k holds the column pass of
        fwd(psi, probe_k) -- made once per step for all modes by ONE launch that gathers the object
        patch once per position (C ABI ``ptycho_cg_fwd_cols_modes``; the reference gathers per mode,
        ptycho.py:330-333) and shared by the intensity sum, the projection and the line search (the
        probe rescale a/b is linear and applied on the fly) -- and ONE further slot M is shared by all
        modes: projected residual of one mode at a time, direction column passes.  The summed intensity
        is a float32 array written once (no per-mode farplane is ever materialised); the object line
        search, which needs fwd(dpsi, probe_k) of every mode at once, runs over M position ranges with
        the M direction column passes of a range side by side in the shared slot: M + 1 farplanes instead
        of 2 M, same work.

        Device resident since round 3: a, b, the line-search costs and the accepted step lengths stay in the float64
        state vector of the native stages; every search is enqueued in full (passes of <= 16, 16, 32, 64 step lengths,
        ``ptycho_cg_ls_obj_chunk / ls_prb_pass / ls_decide``: passes after the deciding one return at once, their column
        passes included) and the host reads the state back only when it logs."""
        dev = data.device
        M = probe.shape[1]
        data, psi = self._cg_operands(data, psi, scan, probe)
        with self._options((b"compact_modes", M, 0)):
            self._scan_key = None                   # the position order becomes chunk-major: sort again
            nscan_total = self._nscan_total()
            st = self._state(dev)
            sp = _ptr(st)
            sums = st[nat.ST_A:nat.ST_A + 2]                    # a, b (views of the state vector)
            cost = st[nat.ST_COST:nat.ST_COST + 1]
            scratch_cost = st[nat.ST_COST2:nat.ST_COST2 + 1]
            costs = st[nat.ST_COSTS:nat.ST_COSTS + nat.ST_NCOSTS]
            gpsi_w = st[nat.ST_GAMMA_PSI:nat.ST_GAMMA_PSI + 1]
            gprb_w = st[nat.ST_GAMMA_PRB:nat.ST_GAMMA_PRB + 1]
            dist_on = self.group is not None
            inten = torch.empty_like(data)
            mode = lambda arr, k: arr[:, k].contiguous()
            A = lambda k: k              # column pass of fwd(psi, probe_k)
            B = M                        # shared: residual of one mode, then column passes of fwd(direction, .)
            vpp = ctypes.c_void_p * M
            prb_scale = M if model == "gaussian" else 1   # ptycho.py:431 (gaussian) / :441 (poisson)

            def mode_ptrs(modes):
                keep = [mode(modes, k) for k in range(M)]
                return keep, vpp(*[t.data_ptr() for t in keep])

            def fwd_cols_all(obj, modes):           # one launch per <= 4 modes, shared patch gather
                self._note_scan(scan)
                keep, ptrs = mode_ptrs(modes)
                nat.check(nat.cg_fwd_cols_modes(self._h, M, 0, _ptr(obj), _ptr(scan), ptrs, 0, 0, _stream()))

            def sum_intensity(stats=None):          # inten = sum_k |slot A(k)|^2 (+ a, b of :342-343) in one pass
                nat.check(nat.cg_intensity_modes(self._h, M, _ptr(inten), _ptr(data),
                                                 _ptr(stats) if stats is not None else None, _stream()))

            def object_line_search():
                """ptycho.py:383-393 for all modes, chunk by chunk; t1_k = (a/b) * slot A(k) (old probe), t2_k = column
                pass of fwd(dpsi, probe_k) (rescaled probe) in part k of the shared slot; 0.5 * step -> state[GAMMA_PSI]."""
                self._note_scan(scan)
                keep, ptrs = mode_ptrs(probe)
                S = _stream()
                nat.check(nat.cg_ls_begin(self._h, sp, 0, S))
                for nxt in LS_MULTI_GROUPS:
                    for c in range(M):
                        nat.check(nat.cg_ls_obj_chunk(self._h, sp, c, _ptr(dpsi), _ptr(scan), ptrs, _ptr(data), _ptr(sums), S))
                    if dist_on:
                        self._allreduce(costs)
                    nat.check(nat.cg_ls_decide(self._h, sp, 0, nxt, S))

            def probe_line_search(m):
                """ptycho.py:451-461: p1 = summed intensity, p2 = |fwd(psi, dprb_m)|^2, p3 = 2 Re(fwd(psi, probe_m) conj(.))."""
                S = _stream()
                nat.check(nat.cg_ls_begin(self._h, sp, 1, S))
                for nxt in LS_MULTI_GROUPS:
                    nat.check(nat.cg_ls_prb_pass(self._h, sp, m, _ptr(data), _ptr(inten), S))
                    if dist_on:
                        self._allreduce(costs)
                    nat.check(nat.cg_ls_decide(self._h, sp, 1, nxt, S))

            dpsi = gradpsi0 = None
            dprb = gradprb0 = gradprb = None
            powers = None
            self._log_header()
            try:
                for i in range(piter):
                    # 1) object step ------------------------------------------------------------
                    fwd_cols_all(psi, probe)                                            # :329-333
                    sums.zero_()
                    sum_intensity(sums)
                    self._allreduce(sums)
                    ab32 = sums.to(torch.float32)
                    probe *= (ab32[0] / ab32[1])                                        # :344
                    gradpsi = torch.zeros((self.ptheta, self.nz, self.n), dtype=torch.complex64, device=dev)
                    cost.zero_()
                    for k in range(M):                                                  # :349-356
                        pk = mode(probe, k)
                        # slot A(k) was made with the probe before its rescale: fpsi = (g s)(1/s)
                        scratch_cost.zero_()
                        nat.check(nat.cg_project_multi(self._h, A(k), B, _ptr(data), _ptr(inten), _ptr(sums), 1,
                                                       _ptr(cost if k == 0 else scratch_cost), _stream()))
                        g = torch.zeros_like(gradpsi)
                        nat.check(nat.cg_adj_cols(self._h, B, _ptr(g), _ptr(scan), _ptr(pk), 0, _stream()))
                        gradpsi += g / (torch.max(torch.abs(pk)) ** 2)
                    self._allreduce(gradpsi)
                    dpsi = _dy_direction(i, gradpsi, gradpsi0, dpsi)
                    gradpsi0 = gradpsi
                    object_line_search()                                                # :383-393 -> state[GAMMA_PSI]
                    gamma32 = gpsi_w.to(torch.float32)

                    if i > 0:                                                           # :398-403
                        scan[0, :] += self._position_shifts(psi, dpsi, gpsi_w, scan, probe).to(scan.dtype)
                    psi = psi + gamma32 * dpsi

                    # 2) probe step, one mode at a time ------------------------------------------
                    if recover_prb:                                                     # :409-465
                        if i == 0:
                            gradprb = probe * 0
                            gradprb0 = probe * 0
                            dprb = probe * 0
                        for m in range(M):
                            # slots A(k) = fwd(psi, probe_k) for the current psi and probes: all of them
                            # after the object step, then only the mode that was just updated
                            if m == 0:
                                fwd_cols_all(psi, probe)
                            else:
                                self._cg_fwd_cols(A(m - 1), psi, scan, mode(probe, m - 1))
                            sum_intensity()                                             # absfprb (= p1 below)
                            scratch_cost.zero_()
                            nat.check(nat.cg_project_multi(self._h, A(m), B, _ptr(data), _ptr(inten), None, 0,
                                                           _ptr(scratch_cost), _stream()))
                            g = torch.zeros((self.ptheta, self.nprb, self.nprb), dtype=torch.complex64, device=dev)
                            nat.check(nat.cg_adj_cols(self._h, B, _ptr(psi), _ptr(scan), _ptr(g), 1, _stream()))
                            self._allreduce(g)
                            gradprb[:, m] = g / torch.max(torch.abs(psi)) ** 2 / nscan_total * prb_scale
                            dprb[:, m] = _dy_direction(i, gradprb[:, m], gradprb0[:, m], dprb[:, m])
                            gradprb0[:, m] = gradprb[:, m]
                            self._cg_fwd_cols(B, psi, scan, mode(dprb, m))
                            probe_line_search(m)                                        # -> state[GAMMA_PRB]
                            probe[:, m] = probe[:, m] + gprb_w.to(torch.float32) * dprb[:, m]
                        if ortho:                                                       # ortho_prb
                            powers = orthogonalize_modes(probe, dprb, gradprb0)

                    if i % self.log_every == 0:
                        self._log_state(i, st)
            finally:
                self._scan_key = None
        self._replay_ls_failures(st)
        return self._result(psi, probe, powers)
