"""The torch array shim and ``PtychoHIP``: the forward / adjoint operators behind ``libptychohip.so`` and their host batching."""
import contextlib
import ctypes

import numpy as np
import torch

from . import _native as nat
from .autograd import FwdFunction


class TorchArrayModule:
    """Minimal ``array_module`` hook (``ptycho.py:55`` of the reference exposes
    ``cp``): what a host framework needs to create device arrays."""
    complex64, float32, float64 = torch.complex64, torch.float32, torch.float64

    @staticmethod
    def _dev():
        return torch.device("cuda", torch.cuda.current_device())

    @classmethod
    def asarray(cls, x, dtype=None):
        if isinstance(x, torch.Tensor):
            return x.to(device=cls._dev(), dtype=dtype) if dtype else x.to(cls._dev())
        return torch.as_tensor(np.ascontiguousarray(x), dtype=dtype, device=cls._dev())

    array = asarray

    @classmethod
    def zeros(cls, shape, dtype=torch.float32):
        return torch.zeros(tuple(shape), dtype=_tdtype(dtype), device=cls._dev())

    @classmethod
    def ones(cls, shape, dtype=torch.float32):
        return torch.ones(tuple(shape), dtype=_tdtype(dtype), device=cls._dev())

    @classmethod
    def empty(cls, shape, dtype=torch.float32):
        return torch.empty(tuple(shape), dtype=_tdtype(dtype), device=cls._dev())


def _tdtype(d):
    if isinstance(d, torch.dtype):
        return d
    return {"complex64": torch.complex64, "float32": torch.float32,
            "float64": torch.float64, "complex128": torch.complex128}[np.dtype(d).name]


def _asnumpy(x):
    return x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr())


class PtychoHIP:
    """Forward / adjoint ptychography operators (``PtychoCuFFT`` of the
    reference, ``ptycho.py:34-162``).

    Attributes
    ----------
    nscan : int   scan positions per angular view
    nprb : int    probe is ``nprb x nprb``
    ndet : int    detector is ``ndet x ndet`` (2..1024, or a power of two up to 2048; powers of two
                  run the fused kernels, other sizes a Bluestein transform)
    ptheta : int  angular views processed per call
    n, nz : int   object width, height
    """

    array_module = TorchArrayModule
    asnumpy = staticmethod(_asnumpy)

    def __init__(self, nscan, probe_shape, detector_shape, ntheta, nz, n):
        # argument order of ptycho.py:58-60 -> native (ptheta, nz, n, nscan, ndet, nprb)
        if not torch.cuda.is_available():
            raise RuntimeError("libtike.hipfft needs a ROCm GPU; there is no CPU path")
        self._h = ctypes.c_void_p()
        nat.check(nat.create(ctypes.byref(self._h), ntheta, nz, n, nscan, detector_shape, probe_shape))
        self._device = torch.device("cuda", torch.cuda.current_device())
        self._det = False      # option "deterministic" as set by set_deterministic()

    # read-only size attributes of the native object (swig/ptychofft.i:11-16)
    ptheta = property(lambda self: int(nat.get(self._h, 0)))
    nz = property(lambda self: int(nat.get(self._h, 1)))
    n = property(lambda self: int(nat.get(self._h, 2)))
    nscan = property(lambda self: int(nat.get(self._h, 3)))
    ndet = property(lambda self: int(nat.get(self._h, 4)))
    nprb = property(lambda self: int(nat.get(self._h, 5)))
    _slot_allocated = lambda self, slot: nat.get(self._h, nat.GET_WORK_SLOT0 + slot) == 1  # noqa: E731  (CG work slot holds memory?)

    def __enter__(self):
        return self

    def __exit__(self, type, value, traceback):
        self.free()

    def __del__(self):
        h = getattr(self, "_h", None)
        if h is not None and h.value:
            try:
                nat.destroy(h)
            except Exception:
                pass
            self._h = None

    def free(self):
        """Release device scratch; idempotent (``ptychofft.cu:49-57``)."""
        if self._h is not None and self._h.value:
            nat.check(nat.free(self._h))

    def set_chunk(self, positions):
        """Positions per launch pair of the adjoint (0 = default: at most 4 GiB of scratch)."""
        nat.check(nat.set_option(self._h, b"chunk", int(positions)))

    def set_window(self, on=True):
        """Object adjoint: LDS overlap-add window (default) or direct atomics."""
        nat.check(nat.set_option(self._h, b"window", int(bool(on))))

    def set_split(self, on=True):
        """ndet = 256: split the DFT over y between the column and the row pass (default on)."""
        nat.check(nat.set_option(self._h, b"split", int(bool(on))))

    def set_tile(self, on=True):
        """ndet <= 128: forward operator and probe adjoint as one launch each, the tile stays in the compute unit's
        LDS (default on); off = the two-pass kernels of the larger sizes."""
        nat.check(nat.set_option(self._h, b"tile", int(bool(on))))

    def set_deterministic(self, on=True):
        """Adjoints accumulate in 64-bit fixed point (integer atomics): bitwise reproducible results
        (the reference's float ``atomicAdd``, kernels.cu:73-80,92-93, is not).  ndet <= 512."""
        nat.check(nat.set_option(self._h, b"deterministic", int(bool(on))))
        self._det = bool(on)

    def release_scratch(self):
        """Free the adjoint's intermediate (up to 4 GiB; ``adj`` allocates it again when needed): the fused CG loops never use it."""
        nat.check(nat.set_option(self._h, b"release_scratch", 1))

    def release_work(self, slot):
        """Free one farplane-sized CG work slot (the next stage that writes it allocates it again).  The native loop holds
        slots 0-3 when the position correction shares the object step's patch gathers, 0-1 (+2 with a process group) without."""
        nat.check(nat.set_option(self._h, b"release_work", int(slot)))

    def work_slots_allocated(self):
        """Indices of the CG work slots that currently hold device memory (``ptheta * nscan * ndet^2 * 8`` bytes each)."""
        return [s for s in range(16) if self._slot_allocated(s)]

    def set_fused(self, tiles=2):
        """ndet = 256: forward operator as one launch (``k_fwd_fused256``), ``tiles`` = 0 (off), 1 or 2."""
        nat.check(nat.set_option(self._h, b"fused", int(tiles)))

    def profile(self, enable=True):
        """Bracket every kernel launch with HIP events (bench.py's live timing)."""
        nat.check(nat.profile(self._h, int(bool(enable))))

    def profile_read(self):
        """``{kernel: (total_ms, launches)}`` since the last read; waits for them."""
        nk = len(nat.KERNEL_NAMES)
        ms = (ctypes.c_double * nk)()
        cnt = (ctypes.c_longlong * nk)()
        nat.check(nat.profile_read(self._h, ms, cnt, nk))
        return {k: (ms[i], int(cnt[i])) for i, k in enumerate(nat.KERNEL_NAMES) if cnt[i]}

    def _operand(self, x, dtype, shape, name):
        assert x.dtype == dtype, f"{name}: {x.dtype}"
        if not x.is_cuda:
            raise ValueError(f"{name} must be a device tensor")
        if tuple(x.shape) != tuple(shape):
            raise ValueError(f"{name}: shape {tuple(x.shape)} != expected {tuple(shape)}")
        return x if x.is_contiguous() else x.contiguous()

    def _note_scan(self, scan):
        """Tell the native side whether ``scan`` is the tensor (same storage, same torch
        version counter) the previous operator call sorted; if so the sort is reused."""
        key = (scan.data_ptr(), scan._version, tuple(scan.shape))
        same = getattr(self, "_scan_key", None) == key
        if same != getattr(self, "_scan_trusted", False):
            nat.check(nat.set_option(self._h, b"trust_order", int(same)))
            self._scan_trusted = same
        self._scan_key = key

    def _stockham_size(self):
        """The fused CG stages run on the detector sizes that have a Stockham plan of their own (csrc/fft_core.hpp): powers
        of two and 48, 80, 96, 112, 192 (112 = the reference's own crop, tests/test_fsc.py:115-120); any other size: Bluestein
        operators + the statement-by-statement loop of ``run``."""
        return (self.ndet >= 16 and (self.ndet & (self.ndet - 1)) == 0) or self.ndet in (48, 80, 96, 112, 192)

    @contextlib.contextmanager
    def _options(self, *settings, mask=None):
        """Handle state for one run: every ``(name, value, restore)`` of ``settings`` is set on entry and, however the run ends,
        put back to ``restore`` in the order given; ``mask`` (uint8 device tensor) goes on the handle, where the fused / native
        loops read it, and comes off again."""
        try:
            if mask is not None and self._stockham_size():
                nat.check(nat.set_mask(self._h, _ptr(mask), _stream()))
            for name, value, _ in settings:
                nat.check(nat.set_option(self._h, name, value))
            yield
        finally:
            if mask is not None:
                nat.check(nat.set_mask(self._h, None, None))
            for name, _, restore in settings:
                nat.check(nat.set_option(self._h, name, restore))

    # -- operators (ptycho.py:80-123) ---------------------------------------
    def fwd(self, psi, scan, probe, out=None):
        """Ptychography transform (FQ).  ``out``: optional farplane tensor to write into (the reference
        allocates a fresh one per call, ptycho.py:85-86)."""
        psi = self._operand(psi, torch.complex64, (self.ptheta, self.nz, self.n), "psi")
        scan = self._operand(scan, torch.float32, (self.ptheta, self.nscan, 2), "scan")
        probe = self._operand(probe, torch.complex64, (self.ptheta, self.nprb, self.nprb), "probe")
        if out is None:
            farplane = torch.empty((self.ptheta, self.nscan, self.ndet, self.ndet), dtype=torch.complex64, device=psi.device)
        else:
            farplane = self._operand(out, torch.complex64, (self.ptheta, self.nscan, self.ndet, self.ndet), "out")
            assert farplane is out, "out must be contiguous"
        self._note_scan(scan)
        nat.check(nat.fwd(self._h, _ptr(farplane), _ptr(psi), _ptr(scan), _ptr(probe), _stream()))
        return farplane

    def adj(self, farplane, scan, probe, out=None):
        """Adjoint ptychography transform (Q*F*).  ``out``: optional object tensor (zeroed here, ptycho.py:102)."""
        farplane = self._operand(farplane, torch.complex64, (self.ptheta, self.nscan, self.ndet, self.ndet), "farplane")
        scan = self._operand(scan, torch.float32, (self.ptheta, self.nscan, 2), "scan")
        probe = self._operand(probe, torch.complex64, (self.ptheta, self.nprb, self.nprb), "probe")
        if out is None:
            psi = torch.zeros((self.ptheta, self.nz, self.n), dtype=torch.complex64, device=farplane.device)
        else:
            psi = self._operand(out, torch.complex64, (self.ptheta, self.nz, self.n), "out")
            assert psi is out, "out must be contiguous"
            psi.zero_()
        self._note_scan(scan)
        nat.check(nat.adj(self._h, _ptr(psi), _ptr(farplane), _ptr(scan), _ptr(probe), 0, _stream()))
        return psi

    def adj_probe(self, farplane, scan, psi):
        """Adjoint ptychography probe transform (O*F*), object is fixed."""
        farplane = self._operand(farplane, torch.complex64, (self.ptheta, self.nscan, self.ndet, self.ndet), "farplane")
        scan = self._operand(scan, torch.float32, (self.ptheta, self.nscan, 2), "scan")
        psi = self._operand(psi, torch.complex64, (self.ptheta, self.nz, self.n), "psi")
        probe = torch.zeros((self.ptheta, self.nprb, self.nprb), dtype=torch.complex64, device=farplane.device)
        self._note_scan(scan)
        nat.check(nat.adj(self._h, _ptr(psi), _ptr(farplane), _ptr(scan), _ptr(probe), 1, _stream()))
        return probe

    def adj_scan(self, farplane, scan, psi, probe, out=None, chunk=None):
        """Scan-position gradient: float32 ``[ptheta, nscan, 2]``, the derivative of ``Re <farplane, fwd(psi, scan, probe)>``
        with respect to ``scan`` with ``farplane`` held fixed, inside the interpolation cell of every position (at an
        integer coordinate: of the cell that the truncation selects).  Skipped positions (integer part < 0) give 0.0.

        ``out``: optional result tensor, every element is written.  ``chunk``: positions per inverse transform; the work
        buffer (``chunk`` detector tiles, from torch's allocator) is at most 256 MiB when ``chunk`` is ``None``.  The result
        does not depend on ``chunk``, and two calls give the same bits."""
        farplane = self._operand(farplane, torch.complex64, (self.ptheta, self.nscan, self.ndet, self.ndet), "farplane")
        scan = self._operand(scan, torch.float32, (self.ptheta, self.nscan, 2), "scan")
        psi = self._operand(psi, torch.complex64, (self.ptheta, self.nz, self.n), "psi")
        probe = self._operand(probe, torch.complex64, (self.ptheta, self.nprb, self.nprb), "probe")
        if out is None:
            grad = torch.empty((self.ptheta, self.nscan, 2), dtype=torch.float32, device=farplane.device)
        else:
            grad = self._operand(out, torch.float32, (self.ptheta, self.nscan, 2), "out")
            assert grad is out, "out must be contiguous"
        total = self.ptheta * self.nscan
        if chunk is None:
            chunk = max(1, (256 << 20) // (self.ndet * self.ndet * 8))
        elif int(chunk) < 1:
            raise ValueError("chunk must be at least 1, got %r" % (chunk,))
        chunk = min(int(chunk), total)
        work = torch.empty((chunk, self.ndet, self.ndet), dtype=torch.complex64, device=farplane.device)
        self._note_scan(scan)
        nat.check(nat.adj_scan(self._h, _ptr(grad), _ptr(farplane), _ptr(psi), _ptr(scan), _ptr(probe), _ptr(work), chunk,
                               _stream()))
        return grad

    def fwd_autograd(self, psi, scan, probe):
        """``fwd`` with a ``torch.autograd`` graph: the same arguments and the same result bits; ``backward`` gives the
        gradients of a real loss for ``psi`` (``adj``), ``probe`` (``adj_probe``) and ``scan`` (``adj_scan``, float32),
        only those that require one.  Several probe modes: sum the intensities of ``fwd_autograd(psi, scan, probe[:, k])``;
        autograd adds the gradients up."""
        return FwdFunction.apply(self, psi, scan, probe)

    def fft2(self, x, inverse=False, out=None):
        """Unnormalised batched 2-D DFT of ``[..., ndet, ndet]`` complex64 tiles
        (the cuFFT plan of ``ptychofft.cu:14-20``)."""
        assert x.dtype == torch.complex64 and x.shape[-1] == x.shape[-2] == self.ndet
        x = x.contiguous()
        out = torch.empty_like(x) if out is None else out
        nb = x.numel() // (self.ndet * self.ndet)
        nat.check(nat.fft2(self._h, _ptr(out), _ptr(x), nb, 1 if inverse else -1, _stream()))
        return out

    def residuals(self, data, psi, scan, probe, mask=None, rescale=False):
        """How well ``(psi, scan, probe)`` explains ``data``, per frame and per detector pixel (``libtike.hipfft.fit``).

        ``probe``: ``[ptheta, M, nprb, nprb]`` or ``[ptheta, nprb, nprb]``, any ``M >= 1``; any detector size of the
        operators.  One farplane is reused for every mode: ``fwd`` into it, ``accumulate_intensity`` for all modes but the
        last, then ``fit_frames``.  ``rescale=True`` reports the fit as the next CG iteration would see it: a first pass
        gives ``a = sum sqrt(I d)`` and ``b = sum I`` on the device, a second pass prices ``I (a / b)^2``.

        Returns the ``fit_frames`` dict (``"frames"``, ``"pixels"``) plus, per frame ``[ptheta, nscan]``,
        ``"cost_gaussian"``, ``"cost_poisson"``, ``"deviance"``, ``"r_factor"`` and ``"flux_ratio"`` (data over model),
        and ``"scale"``: ``a / b`` of the unscaled intensity, a 0-dim float64 device tensor.  The inputs are not modified;
        nothing synchronises.  With a process group the frames are this rank's shard and ``rescale=True`` raises
        ``NotImplementedError`` (``a`` and ``b`` would have to be summed over the ranks).
        """
        from .fit import accumulate_intensity, check_fit_frames, fit_frames   # fit imports this module
        if rescale and getattr(self, "group", None) is not None:
            raise NotImplementedError("residuals(rescale=True) on a solver with a process group")
        if probe.dim() == 3:
            probe = probe[:, None]
        if probe.dim() != 4 or probe.shape[1] < 1:
            raise ValueError("probe must be [ptheta, M, nprb, nprb] or [ptheta, nprb, nprb], got %s" % (tuple(probe.shape),))
        shape = (self.ptheta, self.nscan, self.ndet, self.ndet)
        data = self._operand(data, torch.float32, shape, "data")
        nmodes = probe.shape[1]
        farplane = torch.empty(shape, dtype=torch.complex64, device=data.device)
        check_fit_frames(data, farplane, None, mask)
        inten = None
        for m in range(nmodes):
            self.fwd(psi, scan, probe[:, m], out=farplane)
            if m + 1 < nmodes:
                inten = accumulate_intensity(farplane, out=inten)
        fit = fit_frames(data, farplane, inten, mask, None, pixels=not rescale)
        f = fit["frames"]
        scale = f[..., 2].sum() / f[..., 0].sum()
        if rescale:
            fit = fit_frames(data, farplane, inten, mask, torch.stack((f[..., 2].sum(), f[..., 0].sum())))
            f = fit["frames"]
        fit.update(cost_gaussian=f[..., 3], cost_poisson=f[..., 4], deviance=2.0 * (f[..., 4] - f[..., 5]),
                   r_factor=f[..., 6] / f[..., 7], flux_ratio=f[..., 1] / f[..., 0], scale=scale)
        return fit

    # -- host batching (ptycho.py:70-78, 91-95, 108-111, 125-129) -----------
    def _batch(self, function, output, *inputs):
        """NumPy in / NumPy out, one angular partition of ``ptheta`` views at a
        time (the reference uploads slices of length 1, which is only right for
        ``ptheta == 1``; here the slice length is ``ptheta``)."""
        xp = self.array_module
        step = self.ptheta
        for ids in range(0, inputs[0].shape[0] - step + 1, step):
            dev = [xp.asarray(x[ids:ids + step]) for x in inputs]
            # device -> final host memory in one copy (no intermediate host tensor)
            torch.from_numpy(output[ids:ids + step]).copy_(function(*dev))
        return output

    def fwd_ptycho_batch(self, psi, scan, probe):
        data = np.zeros([scan.shape[0], self.nscan, self.ndet, self.ndet], dtype="complex64")
        return self._batch(self.fwd, data, psi, scan, _single_mode(probe))

    def adj_ptycho_batch(self, farplane, scan, probe):
        psi = np.zeros([scan.shape[0], self.nz, self.n], dtype="complex64")
        return self._batch(self.adj, psi, farplane, scan, _single_mode(probe))

    def adj_ptycho_batch_prb(self, farplane, scan, psi):
        probe = np.zeros([scan.shape[0], self.nprb, self.nprb], dtype="complex64")
        return self._batch(self.adj_probe, probe, farplane, scan, psi)

    def run(self, data, psi, scan, probe, **kwargs):
        raise NotImplementedError("Cannot run a base class.")

    def run_batch(self, data, psi, scan, probe, angle_shard=None, **kwargs):
        """Run by dividing the work into angular partitions (``ptycho.py:135-162``).
        NumPy in / NumPy out; ``scan`` updates are not returned and remainder angles are
        dropped, as in the reference.

        The reference uploads, solves and downloads one partition at a time, fully
        synchronously.  Here the next partition's ``data / psi / scan / probe`` are staged
        through two reused sets of pinned buffers by a worker thread and copied on a copy
        stream while the current partition is being solved (angle streaming).  Angle partitions are independent problems, so a
        multi-GPU job gives every rank its own partitions with no collective:
        ``angle_shard=(rank, world)`` restricts this call to partitions ``rank, rank+world, ...``
        (the other entries of the returned arrays keep their input values).
        """
        assert probe.ndim == 4, "probe needs 4 dimensions, not %d" % probe.ndim
        import threading
        psi = psi.copy()
        probe = probe.copy()
        nparts = scan.shape[0] // self.ptheta
        rank, world = angle_shard if angle_shard is not None else (0, 1)
        mine = list(range(nparts))[rank::world]
        dev = self._device
        copy_stream = torch.cuda.Stream(device=dev)
        arrays = (data, psi, scan, probe)
        # two sets of pinned staging buffers, filled by a worker thread while the main thread
        # drives the solver (the pinned copy of 1 GiB of data takes longer than its DMA)
        pinned = [[torch.empty((self.ptheta,) + x.shape[1:], dtype=torch.from_numpy(x[:0]).dtype).pin_memory()
                   for x in arrays] for _ in range(min(2, len(mine)))]
        done = [None, None]                       # H2D-complete events of the two sets

        def stage(n, box):
            k = mine[n]
            ids = slice(k * self.ptheta, (k + 1) * self.ptheta)
            bufs = pinned[n % 2]
            if done[n % 2] is not None:
                done[n % 2].synchronize()         # the DMA out of this set (partition n-2) is over
            for b, x in zip(bufs, arrays):
                b.copy_(torch.from_numpy(np.ascontiguousarray(x[ids])))
            with torch.cuda.stream(copy_stream):
                t = [b.to(dev, non_blocking=True) for b in bufs]
                ev = torch.cuda.Event()
                ev.record(copy_stream)
            done[n % 2] = ev
            box.append((ids, t, ev))

        def start(n):
            box = []
            th = threading.Thread(target=stage, args=(n, box), daemon=True)
            th.start()
            return th, box

        pending = start(0) if mine else None
        for n in range(len(mine)):
            th, box = pending
            th.join()
            ids, (d_gpu, psi_gpu, scan_gpu, prb_gpu), ev = box[0]
            torch.cuda.current_stream().wait_event(ev)
            for t in (d_gpu, psi_gpu, scan_gpu, prb_gpu):
                t.record_stream(torch.cuda.current_stream())
            pending = start(n + 1) if n + 1 < len(mine) else None
            result = self.run(d_gpu, psi_gpu, scan_gpu, prb_gpu, **kwargs)
            psi[ids] = self.asnumpy(result["psi"])
            probe[ids] = self.asnumpy(result["probe"])
        return {"psi": psi, "probe": probe}


def _single_mode(probe):
    """The ``*_batch`` wrappers accept a ``[ntheta,1,nprb,nprb]`` probe
    (``/root/reference/tests/test_adjoint.py:24,44``): the slice keeps its memory
    layout and the native side reads it as ``[ntheta,nprb,nprb]``."""
    probe = np.asarray(probe)
    if probe.ndim == 4:
        assert probe.shape[1] == 1, "the *_batch wrappers take one probe mode"
        return probe[:, 0]
    return probe


#: drop-in name of the reference class
PtychoCuFFT = PtychoHIP


def _dy_direction(i, grad, grad0, d):
    """Dai-Yuan direction with the reference's complex beta (ptycho.py:366-372)."""
    if i == 0:
        return -grad
    return -grad + (torch.linalg.norm(grad) ** 2 / (torch.sum(torch.conj(d) * (grad - grad0))) * d)
