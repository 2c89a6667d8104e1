"""A first look at a scan before any reconstruction, and a starting object taken from the data.

Every beamline shows the transmission (STXM), dark-field and differential-phase-contrast (DPC) images of a scan within
seconds of its end: one figure per diffraction pattern, spread over the object grid.  They need only ``data``, ``scan``
and a probe (``initial_probe`` gives one).  The zeroth moment of a pattern is the probe-weighted transmission of the
object at that position and its first moment is the probe-weighted phase gradient, so the same figures give an
object to start a reconstruction from: the gradient, integrated by least squares, is an *unwrapped* phase, because a
gradient has no ``2 pi`` ambiguity.

``frame_moments`` is the one pass over the data, ``scan_map`` spreads per-position values over the object with the
weights of ``illumination``, ``integrate_gradient`` is the solver of ``unwrap_phase`` fed with a gradient field instead
of a wrapped phase, ``first_look`` chains them and ``initial_object`` turns the result into ``psi``.  Everything runs on
the device on the current stream; only ``integrate_gradient`` synchronises (once per ``check_every`` iterations).
Kernels: ``csrc/k_dpc.hpp``, C ABI ``ptycho_frame_moments`` / ``ptycho_scan_map`` / ``ptycho_integrate_*``;
include/ptycho_hip.h and DESIGN.md section 18 state the definitions, tests/dpc_ref.py restates them in NumPy.  Bitwise
reproducible.

Under the solver's convention (unnormalised forward FFT, DC at ``[0, 0]``, ``scan[..., 0]`` the row) the phase gradient
in radians per pixel is ``(2 pi / ndet) (c - c0)``, with ``c`` the centre of mass of a pattern in signed frequency
indices (``np.fft.fftfreq(ndet) * ndet``) and ``c0`` the centre of the beam without an object.

What comes out is the object *blurred by the probe*: every figure is an average over the probe's footprint, weighted by
``|probe|^2``.  A detector mask biases both moments (the masked intensity is missing from the sums), so the
transmission comes out low and the gradient is pulled towards the measured side.
"""
import numbers

import numpy as np
import torch

from . import _native as nat
from ._args import _array, _check_out, _dtype, _need_array, _opt, _size, _to_device
from .gauge import check_illumination
from .operators import _ptr, _stream
from .unwrap import check_unwrap

__all__ = ["frame_moments", "scan_map", "integrate_gradient", "first_look", "initial_object", "check_frame_moments",
           "check_scan_map", "check_integrate", "check_first_look"]


# ---- argument checks (no device use) -------------------------------------------------------------------------------------
def _radius(darkfield):
    if darkfield is None:
        return -1.0
    if isinstance(darkfield, bool) or not isinstance(darkfield, numbers.Real) or not 0.0 <= float(darkfield) < float("inf"):
        raise ValueError("darkfield must be a finite radius >= 0 in frequency indices or None, got %r" % (darkfield,))
    return float(darkfield)


def check_frame_moments(data, mask=None, darkfield=None):
    """Validate ``frame_moments``'s arguments (no device use); returns ``(ptheta, nscan, ndet, radius)``."""
    shape = _array(data, "data", "float32", (4,))
    if shape[-1] != shape[-2]:
        raise ValueError("data must be [ptheta, nscan, ndet, ndet], got %s" % (shape,))
    if shape[2] > 46340 or not 1 <= shape[0] <= 65535:
        raise ValueError("data needs ndet <= 46340 and ptheta in [1, 65535], got shape %s" % (shape,))
    if mask is not None:
        _need_array(mask, "mask")
        if tuple(int(v) for v in mask.shape) != shape[-2:]:
            raise ValueError("mask must be %s, got shape %s" % (shape[-2:], tuple(mask.shape)))
    return shape[0], shape[1], shape[2], _radius(darkfield)


def check_scan_map(values, scan, probe, nz, n, keep=None):
    """Validate ``scan_map``'s arguments (no device use); returns ``(ptheta, nscan, nval, nmodes, nprb, nz, n)``."""
    ptheta, nscan, nmodes, nprb, nz, n = check_illumination(scan, probe, nz, n)
    vs = _array(values, "values", "float32", (2, 3))
    if vs[:2] != (ptheta, nscan):
        raise ValueError("values must be [ptheta, nscan] or [ptheta, nscan, nval] with scan's %s, got %s" % ((ptheta, nscan), vs))
    if keep is not None:
        _need_array(keep, "keep")
        if _dtype(keep) not in ("bool", "uint8"):
            raise TypeError("keep must be bool or uint8, got %s" % _dtype(keep))
        if tuple(int(v) for v in keep.shape) != (ptheta, nscan):
            raise ValueError("keep must be %s, got shape %s" % ((ptheta, nscan), tuple(keep.shape)))
    return ptheta, nscan, vs[2] if len(vs) == 3 else 1, nmodes, nprb, nz, n


def check_integrate(gy, gx, weight=None, tol=1e-4, maxiter=None, check_every=256, out=None):
    """Validate ``integrate_gradient``'s arguments (no device use); returns ``(ptheta, nz, n, maxiter)``."""
    shape = _array(gy, "gy", "float32", (2, 3))
    if _array(gx, "gx", "float32", (2, 3)) != shape:
        raise ValueError("gx must have gy's shape %s, got %s" % (shape, tuple(gx.shape)))
    return check_unwrap(gy, weight, True, tol, maxiter, check_every, out)


def check_first_look(data, scan, probe, nz, n, mask=None, reference="mean", keep=None, floor=0.05, darkfield=None,
                     tol=1e-4, maxiter=None):
    """Validate ``first_look``'s arguments (no device use); returns ``(ptheta, nscan, ndet, nz, n, reference)`` with
    ``reference`` ``None`` for ``"mean"`` or the pair as floats."""
    ptheta, nscan, ndet, _ = check_frame_moments(data, mask, darkfield)
    if check_scan_map(np.empty((ptheta, nscan), np.float32), scan, probe, nz, n, keep)[:2] != (ptheta, nscan):
        raise ValueError("data and scan differ in ptheta or nscan: %s and %s" % (tuple(data.shape), tuple(scan.shape)))
    if isinstance(reference, str):
        if reference != "mean":
            raise ValueError("reference must be 'mean' or a pair (cy, cx), got %r" % (reference,))
        ref = None
    else:
        try:
            ref = tuple(float(v) for v in reference)
        except (TypeError, ValueError):
            raise ValueError("reference must be 'mean' or a pair (cy, cx), got %r" % (reference,))
        if len(ref) != 2 or not all(np.isfinite(ref)):
            raise ValueError("reference must be 'mean' or a pair of finite numbers (cy, cx), got %r" % (reference,))
    if isinstance(floor, bool) or not isinstance(floor, numbers.Real) or not 0.0 <= float(floor) <= 1.0:
        raise ValueError("floor must be in [0, 1], got %r" % (floor,))
    if nz < 2 or n < 2 or nz * n >= 2 ** 31:
        raise ValueError("the object needs nz >= 2, n >= 2 and nz * n < 2^31, got %s" % ((nz, n),))
    check_unwrap(np.empty((2, 2), np.float32), None, True, tol, maxiter)
    return ptheta, nscan, ndet, int(nz), int(n), ref


_HOST = "operands must be device tensors or NumPy arrays"   # what a host tensor among the operands raises


# ---- the pieces ---------------------------------------------------------------------------------------------------------------
def frame_moments(data, mask=None, darkfield=None):
    """The moments of every diffraction pattern, in one pass over ``data``.

    ``data``: float32 ``[ptheta, nscan, ndet, ndet]`` with DC at ``[0, 0]`` (the solver's layout), a device tensor or a
    NumPy array, any ``ndet`` (odd included).  ``mask``: ``[ndet, ndet]``, nonzero = measured, shared by every frame; an
    unmeasured pixel enters no sum whatever ``data`` holds there (NaN and Inf included), a non-finite value at a measured
    pixel stays in its own frame.  ``darkfield``: a radius ``R`` in frequency indices, or ``None``.

    Returns a dict of device tensors: ``"moments"`` float64 ``[ptheta, nscan, 8]``, the sums over the measured pixels of
    ``I, k_y I, k_x I, k_y^2 I, k_x^2 I, k_y k_x I``, of ``I`` over the pixels with ``k_y^2 + k_x^2 > R^2`` (0 without
    ``darkfield``) and 0, with ``k`` the signed frequency index (``np.fft.fftfreq(ndet) * ndet``); ``"sum"`` (column 0),
    ``"center"`` ``[ptheta, nscan, 2]`` (columns 1 and 2 over column 0, NaN for an empty frame) and ``"darkfield"``
    (column 6).  Every term is formed and added in float64 in a fixed order.  Bitwise reproducible; two launches, no
    synchronisation.
    """
    ptheta, nscan, ndet, radius = check_frame_moments(data, mask, darkfield)
    if mask is not None and not isinstance(mask, torch.Tensor):
        mask = np.ascontiguousarray(np.asarray(mask) != 0)
    (d, m), dev = _to_device((data, mask), "dpc", _HOST)
    if m is not None:
        m = (m != 0).to(torch.uint8).contiguous()
    words = int(nat.frame_moments_work_words(ptheta, nscan, ndet))
    with torch.cuda.device(dev):
        mom = torch.empty((ptheta, nscan, 8), dtype=torch.float64, device=dev)
        work = torch.empty((max(words, 1),), dtype=torch.float64, device=dev)
        nat.check(nat.frame_moments(_ptr(mom), _ptr(d), _opt(m), radius, ptheta, nscan, ndet, _ptr(work), _stream()))
        total = mom[..., 0:1]
        center = torch.where(total != 0, mom[..., 1:3] / total, torch.full_like(total, float("nan")))
    return {"moments": mom, "sum": mom[..., 0], "center": center, "darkfield": mom[..., 6]}


def scan_map(values, scan, probe, nz, n, keep=None, normalize=True):
    """Spread per-position ``values`` over an ``nz x n`` object with the weights of ``illumination``.

    ``values``: float32 ``[ptheta, nscan, nval]`` (or ``[ptheta, nscan]``), any ``nval`` (four channels go into one
    call); ``scan``, ``probe``, ``nz``, ``n`` as for ``illumination``; ``keep``: bool or uint8 ``[ptheta, nscan]``, a zero
    entry excludes that position, e.g. ``~flag_frames(...)``.  Device tensors or NumPy arrays.

    Returns ``(weight, out)``: ``weight`` ``[ptheta, nz, n]`` is ``illumination`` of the kept positions, bit for bit, and
    ``out`` ``[ptheta, nval, nz, n]`` (``[ptheta, nz, n]`` for 2-D ``values``) is
    ``sum_j sum_ab (w_ab A) v_j / weight`` where ``weight > 0``, else 0: the average of the values of the positions
    that light a pixel, weighted by how much each lights it.  A position that the illumination skips or that ``keep``
    excludes adds to nothing, whatever its values hold.  ``normalize=False`` returns the sums themselves, not divided by
    the weight.  Positions in order, float32, no fused multiply-add: bitwise reproducible.  No synchronisation.
    """
    ptheta, nscan, nval, nmodes, nprb, nz, n = check_scan_map(values, scan, probe, nz, n, keep)
    if not isinstance(normalize, (bool, np.bool_)):
        raise TypeError("normalize must be a bool, got %r" % (normalize,))
    if keep is not None and not isinstance(keep, torch.Tensor):
        keep = np.ascontiguousarray(np.asarray(keep) != 0)
    (v, s, p, k), dev = _to_device((values, scan, probe, keep), "dpc", _HOST)
    v3 = v.reshape(ptheta, nscan, nval)
    if k is not None:
        k = (k != 0).to(torch.uint8).contiguous()
    with torch.cuda.device(dev):
        weight = torch.empty((ptheta, nz, n), dtype=torch.float32, device=dev)
        out = torch.empty((ptheta, nval, nz, n), dtype=torch.float32, device=dev)
        work = torch.empty((ptheta, nscan, 2), dtype=torch.float32, device=dev) if k is not None else None
        for c0 in range(0, nval, nat.SCAN_MAP_MAX_VALUES):
            nv = min(nat.SCAN_MAP_MAX_VALUES, nval - c0)
            part = v3[..., c0:c0 + nv].contiguous()
            dst = out if nv == nval else torch.empty((ptheta, nv, nz, n), dtype=torch.float32, device=dev)
            nat.check(nat.scan_map(_ptr(weight), _ptr(dst), _ptr(part), _opt(k), _ptr(s), _ptr(p), ptheta, nscan, nv, nmodes,
                                   nprb, nz, n, 0 if normalize else 1, _opt(work), _stream()))
            if dst is not out:
                out[:, c0:c0 + nv] = dst
    return weight, (out[:, 0] if len(values.shape) == 2 else out)


def integrate_gradient(gy, gx, weight=None, tol=1e-4, maxiter=None, check_every=256, out=None):
    """The surface whose neighbour differences match the gradient field ``(gy, gx)`` best, by weighted least squares.

    ``gy``, ``gx``: float32 ``[nz, n]`` or ``[ptheta, nz, n]``, the gradient along the row index and along the column
    index in units per pixel; ``weight``: the same shape, float32 or bool, as for ``unwrap_phase`` (an edge weighs the
    smaller weight of its two pixels, what the field holds at a pixel of weight 0 never matters).  The difference of an
    edge is the mean of the gradient at its two ends; the solver, its controls ``tol``, ``maxiter`` and ``check_every`` and
    its synchronisation (one read-back of the state per ``check_every`` iterations) are ``unwrap_phase``'s.

    Returns a dict: ``"phase"`` (float32 on the device, ``out`` if given), the surface minus its weighted mean where a
    pixel has a weighted edge and 0 elsewhere, and per angle on the host ``"iterations"``, ``"residual"``,
    ``"converged"`` and ``"status"``.  For 2-D input the angle axis is dropped.  Bitwise reproducible.
    """
    ptheta, nz, n, maxiter = check_integrate(gy, gx, weight, tol, maxiter, check_every, out)
    (y, x, w), dev = _to_device((gy, gx, weight), "dpc", _HOST)
    if w is not None:
        w = w.to(torch.float32).contiguous()
    _check_out(out, dev, "out must be a contiguous tensor on the operands' device")
    with torch.cuda.device(dev):
        buf = torch.empty((int(nat.unwrap_buffer_floats(ptheta, nz, n)),), dtype=torch.float32, device=dev)
        work = torch.empty((int(nat.unwrap_work_words(ptheta, nz, n)),), dtype=torch.float64, device=dev)
        state = torch.empty((ptheta, nat.UNWRAP_STATE_WORDS), dtype=torch.float64, device=dev)
        res = torch.empty((ptheta, nz, n), dtype=torch.float32, device=dev) if out is None else out
        sizes = (ptheta, nz, n)
        nat.check(nat.integrate_begin(_ptr(buf), _ptr(state), _ptr(y), _ptr(x), _opt(w), *sizes, _ptr(work), _stream()))
        done = 0
        while True:
            niter = min(int(check_every), maxiter - done)
            nat.check(nat.unwrap_iterate(_ptr(buf), _ptr(state), _opt(w), *sizes, niter, maxiter, float(tol), _ptr(work),
                                         _stream()))
            done += niter
            host = state.cpu()                          # the only synchronisation of the loop
            if bool((host[:, nat.UNWRAP_STATUS] != 0).all()) or done >= maxiter:
                break
        nat.check(nat.integrate_finish(_ptr(res), _ptr(state), _ptr(buf), _opt(w), *sizes, _ptr(work), _stream()))
        host = host.numpy()
    status = host[:, nat.UNWRAP_STATUS].astype(np.int64)
    info = {"iterations": host[:, nat.UNWRAP_ITER].astype(np.int64), "residual": host[:, nat.UNWRAP_RELRES].copy(),
            "converged": status == 1, "status": status}
    if len(gy.shape) == 2:
        res = res if out is not None else res[0]
        info = {k: v[0].item() for k, v in info.items()}
    info["phase"] = res
    return info


# ---- the chain ----------------------------------------------------------------------------------------------------------------
def first_look(data, scan, probe, nz, n, mask=None, reference="mean", keep=None, floor=0.05, darkfield=None, tol=1e-4,
               maxiter=None):
    """STXM, dark-field and DPC maps of a scan, and the phase that the DPC gradient integrates to.

    ``data``: float32 ``[ptheta, nscan, ndet, ndet]`` in the solver's layout; ``scan``: ``[ptheta, nscan, 2]``;
    ``probe``: ``[ptheta, M, nprb, nprb]`` or ``[ptheta, nprb, nprb]`` (``initial_probe`` gives one); ``nz``, ``n``: the
    object grid.  ``mask``, ``darkfield``: as for ``frame_moments``.  ``keep``: as for ``scan_map``; a frame without
    intensity or with a non-finite moment is excluded as well.

    The gradient of a frame is ``(2 pi / ndet) (c - c0)``.  ``reference="mean"`` takes ``c0`` as the mean centre of the
    angle's kept frames, weighted by their intensity: that removes exactly a ramp from the phase, which is gauge (a ramp
    on the object against a shift of the probe's spectrum).  ``reference=(cy, cx)`` gives ``c0``: from a frame taken
    without the object, or for a known probe from
    ``frame_moments(|fwd(ones, one whole-pixel position, probe)|^2)["center"]``.

    The four channels ``sum I, dark-field sum, g_y, g_x`` go through one ``scan_map``;
    ``lit = weight >= floor max(weight)`` per angle (and ``weight > 0``), and ``integrate_gradient`` runs with the weight
    ``weight / max`` where lit, 0 elsewhere, and ``tol``, ``maxiter``.

    Returns a dict of device tensors ``[ptheta, nz, n]`` -- ``"transmission"`` (the map of ``sum I`` over
    ``sum_m sum |P_m|^2``: ``|object|^2`` averaged over the probe), ``"darkfield"``, ``"dpc_y"``, ``"dpc_x"`` (rad / pixel),
    ``"phase"``, ``"illumination"``, ``"lit"`` (bool) -- with ``"moments"`` (``frame_moments``'s ``[ptheta, nscan, 8]``),
    ``"reference"`` (``c0``, ``[ptheta, 2]``) and the solver's ``"iterations"``, ``"residual"``, ``"converged"``,
    ``"status"`` per angle on the host.  The maps are the object blurred by the probe, and a mask biases both moments
    (module docstring).
    """
    ptheta, nscan, ndet, nz, n, ref = check_first_look(data, scan, probe, nz, n, mask, reference, keep, floor, darkfield,
                                                       tol, maxiter)
    if keep is not None and not isinstance(keep, torch.Tensor):
        keep = np.ascontiguousarray(np.asarray(keep) != 0)
    (d, s, p, k), dev = _to_device((data, scan, probe, keep), "dpc", _HOST)
    with torch.cuda.device(dev):
        fm = frame_moments(d, mask, darkfield)
        mom = fm["moments"]
        used = (mom[..., 0] > 0) & torch.isfinite(mom[..., :3]).all(-1)
        if k is not None:
            used = used & (k != 0)
        if ref is None:
            m = torch.where(used[..., None], mom[..., :3], torch.zeros_like(mom[..., :3])).sum(dim=1)
            c0 = torch.where(m[:, 0:1] > 0, m[:, 1:3] / m[:, 0:1], torch.zeros_like(m[:, 1:3]))
        else:
            c0 = torch.tensor(ref, dtype=torch.float64, device=dev).expand(ptheta, 2)
        g = (2.0 * np.pi / ndet) * (fm["center"] - c0[:, None, :])
        values = torch.stack([mom[..., 0], mom[..., 6], g[..., 0], g[..., 1]], dim=-1)
        values = torch.where(used[..., None], values, torch.zeros_like(values)).to(torch.float32)
        weight, out = scan_map(values, s, p, nz, n, used)
        top = torch.amax(weight, dim=(-2, -1), keepdim=True)
        lit = (weight >= torch.tensor(floor, dtype=torch.float32, device=dev) * top) & (weight > 0)
        w = torch.where(lit, weight / torch.where(top > 0, top, torch.ones_like(top)), torch.zeros_like(weight))
        power = (p.to(torch.complex128).abs() ** 2).reshape(ptheta, -1).sum(dim=1).to(torch.float32)
        look = integrate_gradient(out[:, 2].contiguous(), out[:, 3].contiguous(), w, tol=tol, maxiter=maxiter)
        look.update({"moments": mom, "transmission": out[:, 0] / power[:, None, None], "darkfield": out[:, 1],
                     "dpc_y": out[:, 2], "dpc_x": out[:, 3], "illumination": weight, "lit": lit, "reference": c0})
    return look


def initial_object(look, amplitude=True):
    """A starting object from ``first_look``'s result: complex64 ``[ptheta, nz, n]``,
    ``sqrt(max(transmission, 0)) exp(i phase)`` where lit (amplitude 1 with ``amplitude=False``) and ``1 + 0j`` elsewhere.

    It is the object blurred by the probe, in the gauge of ``first_look``'s reference: a reconstruction started from it
    begins at a fraction of the cost of ``psi = 1`` and with the phase already unwrapped.
    """
    if not isinstance(look, dict) or not all(k in look for k in ("transmission", "phase", "lit")):
        raise ValueError("look must be the dict that first_look returns")
    if not isinstance(amplitude, (bool, np.bool_)):
        raise TypeError("amplitude must be a bool, got %r" % (amplitude,))
    phase, lit = look["phase"], look["lit"]
    amp = torch.sqrt(torch.clamp(look["transmission"], min=0.0)) if amplitude else torch.ones_like(phase)
    psi = torch.polar(amp, phase)
    return torch.where(lit, psi, torch.ones_like(psi)).contiguous()
