"""B-spline resampling of images on the device: rotation, change of pixel size, sub-pixel shifts, centre of mass.

A reconstructed phase becomes a tomography projection by a rotation through the tilt, a recentring on its centre of mass
and a crop; two reconstructions with different pixel sizes meet on one grid before ``frc`` compares them; a run starts
from a coarser one.  ``warp`` does all of these in one pass: an affine map in the convention of
``scipy.ndimage.affine_transform`` -- output pixel ``o = (oy, ox)`` takes the value at the source coordinate
``matrix @ o + offset``, axes in ``(y, x)`` order -- interpolated by B-splines of order 0 ... 5 with mirror extension, as
``scipy.ndimage`` does with ``mode="mirror"``.  ``rotate``, ``zoom`` and ``shift`` build the maps of their SciPy
namesakes, ``spline_prefilter`` is ``scipy.ndimage.spline_filter(mode="mirror")`` and ``center_of_mass`` returns the
first and second moments.  Kernels: ``csrc/k_resample.hpp``, C ABI ``ptycho_spline_prefilter``, ``ptycho_warp``,
``ptycho_moments``; include/ptycho_hip.h and DESIGN.md section 17 state the definition in full, and
tests/resample_ref.py restates it in NumPy.  Coordinates are float64, weights and sums float32.  Bitwise reproducible.

The steps that turn a phase into a projection, in one pass over the image::

    phase = unwrap_phase(fa["psi"], weight=fa["lit"])["phase"]
    com = center_of_mass(phase, which="positive")["center"].cpu().numpy()
    projection = rotate(phase, -tilt, center=com, shape=(height, width), order=5)
"""
import numbers

import numpy as np
import torch

from . import _native as nat
from ._args import _check_out, _dtype, _need_array, _opt, _to_device
from .operators import _ptr, _stream

__all__ = ["spline_prefilter", "warp", "rotate", "zoom", "shift", "center_of_mass", "check_warp"]

IMAGE_DTYPES = ("float32", "complex64")
MODES = {"constant": 0, "mirror": nat.WARP_MIRROR}
WHICH = {"value": 0, "positive": 1, "power": 2}
MAX_IMAGES, MAX_SIDE, MAX_PIXELS = 65535, 65536, 2 ** 31
TILE = 32


def _image(x, name="x"):
    """``(lead, nimg, ny, nx, cplx)`` of an image batch ``[..., ny, nx]`` (no device use)."""
    _need_array(x, name)
    if _dtype(x) not in IMAGE_DTYPES:
        raise TypeError("%s must be float32 or complex64, got %s" % (name, _dtype(x)))
    shape = tuple(int(v) for v in x.shape)
    if len(shape) < 2:
        raise ValueError("%s must be [..., ny, nx], got shape %s" % (name, shape))
    lead, (ny, nx) = shape[:-2], shape[-2:]
    nimg = int(np.prod(lead, dtype=np.int64)) if lead else 1
    if ny < 2 or nx < 2 or ny > MAX_SIDE or nx > MAX_SIDE or ny * nx >= MAX_PIXELS or not 1 <= nimg <= MAX_IMAGES:
        raise ValueError("%s needs sides in [2, 65536], ny * nx < 2^31 and 1 to 65535 images, got shape %s" % (name, shape))
    return lead, nimg, ny, nx, _dtype(x) == "complex64"


def _order(order):
    if isinstance(order, bool) or not isinstance(order, numbers.Integral) or not 0 <= order <= 5:
        raise ValueError("order must be an integer in [0, 5], got %r" % (order,))
    return int(order)


def _host_floats(v, name, tail, lead):
    """``v`` as float64 ``[nimg] + tail`` on the host: one for all images, or one per image."""
    if isinstance(v, torch.Tensor):
        v = v.detach().cpu().numpy()
    try:
        a = np.asarray(v, dtype=np.float64)
    except (TypeError, ValueError):
        raise TypeError("%s must be an array of real numbers, got %r" % (name, type(v).__name__)) from None
    if a.shape != tail and a.shape != lead + tail:
        raise ValueError("%s must have shape %s or %s, got %s" % (name, tail, lead + tail, a.shape))
    if not np.isfinite(a).all():
        raise ValueError("%s must be finite" % name)
    nimg = int(np.prod(lead, dtype=np.int64)) if lead else 1
    return np.ascontiguousarray(np.broadcast_to(a, lead + tail)).reshape((nimg,) + tail)


def check_warp(x, matrix=None, offset=None, shape=None, order=3, mode="constant", cval=0.0, prefilter=True, out=None):
    """Validate ``warp``'s arguments (no device use); returns ``(lead, ny, nx, oh, ow, cplx, xf)`` with ``xf`` the float64
    ``[nimg, 6]`` rows ``(m00, m01, m10, m11, offy, offx)`` that the kernel reads."""
    lead, nimg, ny, nx, cplx = _image(x)
    m = _host_floats(np.eye(2) if matrix is None else matrix, "matrix", (2, 2), lead)
    o = _host_floats(np.zeros(2) if offset is None else offset, "offset", (2,), lead)
    if shape is None:
        shape = (ny, nx)
    try:
        oh, ow = shape
    except (TypeError, ValueError):
        raise ValueError("shape must be (height, width), got %r" % (shape,)) from None
    for v in (oh, ow):
        if isinstance(v, bool) or not isinstance(v, numbers.Integral) or not 1 <= v <= MAX_SIDE:
            raise ValueError("shape must hold two integers in [1, 65536], got %r" % (shape,))
    if oh * ow >= MAX_PIXELS:
        raise ValueError("shape must hold fewer than 2^31 pixels, got %r" % (shape,))
    _order(order)
    if mode not in MODES:
        raise ValueError("mode must be 'constant' or 'mirror', got %r" % (mode,))
    if isinstance(cval, bool) or not isinstance(cval, numbers.Complex):
        raise TypeError("cval must be a number, got %r" % (cval,))
    if not cplx and not isinstance(cval, numbers.Real):
        raise TypeError("cval must be real for a real image, got %r" % (cval,))
    if not isinstance(prefilter, (bool, np.bool_)):
        raise TypeError("prefilter must be a bool, got %r" % (prefilter,))
    if out is not None:
        _need_array(out, "out")
        if _dtype(out) != _dtype(x):
            raise TypeError("out must be %s like x, got %s" % (_dtype(x), _dtype(out)))
        if tuple(out.shape) != lead + (int(oh), int(ow)):
            raise ValueError("out must have shape %s, got %s" % (lead + (int(oh), int(ow)), tuple(out.shape)))
    xf = np.concatenate([m.reshape(nimg, 4), o], axis=1)
    return lead, ny, nx, int(oh), int(ow), cplx, xf


_HOST = "x and weight must be device tensors or NumPy arrays"   # what a host tensor among the operands raises


def _prefilter(xi, nimg, ny, nx, cplx, order, res):
    """``res`` <- coefficients of the contiguous device tensor ``xi``; ``res`` may be ``xi``."""
    words = int(nat.spline_work_words(nimg, ny, nx, int(cplx)))
    work = torch.empty((words,), dtype=torch.float64, device=xi.device)
    nat.check(nat.spline_prefilter(_ptr(res), _ptr(xi), nimg, ny, nx, int(cplx), order, _ptr(work), _stream()))
    return res


def spline_prefilter(x, order=3, out=None):
    """B-spline coefficients of ``x`` (``[..., ny, nx]`` float32 or complex64, a device tensor or a NumPy array) along its
    last two axes, mirror extension: ``scipy.ndimage.spline_filter(x, order, mode="mirror")`` per image, in float32.
    Orders 0 and 1 return a copy.  ``out``: a contiguous device tensor like ``x``; it may be ``x`` itself."""
    lead, nimg, ny, nx, cplx = _image(x)
    order = _order(order)
    if out is not None:
        _need_array(out, "out")
        if _dtype(out) != _dtype(x) or tuple(out.shape) != tuple(x.shape):
            raise ValueError("out must be %s of shape %s" % (_dtype(x), tuple(x.shape)))
    (xi,), dev = _to_device((x,), "resample", _HOST)
    _check_out(out, dev, "out must be a contiguous tensor on the operands' device")
    with torch.cuda.device(dev):
        res = torch.empty_like(xi) if out is None else out
        return _prefilter(xi, nimg, ny, nx, cplx, order, res)


def _warp(x, matrix, offset, shape, order, mode, cval, prefilter, out, force_global=False, paths=False):
    """``warp`` and what the tests ask of it: ``force_global`` reads every tap from global memory, ``paths`` also returns
    the int32 ``[..., tiles_y, tiles_x]`` map of the path each output tile took (0 outside, 1 LDS, 2 global)."""
    lead, ny, nx, oh, ow, cplx, xf = check_warp(x, matrix, offset, shape, order, mode, cval, prefilter, out)
    nimg = xf.shape[0]
    (xi,), dev = _to_device((x,), "resample", _HOST)
    _check_out(out, dev, "out must be a contiguous tensor on the operands' device")
    with torch.cuda.device(dev):
        coef = xi
        if prefilter and order >= 2:
            coef = _prefilter(xi, nimg, ny, nx, cplx, int(order), torch.empty_like(xi))
        elif out is not None and out.data_ptr() == xi.data_ptr():
            coef = xi.clone()
        res = torch.empty(lead + (oh, ow), dtype=xi.dtype, device=dev) if out is None else out
        xf_dev = torch.from_numpy(xf).to(dev)
        path = None
        if paths:
            path = torch.empty(lead + (-(-oh // TILE), -(-ow // TILE)), dtype=torch.int32, device=dev)
        flags = MODES[mode] | (nat.WARP_GLOBAL if force_global else 0)
        c = complex(cval)
        nat.check(nat.warp(_ptr(res), _ptr(coef), _ptr(xf_dev), nimg, ny, nx, oh, ow, int(cplx), int(order), flags,
                           c.real, c.imag, _opt(path), _stream()))
    return (res, path) if paths else res


def warp(x, matrix=None, offset=None, shape=None, order=3, mode="constant", cval=0.0, prefilter=True, out=None):
    """Resample ``x`` under an affine map, as ``scipy.ndimage.affine_transform`` does with ``mode="mirror"`` splines.

    ``x``: ``[..., ny, nx]`` float32 or complex64, a device tensor or a NumPy array (copied to the device).  Output pixel
    ``(oy, ox)`` takes the value of the spline through ``x`` at ``matrix @ (oy, ox) + offset``; ``matrix`` is ``[2, 2]``
    or ``[..., 2, 2]`` and ``offset`` ``[2]`` or ``[..., 2]`` (one per image), host arrays of finite numbers, ``None`` the
    identity and zero.  ``shape = (height, width)`` of the output, ``None``: that of ``x``; cropping or extending costs
    nothing.  ``order`` 0 ... 5.  ``mode="constant"``: a pixel whose source lies outside ``[0, ny - 1] x [0, nx - 1]``
    (by more than ``2^-20`` pixel, within which it is clamped) becomes ``cval``; ``mode="mirror"``: every pixel is
    evaluated on the mirrored image.  ``prefilter=False`` takes ``x`` as coefficients already
    (``spline_prefilter``), which saves the filter when one image is warped several times.  Complex images interpolate
    real and imaginary part alike.  Returns a device tensor ``[..., height, width]`` of ``x``'s dtype (``out`` if given:
    contiguous, written in full).  Two launches for the prefilter and one for the warp, no synchronisation."""
    return _warp(x, matrix, offset, shape, order, mode, cval, prefilter, out)


def _pairs(v, name, lead):
    return _host_floats(v, name, (2,), lead).reshape(lead + (2,))


def rotate(x, angle, center=None, order=3, shape=None, mode="constant", cval=0.0, prefilter=True, out=None):
    """Rotate ``x`` by ``angle`` degrees (one number, or one per image: ``[...]``) in the sense of
    ``scipy.ndimage.rotate(x, angle, reshape=False)``.  ``center = (cy, cx)`` (or ``[..., 2]``) is the point of ``x`` that
    the rotation turns about AND that lands on the centre ``(shape - 1) / 2`` of the output; ``None``: the centre
    ``((ny - 1) / 2, (nx - 1) / 2)`` of ``x``.  With ``center`` a centre of mass and ``shape`` a crop this rotates,
    recentres and crops in one pass.  The other arguments are ``warp``'s."""
    lead, nimg, ny, nx, cplx = _image(x)
    ang = np.deg2rad(_host_floats(angle, "angle", (), lead).reshape(lead))
    c, s = np.cos(ang), np.sin(ang)
    matrix = np.stack([np.stack([c, s], -1), np.stack([-s, c], -1)], -2)
    if shape is None:
        shape = (ny, nx)
    oh, ow = check_warp(x, None, None, shape, order, mode, cval, prefilter, out)[3:5]
    centre = _pairs(np.array([(ny - 1) / 2.0, (nx - 1) / 2.0]) if center is None else center, "center", lead)
    out_centre = np.array([(oh - 1) / 2.0, (ow - 1) / 2.0])
    offset = centre - matrix @ out_centre
    return warp(x, matrix, offset, shape, order, mode, cval, prefilter, out)


def _zoom_shape(n, f):
    return int(round(n * f))


def zoom(x, factor, order=3, mode="constant", cval=0.0, prefilter=True, out=None):
    """Change the pixel size of ``x`` by ``factor`` (one number, or ``(fy, fx)``), as ``scipy.ndimage.zoom``: the output
    has sides ``round(n * factor)`` and its corner pixels sit on the corner pixels of ``x`` (source coordinate
    ``o (n_in - 1) / (n_out - 1)``).  The other arguments are ``warp``'s."""
    lead, nimg, ny, nx, cplx = _image(x)
    if np.ndim(factor) == 0:
        f = np.full(2, _host_floats(factor, "factor", (), ())[0])
    else:
        f = _host_floats(factor, "factor", (2,), ())[0]
    if not (f > 0).all():
        raise ValueError("factor must be positive, got %r" % (factor,))
    oh, ow = _zoom_shape(ny, f[0]), _zoom_shape(nx, f[1])
    if oh < 1 or ow < 1:
        raise ValueError("factor %r leaves no pixels of shape %s" % (factor, (ny, nx)))
    zy = (ny - 1) / (oh - 1) if oh > 1 else 1.0
    zx = (nx - 1) / (ow - 1) if ow > 1 else 1.0
    return warp(x, np.array([[zy, 0.0], [0.0, zx]]), None, (oh, ow), order, mode, cval, prefilter, out)


def shift(x, shift, order=3, mode="constant", cval=0.0, prefilter=True, out=None):
    """Shift ``x`` by ``shift = (dy, dx)`` pixels (or one pair per image: ``[..., 2]``), as ``scipy.ndimage.shift``: output
    pixel ``o`` takes the value at ``o - shift``.  The other arguments are ``warp``'s."""
    lead = _image(x)[0]
    return warp(x, None, -_pairs(shift, "shift", lead), None, order, mode, cval, prefilter, out)


def center_of_mass(x, weight=None, which="value"):
    """First and second moments of the images ``x`` (``[..., ny, nx]``), in float64 on the device, in a fixed order.

    The mass of a pixel is ``w = x`` (``which="value"``), ``max(x, 0)`` (``"positive"``) or ``|x|^2`` (``"power"``, the
    only choice for complex ``x``), times ``weight`` (float32, ``x``'s shape) if given.  Returns a dict of device tensors:
    ``"center"`` ``[..., 2]``, ``(sum w y, sum w x) / sum w``; ``"second"`` ``[..., 2]``, the variances
    ``sum w y^2 / sum w - cy^2`` and likewise for ``x``; ``"mass"`` ``[...]``, ``sum w``; ``"sums"`` ``[..., 5]``, the raw
    ``sum w, sum w y, sum w x, sum w y^2, sum w x^2``.  An image without mass gives NaN.  Two launches, no
    synchronisation."""
    lead, nimg, ny, nx, cplx = _image(x)
    if which not in WHICH:
        raise ValueError("which must be 'value', 'positive' or 'power', got %r" % (which,))
    if cplx and which != "power":
        raise ValueError("a complex image has no value or positive part: which must be 'power'")
    if weight is not None:
        _need_array(weight, "weight")
        if _dtype(weight) != "float32":
            raise TypeError("weight must be float32, got %s" % _dtype(weight))
        if tuple(weight.shape) != tuple(x.shape):
            raise ValueError("weight must have x's shape %s, got %s" % (tuple(x.shape), tuple(weight.shape)))
    (xi, w), dev = _to_device((x, weight), "resample", _HOST)
    with torch.cuda.device(dev):
        work = torch.empty((int(nat.moments_work_words(nimg, ny, nx)),), dtype=torch.float64, device=dev)
        sums = torch.empty(lead + (5,), dtype=torch.float64, device=dev)
        nat.check(nat.moments(_ptr(sums), _ptr(xi), _opt(w), nimg, ny, nx, int(cplx), WHICH[which], _ptr(work), _stream()))
        mass = sums[..., 0]
        center = sums[..., 1:3] / mass[..., None]
        second = sums[..., 3:5] / mass[..., None] - center * center
    return {"center": center, "second": second, "mass": mass, "sums": sums}
