"""ctypes binding of ``libptychohip.so`` (C ABI: ``include/ptycho_hip.h``).

Replaces the SWIG / pybind11 extension module ``libtike.cufft.ptychofft``
(``/root/reference/src/cuda/swig/ptychofft.i:1-26``,
``/root/reference/src/cuda/pybind11/ptychofft.cxx:1-27``).  There is no
fallback: if the shared library is missing this module raises at import.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("PTYCHO_HIP_LIB") or os.path.join(_HERE, "libptychohip.so")

#: every symbol ``include/ptycho_hip.h`` declares
SYMBOLS = ("ptycho_create", "ptycho_free", "ptycho_destroy", "ptycho_get",
           "ptycho_fwd", "ptycho_adj", "ptycho_fft2", "ptycho_adj_scan", "ptycho_set_option",
           "ptycho_profile", "ptycho_profile_read",
           "ptycho_cg_fwd_cols", "ptycho_cg_stats", "ptycho_cg_project",
           "ptycho_cg_adj_cols", "ptycho_cg_linesearch",
           "ptycho_cg_project_multi",
           "ptycho_cg_intensity_modes", "ptycho_cg_linesearch_modes",
           "ptycho_cg_cross", "ptycho_cg_argmax", "ptycho_cg_zoom",
           "ptycho_cg_fwd_cols_modes", "ptycho_cg_linesearch_chunk",
           "ptycho_cg_obj_begin", "ptycho_cg_obj_grad", "ptycho_cg_obj_dir", "ptycho_cg_ls_next",
           "ptycho_cg_reg_prepare",
           "ptycho_cg_obj_finish", "ptycho_cg_prb_grad", "ptycho_cg_prb_dir", "ptycho_cg_prb_finish",
           "ptycho_cg_ls_begin", "ptycho_cg_ls_obj_chunk", "ptycho_cg_ls_prb_pass", "ptycho_cg_ls_decide",
           "ptycho_cg_cross_dev", "ptycho_cg_obj_begin2", "ptycho_cg_obj_dir2",
           "ptycho_set_mask", "ptycho_orthogonalize_modes",
           "ptycho_frc_prepare", "ptycho_frc_rings",
           "ptycho_illumination", "ptycho_gauge_fit", "ptycho_gauge_apply",
           "ptycho_fit_accumulate", "ptycho_fit_work_words", "ptycho_fit_frames",
           "ptycho_prepare_work_words", "ptycho_prepare_frames",
           "ptycho_unwrap_work_words", "ptycho_unwrap_buffer_floats", "ptycho_unwrap_begin", "ptycho_unwrap_iterate",
           "ptycho_unwrap_finish", "ptycho_unwrap_residues",
           "ptycho_frame_moments_work_words", "ptycho_frame_moments", "ptycho_scan_map",
           "ptycho_integrate_begin", "ptycho_integrate_finish",
           "ptycho_propagate_work_words", "ptycho_propagate",
           "ptycho_spline_work_words", "ptycho_spline_prefilter", "ptycho_warp",
           "ptycho_moments_work_words", "ptycho_moments",
           "ptycho_last_error", "ptycho_version")

if not os.path.exists(LIB_PATH):
    raise ImportError(
        "libtike.hipfft: %s not found -- build it with "
        "`make -C libtike-cufft_amd/csrc` (or `python -c 'import "
        "__graft_entry__ as g; g.build()'`). There is no CPU fallback." % LIB_PATH)

lib = ctypes.CDLL(LIB_PATH)

_vp, _sz, _i, _ll = ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int, ctypes.c_longlong


def _sig(name, res, *args):
    fn = getattr(lib, name)
    fn.restype = res
    fn.argtypes = list(args)
    return fn


create = _sig("ptycho_create", _i, ctypes.POINTER(_vp), _sz, _sz, _sz, _sz, _sz, _sz)
free = _sig("ptycho_free", _i, _vp)
destroy = _sig("ptycho_destroy", _i, _vp)
get = _sig("ptycho_get", _ll, _vp, _i)
fwd = _sig("ptycho_fwd", _i, _vp, _vp, _vp, _vp, _vp, _vp)
adj = _sig("ptycho_adj", _i, _vp, _vp, _vp, _vp, _vp, _i, _vp)
fft2 = _sig("ptycho_fft2", _i, _vp, _vp, _vp, _sz, _i, _vp)
#: h, out, g, f, scan, prb, work, work_tiles, stream
adj_scan = _sig("ptycho_adj_scan", _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _vp)
set_option = _sig("ptycho_set_option", _i, _vp, ctypes.c_char_p, _ll)
cg_fwd_cols = _sig("ptycho_cg_fwd_cols", _i, _vp, _i, _vp, _vp, _vp, _vp)
cg_stats = _sig("ptycho_cg_stats", _i, _vp, _i, _vp, _vp, _vp)
cg_project = _sig("ptycho_cg_project", _i, _vp, _i, _i, _vp, _vp, _vp, _vp)
cg_adj_cols = _sig("ptycho_cg_adj_cols", _i, _vp, _i, _vp, _vp, _vp, _i, _vp)
cg_linesearch = _sig("ptycho_cg_linesearch", _i, _vp, _i, _i, _vp, _vp, ctypes.c_double, _i, _vp, _vp)
cg_project_multi = _sig("ptycho_cg_project_multi", _i, _vp, _i, _i, _vp, _vp, _vp, _i, _vp, _vp)
cg_intensity_modes = _sig("ptycho_cg_intensity_modes", _i, _vp, _i, _vp, _vp, _vp, _vp)
cg_linesearch_modes = _sig("ptycho_cg_linesearch_modes", _i, _vp, _i, _i, _vp, _vp, _vp, ctypes.c_double, _i, _vp, _vp)
cg_cross = _sig("ptycho_cg_cross", _i, _vp, _i, _i, ctypes.c_double, _vp, _vp)
cg_argmax = _sig("ptycho_cg_argmax", _i, _vp, _i, _vp, _vp)
cg_zoom = _sig("ptycho_cg_zoom", _i, _vp, _vp, _vp, _vp, _vp, _i, _i, ctypes.c_double, _vp, _vp)
_d = ctypes.c_double
cg_fwd_cols_modes = _sig("ptycho_cg_fwd_cols_modes", _i, _vp, _i, _i, _vp, _vp, ctypes.POINTER(_vp), _i, _i, _vp)
cg_linesearch_chunk = _sig("ptycho_cg_linesearch_chunk", _i, _vp, _i, _vp, _vp, _d, _i, _vp, _vp)
cg_obj_begin = _sig("ptycho_cg_obj_begin", _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
cg_obj_grad = _sig("ptycho_cg_obj_grad", _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
cg_obj_dir = _sig("ptycho_cg_obj_dir", _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
cg_ls_next = _sig("ptycho_cg_ls_next", _i, _vp, _vp, _i, _i, _vp, _i, _vp)
cg_reg_prepare = _sig("ptycho_cg_reg_prepare", _i, _vp, _vp, _vp, _vp, _vp, _vp)
cg_obj_finish = _sig("ptycho_cg_obj_finish", _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _i, _i, _d, _vp)
cg_prb_grad = _sig("ptycho_cg_prb_grad", _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
cg_prb_dir = _sig("ptycho_cg_prb_dir", _i, _vp, _vp, _i, _d, _d, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
cg_prb_finish = _sig("ptycho_cg_prb_finish", _i, _vp, _vp, _vp, _vp, _vp)
cg_ls_begin = _sig("ptycho_cg_ls_begin", _i, _vp, _vp, _i, _vp)
cg_ls_obj_chunk = _sig("ptycho_cg_ls_obj_chunk", _i, _vp, _vp, _i, _vp, _vp, ctypes.POINTER(_vp), _vp, _vp, _vp)
cg_ls_prb_pass = _sig("ptycho_cg_ls_prb_pass", _i, _vp, _vp, _i, _vp, _vp, _vp)
cg_ls_decide = _sig("ptycho_cg_ls_decide", _i, _vp, _vp, _i, _i, _vp)
cg_cross_dev = _sig("ptycho_cg_cross_dev", _i, _vp, _i, _i, _vp, _vp, _vp)
cg_obj_begin2 = _sig("ptycho_cg_obj_begin2", _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
cg_obj_dir2 = _sig("ptycho_cg_obj_dir2", _i, _vp, _vp, _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp)
set_mask = _sig("ptycho_set_mask", _i, _vp, _vp, _vp)
#: orthogonal probe modes (no handle): prb, dprb, gradprb0, ptheta, nmodes, npix, v_out, powers, stream
orthogonalize_modes = _sig("ptycho_orthogonalize_modes", _i, _vp, _vp, _vp, _sz, _i, _sz, _vp, _vp, _vp)
ORTHO_MAX_MODES = 16
#: Fourier ring correlation (no handle): out, a, b, ptheta, nz, n, y0, x0, s, window, stream
frc_prepare = _sig("ptycho_frc_prepare", _i, _vp, _vp, _vp, _sz, _sz, _sz, _sz, _sz, _sz, _vp, _vp)
#: sums, spec, ptheta, s, shift, stream
frc_rings = _sig("ptycho_frc_rings", _i, _vp, _vp, _sz, _sz, _vp, _vp)
#: illumination map (no handle): out, scan, probe, ptheta, nscan, nmodes, nprb, nz, n, stream
illumination = _sig("ptycho_illumination", _i, _vp, _vp, _vp, _sz, _sz, _i, _sz, _sz, _sz, _vp)
#: gauge, psi, ref, weight, ptheta, nz, n, work, stream
gauge_fit = _sig("ptycho_gauge_fit", _i, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp)
#: x, gauge, ptheta, ny, nx, which, stream
gauge_apply = _sig("ptycho_gauge_apply", _i, _vp, _vp, _sz, _sz, _sz, _i, _vp)
#: float64 words of ``gauge_fit``'s scratch per angle (PTYCHO_GAUGE_WORK_PER_ANGLE)
GAUGE_WORK_PER_ANGLE = 16384
#: fit residuals (no handle): inten, g, count, add, stream
fit_accumulate = _sig("ptycho_fit_accumulate", _i, _vp, _vp, _sz, _i, _vp)
#: ptheta, nscan, npix -> float64 words of ``fit_frames``'s scratch (0 for sizes out of range)
fit_work_words = _sig("ptycho_fit_work_words", _sz, _sz, _sz, _sz)
#: frames, pixels, inten, g, data, mask, ab, ptheta, nscan, npix, work, stream
fit_frames = _sig("ptycho_fit_frames", _i, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp)
#: frame preparation (no handle): ptheta, nscan, npix -> float64 words of ``prepare_frames``'s scratch (0: out of range)
prepare_work_words = _sig("ptycho_prepare_work_words", _sz, _sz, _sz, _sz)
#: data, mask, frames, pixels, raw, dtype, index, dark, gain, bad, ptheta, nraw, nscan, H, W, y0, x0, bin, ndet,
#: saturation, scale, clip, work, stream
prepare_frames = _sig("ptycho_prepare_frames", _i, _vp, _vp, _vp, _vp, _vp, _i, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _sz, _sz,
                      _ll, _ll, _i, _sz, ctypes.c_float, ctypes.c_float, _i, _vp, _vp)
#: ``dtype`` codes of ``prepare_frames``'s raw frames
PREPARE_DTYPES = {"uint16": 0, "uint32": 1, "int32": 2, "float32": 3}
#: phase unwrapping (no handle): ptheta, nz, n -> float64 words of scratch / float32 words of ``buf`` (0: out of range)
unwrap_work_words = _sig("ptycho_unwrap_work_words", _sz, _sz, _sz, _sz)
unwrap_buffer_floats = _sig("ptycho_unwrap_buffer_floats", _sz, _sz, _sz, _sz)
#: buf, state, phase, weight, ptheta, nz, n, work, stream
unwrap_begin = _sig("ptycho_unwrap_begin", _i, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp)
#: buf, state, weight, ptheta, nz, n, niter, maxiter, tol, work, stream
unwrap_iterate = _sig("ptycho_unwrap_iterate", _i, _vp, _vp, _vp, _sz, _sz, _sz, _i, _i, ctypes.c_double, _vp, _vp)
#: out, state, buf, phase, weight, congruent, ptheta, nz, n, work, stream
unwrap_finish = _sig("ptycho_unwrap_finish", _i, _vp, _vp, _vp, _vp, _vp, _i, _sz, _sz, _sz, _vp, _vp)
#: charge, count, phase, weight, ptheta, nz, n, stream
unwrap_residues = _sig("ptycho_unwrap_residues", _i, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _vp)
#: first look (no handle): ptheta, nscan, ndet -> float64 words of ``frame_moments``'s scratch (0: out of range)
frame_moments_work_words = _sig("ptycho_frame_moments_work_words", _sz, _sz, _sz, _sz)
#: moments, data, mask, darkfield, ptheta, nscan, ndet, work, stream
frame_moments = _sig("ptycho_frame_moments", _i, _vp, _vp, _vp, ctypes.c_double, _sz, _sz, _sz, _vp, _vp)
#: weight, out, values, keep, scan, probe, ptheta, nscan, nval, nmodes, nprb, nz, n, raw, work, stream
scan_map = _sig("ptycho_scan_map", _i, _vp, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _i, _i, _sz, _sz, _sz, _i, _vp, _vp)
#: buf, state, gy, gx, weight, ptheta, nz, n, work, stream (buf, state, work: the unwrapper's)
integrate_begin = _sig("ptycho_integrate_begin", _i, _vp, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp)
#: out, state, buf, weight, ptheta, nz, n, work, stream
integrate_finish = _sig("ptycho_integrate_finish", _i, _vp, _vp, _vp, _vp, _sz, _sz, _sz, _vp, _vp)
#: channels of one ``scan_map`` call
SCAN_MAP_MAX_VALUES = 4
#: propagation (handle of ndet = S): h, nfield, nplane, planes_wanted -> float64 words of ``propagate``'s scratch
propagate_work_words = _sig("ptycho_propagate_work_words", _sz, _vp, _sz, _sz, _i)
#: h, planes, metrics, spec, nfield, zl, nplane, q0, method, work, stream
propagate = _sig("ptycho_propagate", _i, _vp, _vp, _vp, _vp, _sz, _vp, _sz, ctypes.c_double, _i, _vp, _vp)
#: resampling (no handle): nimg, ny, nx, cplx -> float64 words of ``spline_prefilter``'s scratch (0: out of range)
spline_work_words = _sig("ptycho_spline_work_words", _sz, _sz, _sz, _sz, _i)
#: out, in, nimg, ny, nx, cplx, order, work, stream
spline_prefilter = _sig("ptycho_spline_prefilter", _i, _vp, _vp, _sz, _sz, _sz, _i, _i, _vp, _vp)
#: out, coef, xf, nimg, ny, nx, oh, ow, cplx, order, flags, cval_re, cval_im, path, stream
warp = _sig("ptycho_warp", _i, _vp, _vp, _vp, _sz, _sz, _sz, _sz, _sz, _i, _i, _i, ctypes.c_float, ctypes.c_float, _vp, _vp)
#: nimg, ny, nx -> float64 words of ``moments``'s scratch (0: out of range)
moments_work_words = _sig("ptycho_moments_work_words", _sz, _sz, _sz, _sz)
#: sums, x, weight, nimg, ny, nx, cplx, which, work, stream
moments = _sig("ptycho_moments", _i, _vp, _vp, _vp, _sz, _sz, _sz, _i, _i, _vp, _vp)
#: samples of a line per segment of the prefilter (PTYCHO_SPLINE_SEGMENT), the halo per order, ``warp``'s flags
SPLINE_SEGMENT = 64
SPLINE_HALO = {2: 12, 3: 16, 4: 28, 5: 32}
WARP_MIRROR, WARP_GLOBAL = 1, 2
#: ``method`` codes of ``propagate`` and the float64 words it leaves per (field, plane)
PROPAGATE_METHODS = {"fresnel": 0, "angular": 1}
PROPAGATE_WORDS = 8
#: float64 words of the unwrapper's state per angle (PTYCHO_UNWRAP_STATE_WORDS) and the slots the wrapper reads
UNWRAP_STATE_WORDS = 16
UNWRAP_ITER, UNWRAP_STATUS, UNWRAP_RELRES, UNWRAP_C = 5, 6, 7, 8
#: ``get`` keys: options "chunk" and "window" as set; ``GET_WORK_SLOT0 + s``: 1 if CG work slot ``s`` holds device memory
GET_CHUNK, GET_WINDOW, GET_WORK_SLOT0 = 100, 101, 200
#: ``get`` key: 1 if a measured-pixel mask is set on the handle
GET_MASK = 102
#: ``get`` key: option "model" of the CG stages that read data (MODEL_GAUSSIAN, MODEL_POISSON_ML)
GET_MODEL = 103
MODEL_GAUSSIAN, MODEL_POISSON_ML = 0, 1
#: word offsets of the device-resident CG state (enum PTYCHO_ST_* in include/ptycho_hip.h)
ST_A, ST_B, ST_COST, ST_COST2 = 0, 1, 2, 3
ST_GAMMA_PSI, ST_GAMMA_PRB, ST_LS_FAILED, ST_HINT, ST_COSTS, ST_WORDS = 12, 13, 19, 20, 24, 160
ST_NCOSTS = 7 * 17
profile = _sig("ptycho_profile", _i, _vp, _i)
profile_read = _sig("ptycho_profile_read", _i, _vp, ctypes.POINTER(ctypes.c_double),
                    ctypes.POINTER(_ll), _i)
KERNEL_NAMES = ("k_cols<FWD>", "k_rows<fwd>", "k_rows<inv>", "k_cols<ADJ_OBJ>",
                "k_cols<ADJ_PRB>", "k_cols<PLAIN>", "sort_positions",
                "k_rows_fused<STATS>", "k_rows_fused<PROJECT>", "k_rows_fused<LINESEARCH>",
                "k_cg_scalars", "k_fwd_fused256", "k_cg_update",
                "k_rows_fused<CROSS>", "k_cols_argmax", "k_zoom_argmax",
                "k_fwd_tile", "k_adjprb_tile")
last_error = _sig("ptycho_last_error", ctypes.c_char_p)
version = _sig("ptycho_version", ctypes.c_char_p)


class PtychoHipError(RuntimeError):
    pass


def check(rc):
    if rc != 0:
        raise PtychoHipError("libptychohip error %d: %s"
                             % (rc, last_error().decode("utf-8", "replace")))
