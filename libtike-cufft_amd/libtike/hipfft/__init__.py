"""``libtike.hipfft`` -- MI355X (gfx950) backend with the ``libtike.cufft``
operator API (``/root/reference/src/libtike/cufft/__init__.py:1-9``)."""
from libtike.hipfft.ptycho import *  # noqa: F401,F403
from libtike.hipfft.frc import frc  # noqa: F401
from libtike.hipfft.gauge import illumination, fit_gauge, apply_gauge, fix_gauge  # noqa: F401
from libtike.hipfft.fit import fit_frames, accumulate_intensity, flag_frames  # noqa: F401
from libtike.hipfft.prepare import prepare_frames, initial_probe  # noqa: F401
from libtike.hipfft.unwrap import unwrap_phase, phase_residues  # noqa: F401
from libtike.hipfft.propagate import propagate, focus_series, object_pixel_size  # noqa: F401
from libtike.hipfft.resample import spline_prefilter, warp, rotate, zoom, shift, center_of_mass  # noqa: F401
from libtike.hipfft.dpc import frame_moments, scan_map, integrate_gradient, first_look, initial_object  # noqa: F401

__version__ = "0.1.0"
