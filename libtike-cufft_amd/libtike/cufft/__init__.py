"""Alias so that ``import libtike.cufft as pt`` (the import line of every
reference script, e.g. ``/root/reference/tests/test_adjoint.py:5``) resolves to
the MI355X backend."""
from libtike.hipfft.ptycho import *  # noqa: F401,F403
from libtike.hipfft.frc import frc  # noqa: F401
from libtike.hipfft.gauge import illumination, fit_gauge, apply_gauge, fix_gauge  # noqa: F401
from libtike.hipfft.fit import fit_frames, accumulate_intensity, flag_frames  # noqa: F401
from libtike.hipfft.prepare import prepare_frames, initial_probe  # noqa: F401
from libtike.hipfft import __version__  # noqa: F401
