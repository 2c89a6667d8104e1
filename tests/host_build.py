"""The host programs of ``csrc/host_*.cpp`` for the ``test_*_cpu.py`` modules: the index logic of the kernels built with the
host compiler, always with ``-std=c++17 -O2 -Wall -Werror`` (no GPU involved)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libtike-cufft_amd", "csrc")
CXX = "/opt/rocm/lib/llvm/bin/clang++"
FLAGS = ["-std=c++17", "-O2", "-Wall", "-Werror"]


def build(name, tmp_dir):
    """Compile ``csrc/<name>.cpp`` into ``tmp_dir``; returns ``run(*args, stdin=None, check=True)``, which runs the program
    with ``args`` (each through ``str``) and ``stdin`` as its input and returns the ``CompletedProcess`` (text mode, output
    captured).  ``check``: a nonzero exit status raises."""
    exe = os.path.join(str(tmp_dir), "pty_" + name)
    subprocess.run([CXX] + FLAGS + [os.path.join(CSRC, name + ".cpp"), "-o", exe], check=True)

    def run(*args, stdin=None, check=True):
        return subprocess.run([exe] + [str(a) for a in args], input=stdin, capture_output=True, text=True, check=check)
    return run
