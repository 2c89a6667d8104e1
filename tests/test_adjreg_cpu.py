"""The register-resident overlap-add window of the object adjoint (``csrc/adjreg_map.hpp``) on the host:
``csrc/host_adjreg.cpp`` emulates the threads of one workgroup of ``k_cols_adjreg`` with the very arithmetic the kernel
uses -- ownership, retire, clamped tile rows, combine -- for ndet = 256 and 512, and compares every object pixel with a
four-tap scatter in float64.  No GPU involved."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "libtike-cufft_amd", "csrc")


def test_adjreg_window_on_host(tmp_path):
    exe = str(tmp_path / "pty_host_adjreg")
    subprocess.run(["/opt/rocm/lib/llvm/bin/clang++", "-std=c++17", "-O2",
                    os.path.join(CSRC, "host_adjreg.cpp"), "-o", exe], check=True)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.splitlines()
    assert lines[-1] == "OK", out.stdout
    # both sizes, full probe and nprb < ndet, and no pixel touched after a slide retired it
    assert sum("touched_after_retire=0 " in ln and ln.endswith(" ok") for ln in lines) == 4, out.stdout
    assert any(ln.startswith("N=256 nprb=256 G=12 RPG=24 HW=288 ") for ln in lines), out.stdout
    assert any(ln.startswith("N=512 nprb=512 G=25 RPG=22 HW=550 ") for ln in lines), out.stdout
