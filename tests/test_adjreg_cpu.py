"""The register-resident overlap-add window of the object adjoint (``csrc/adjreg_map.hpp``) on the host:
``csrc/host_adjreg.cpp`` emulates the threads of one workgroup of ``k_cols_adjreg`` with the very arithmetic the kernel
uses -- ownership, retire, clamped tile rows, combine -- for ndet = 256 and 512, and compares every object pixel with a
four-tap scatter in float64.  No GPU involved."""
import host_build


def test_adjreg_window_on_host(tmp_path):
    out = host_build.build("host_adjreg", tmp_path)(check=False)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.splitlines()
    assert lines[-1] == "OK", out.stdout
    # both sizes, full probe and nprb < ndet, and no pixel touched after a slide retired it
    assert sum("touched_after_retire=0 " in ln and ln.endswith(" ok") for ln in lines) == 4, out.stdout
    assert any(ln.startswith("N=256 nprb=256 G=12 RPG=24 HW=288 ") for ln in lines), out.stdout
    assert any(ln.startswith("N=512 nprb=512 G=25 RPG=22 HW=550 ") for ln in lines), out.stdout
