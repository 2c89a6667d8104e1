"""The rule that picks the column pass and the row pass of an operator or a CG stage (``csrc/col_path.hpp``) on the host:
``csrc/host_colpath.cpp`` sweeps every detector size with a Stockham plan x option window x option split x "the caller
allows split" x mode against the table of the ladders the launch sites used to write out, and checks what those ladders
only implied: split only at 256 and only with the window, the register window only at 256 / 512 and only for the object
adjoint, no windowed kernel where the window does not fit, 32-column strips only for the split forward pass.  The in-library
profiler cannot tell a windowed kernel from a plain one; this sweep can.  No GPU involved."""
import host_build


def test_column_path_rule_on_host(tmp_path):
    out = host_build.build("host_colpath", tmp_path)(check=False)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.splitlines()
    assert lines[-1] == "OK", out.stdout
    # 13 sizes x 2 x 2 x 2 options x 3 modes, each with 2 x 2 row-pass cases
    assert lines[-2] == "host_colpath: 1560 cases, 0 errors", out.stdout
