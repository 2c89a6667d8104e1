"""The LDS-DMA tile ring of the split object adjoint (``AdjRingCfg`` in ``csrc/adjreg_map.hpp``) on the host:
``csrc/host_adjdma.cpp`` walks every wave, request and lane of a workgroup of ``k_cols_adjreg`` at ndet = 256 with the
functions the kernel uses, fills an emulated ring lane-linearly as the hardware does and reads it back as the threads
do: every tile element requested once from a 16-byte-aligned source, inside its own wave's segment, and every thread's
16 reads the rows ``Fft::load`` names for it.  No GPU involved."""
import host_build


def test_adjreg_tile_ring_on_host(tmp_path):
    out = host_build.build("host_adjdma", tmp_path)(check=False)
    assert out.returncode == 0, out.stdout
    lines = out.stdout.splitlines()
    assert lines[-1] == "OK", out.stdout
    # split and un-split rows; four waves of eight 1-KiB requests, one 8-KiB segment each
    assert sum(" bad=0 ok" in ln for ln in lines) == 2, out.stdout
    assert any(ln.startswith("N=256 split waves=4 requests=8 segment=8192 B ring=32768 B row_step=32 ") for ln in lines), out.stdout
    assert any(ln.startswith("N=256 unsplit waves=4 requests=8 segment=8192 B ring=32768 B row_step=32 ") for ln in lines), out.stdout
