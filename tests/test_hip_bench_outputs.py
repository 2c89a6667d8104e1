"""``bench.py --dump-outputs``: the arrays the last timed step returned, written so that two builds can be compared output
for output.  Two runs with the same arguments write the same farplane bits and the same object up to float32 rounding (the
timed adjoint sums with float atomics, whose order varies: only option "deterministic" fixes it), and the files hold the
operators' results on the bench's own seeded inputs (checked against the oracle)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
R, STEP, NDET = 16, 8, 256


def run_bench(out):
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1",
           "--raster", str(R), "--step-px", str(STEP), "--dump-outputs", str(out)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    return json.loads(lines[0])


def load_complex(path):
    x = np.load(path)
    assert x.dtype == np.float32 and x.shape[-1] == 2
    return x[..., 0] + 1j * x[..., 1]


def test_dumped_outputs_are_reproducible_and_right(tmp_path):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = run_bench(tmp_path / "a")
    run_bench(tmp_path / "b")
    assert d["steps"] == 3 and d["ms_per_step"] > 0
    # a plain run (no --full): the headline figure and nothing that takes runs of its own
    assert d["metric"] == "fwd+adj patterns/s" and d["unit"] == "patterns/s" and d["higher_is_better"] is True
    assert d["dtype"] == "f32" and d["value"] == pytest.approx(R * R / (d["ms_per_step"] * 1e-3))
    assert d["full"] is False and "kernels" not in d["roofline"]
    assert not [k for k in d if k.startswith(("cg_", "cfg", "cpu_", "ndet", "generic", "bluestein", "ms_per_step_sorting"))]
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["farplane.npy", "object.npy"]
    assert sum(os.path.getsize(tmp_path / "a" / f) for f in names) <= 64e6
    assert np.array_equal(np.load(tmp_path / "a" / "farplane.npy"), np.load(tmp_path / "b" / "farplane.npy"))
    a, b = np.load(tmp_path / "a" / "object.npy"), np.load(tmp_path / "b" / "object.npy")
    assert np.abs(a - b).max() <= 5e-6 * np.abs(a).max()

    import bench
    from oracle import ptycho_oracle as op
    psi, prb, scan, nz, n = bench.workload(R, STEP, NDET)
    far = load_complex(tmp_path / "a" / "farplane.npy")
    idx = bench.dump_index(R * R, 32 << 20, NDET * NDET * 8)
    assert len(idx) == 64 and far.shape == (1, 64, NDET, NDET)
    want = op.fwd(psi, scan[:, idx], prb, NDET, "double")
    assert np.abs(far - want).max() < 2e-5 * np.abs(want).max()
    obj = load_complex(tmp_path / "a" / "object.npy")
    assert obj.shape == (1, nz, n)
    want = op.adj(op.fwd(psi, scan, prb, NDET, "double"), scan, prb, nz, n, "double")
    assert np.abs(obj - want).max() < 2e-5 * np.abs(want).max()
