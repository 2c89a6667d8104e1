"""``bench.py``'s command line: a plain run is the headline figure alone, and every secondary figure waits for ``--full``
(what a plain line then holds is checked on the GPU in ``tests/test_hip_bench_outputs.py``)."""
import sys

import pytest


def parse(monkeypatch, *argv):
    import bench
    monkeypatch.setattr(sys, "argv", ["bench.py", *argv])
    return bench.parse()


def test_full_is_off_unless_asked_for(monkeypatch):
    a = parse(monkeypatch, "--gpus", "1", "--steps", "7", "--warmup", "2")
    assert a.full is False and (a.gpus, a.steps, a.warmup, a.dump_outputs) == (1, 7, 2, None)
    assert parse(monkeypatch, "--full").full is True


def test_options_of_the_secondary_figures_are_still_taken(monkeypatch):
    a = parse(monkeypatch, "--full", "--no-cpu", "--no-cg", "--no-cfg3", "--no-shard", "--cg-iters", "3", "--cfg3-iters", "2")
    assert a.full and a.no_cpu and a.no_cg and a.no_cfg3 and a.no_shard and (a.cg_iters, a.cfg3_iters) == (3, 2)
    a = parse(monkeypatch, "--no-cpu", "--no-cg")           # accepted without --full, where they change nothing
    assert a.full is False


def test_steps_must_be_positive(monkeypatch):
    with pytest.raises(SystemExit):
        parse(monkeypatch, "--steps", "0")
