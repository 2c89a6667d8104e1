"""The scans of tests/gatherwin_cases.py reach the window events they were built for -- conditions on the inputs, checked with
the model of the bookkeeping alone, for every case and launcher that tests/test_hip_gatherwin.py sends them through, at the
256 compute units of an MI355X.  No GPU, no code under test: a case that misses a counter is changed, not the condition."""
import numpy as np
import pytest

import gatherwin_cases as gc

N_CU = 256


@pytest.mark.parametrize("plan", gc.PLANS, ids=lambda p: "%s-%s-%s" % (p[0], "+".join(p[1]), p[2] or "whole"))
def test_case_reaches_its_events(plan):
    name, launchers, chunk = plan
    case = gc.case_scan(name)
    for launch in launchers:
        ev = gc.plan_events(case, launch, N_CU, chunk)
        print(name, launch, {k: v for k, v in ev.items() if k != "runs"}, "runs of", sorted(set(ev["runs"])))
        gc.assert_events(name, launch, ev)


def test_run_split_restates_the_launchers():
    """split_runs / min_run by hand: 55 positions x 16 strips on 256 CUs cannot fill the chip at runs of 16 -> runs of 4; 32
    strips -> 6; 4096 positions -> 64 workgroups of 64; the clamp to 128."""
    assert gc.run_split(55, 16, 256, 4) == (14, 4)
    assert gc.run_split(55, 32, 256, 4) == (10, 6)
    assert gc.run_split(4096, 16, 256, 4) == (64, 64)
    assert gc.run_split(4096, 8, 256, 2) == (64, 64)
    assert gc.run_split(100000, 16, 256, 4) == (782, 128)
    assert gc.run_split(300, 16, 256, 6) == (19, 16)


def test_strip_range_and_rows_per_trip():
    assert gc.strip_range(256, 256, 16) == (0, 16) and gc.strip_range(256, 200, 16) == (1, 14)
    assert gc.strip_range(256, 200, 32) == (0, 8) and gc.strip_range(512, 470, 16) == (1, 30)
    assert gc.strip_range(192, 150, 16) == (1, 10) and gc.strip_range(128, 100, 32) == (0, 4)
    # rows per trip of the per-thread load path, NT // WC
    for ndet, launch, want in ((256, "fwd", 12), (256, "fwd_split", 14), (512, "fwd", 25), (192, "fwd", 6), (128, "fwd", 7)):
        C, T, _ = gc.launcher(launch, ndet)
        assert (T * C) // (C + gc.BUCKET) == want


def test_sorted_order_and_decode():
    scan = np.array([[[9.5, 8.0], [3.0, 9.0], [-1.5, 2.0], [-0.25, 13.0], [3.0, 4.5], [3.0, 8.5]],
                     [[2.0, -0.5], [1.0, 1.0], [7.0, -3.0], [0.0, 0.0], [5.0, 1.0], [4.0, 40.0]]], np.float32)
    sy, sx, valid = gc.decode(scan)
    assert valid.tolist() == [[True, True, False, True, True, True], [True, True, False, True, True, True]]
    assert sy[0, 3] == 0 and sx[1, 0] == 0
    # angle 0: bucket 1 (4.5), bucket 2 rows 3 (index 1 before 5: tie by index), 9; bucket 3; skipped last; then angle 1
    assert gc.sorted_order(scan) == [4, 1, 5, 0, 3, 2, 9, 7, 6, 10, 11, 8]


def test_rows_layout():
    ndet, nprb, ntheta, nz, n, scan = gc.rows(256, 256, 16)
    assert scan.dtype == np.float32 and scan.shape == (1, 76, 2) and n == 288
    sy, sx, valid = gc.decode(scan)
    assert valid.all() and len(set((sx[0] // gc.BUCKET).tolist())) == 1
    gaps = np.diff(sy[0])
    assert (gaps >= 0).all()
    for g in (0, 1, 12, 13, 255, 256, 257, 258, 263, 264, 265, 531):
        assert (gaps == g).sum() >= 4, g
    assert (sy[0] + nprb + 1 > nz).sum() == 2
    frac = scan[0] - np.trunc(scan[0])
    assert (frac[:, 0] == 0).sum() >= 15 and (frac[:, 1] == 0).sum() >= 15


def test_cols_layout():
    for ndet, nprb in ((256, 200), (192, 150), (512, 470), (128, 100)):
        _, _, ntheta, nz, n, scan = gc.cols(ndet, nprb)
        sy, sx, valid = gc.decode(scan)
        assert ntheta == 2 and (~valid[0]).sum() == 2 and (~valid[1]).sum() == 3
        assert scan[0, 0, 0] == np.float32(-0.25) and valid[0, 0]
        assert ((sx + nprb + 1 > n) & valid).sum() == 8
        assert len(set((sx[valid] // gc.BUCKET).tolist())) == 5
        assert set((sx[valid] % gc.BUCKET).tolist()) == {0, 1, 2, 3}
        assert ((ndet - nprb) // 2) % gc.STRIP_C[ndet] != 0
