"""Scans that drive the LDS window of ``k_cols_gatherwin`` (csrc/k_cols_window.hpp) over its edges, and a model of the
window's bookkeeping that proves they do.

The kernel keeps the object rows ``[Ylo, Yhi)`` of a strip at slot ``Y % H`` (``H = ndet + 8``; row ``H`` mirrors row 0) and
moves that window along a run of sorted positions.  ``events`` restates, in plain Python, how the launchers cut the sorted
order into runs (``run_split``: csrc/run_split.hpp with the targets of csrc/host_ops.hpp and csrc/host_cg.hpp) and what
``prepare_issue`` decides for every position of a run, and counts the decisions.  It is test code: it only shows that a
scan reaches an event (tests/test_gatherwin_cases_cpu.py asserts it without a GPU, tests/test_hip_gatherwin.py again
with the device's CU count).  Expected values never come from here; they come from ``oracle.ptycho_oracle``.

An event is counted only at a position that follows a valid position of the same run, i.e. where the window holds
something: the first fill of a run is none of them.
"""
import functools

import numpy as np

BUCKET = 4                                          # kBucketPx (csrc/adjreg_map.hpp): column bucket of the sort key, window slack
RUN_MAX = 128                                       # kRunMax (csrc/run_split.hpp)
PLAN_T = {128: 8, 192: 8, 256: 16, 512: 32}         # threads per transform, Plan<N>::T (csrc/fft_core.hpp)
STRIP_C = {128: 32, 192: 16, 256: 16, 512: 16}      # ColCfg<N>::C (csrc/ptycho_common.hpp)
SPLIT_FWD_C = 32                                    # kSplitFwdC (csrc/col_path.hpp)

COUNTERS = ("thread", "loop", "thread_max", "loop_min", "mirror_thread", "mirror_loop", "lastslot_thread", "lastslot_loop",
            "ra_eq_yhi", "reanchor_rows", "reanchor_cols", "reanchor_angle", "nothing_new", "skipped_inside")
ROWS_COUNTERS = ("thread", "loop", "thread_max", "loop_min", "mirror_thread", "mirror_loop", "lastslot_thread",
                 "lastslot_loop", "ra_eq_yhi", "reanchor_rows", "nothing_new")
COLS_COUNTERS = ("reanchor_cols", "reanchor_angle", "skipped_inside")


def launcher(name, ndet):
    """``(C, T, wg_mult)`` of a launch of ``k_cols_gatherwin``: strip width, threads per transform and workgroups per CU
    the launcher aims at.  ``fwd`` / ``adj_probe``: ``launch_gatherwin`` un-split; ``fwd_split`` / ``adj_probe_split``: the
    split passes of ndet 256; ``modes``: ``launch_gatherwin_modes``."""
    c, t = STRIP_C[ndet], PLAN_T[ndet]
    if name in ("fwd", "adj_probe", "modes"):
        return c, t, 4
    assert ndet == 256, "the split passes exist at 256 only"
    if name == "fwd_split":
        return SPLIT_FWD_C, t, 2
    if name == "adj_probe_split":
        return c, t, 6
    raise KeyError(name)


def run_split(np_, nstrips, n_cu, wg_mult, floor=16):
    """``(nseg, seglen)`` of ``split_runs(np, nstrips, wg_mult * n_cu, min_run(np, nstrips, n_cu, floor))``."""
    m = max(floor, 1)
    fill = np_ * nstrips // max(n_cu, 1)
    if fill < m:
        m = 4 if fill < 4 else fill
    nseg = max((wg_mult * n_cu + nstrips - 1) // nstrips, 1)
    seglen = min(max((np_ + nseg - 1) // nseg, m), RUN_MAX)
    return (np_ + seglen - 1) // seglen, seglen


def strip_range(ndet, nprb, C):
    """``(strip0, nstrips)``: the strips of C detector columns that the probe touches (csrc/host_ops.hpp)."""
    pad = (ndet - nprb) // 2
    return pad // C, (pad + nprb - 1) // C - pad // C + 1


def decode(scan):
    """``decode_xy`` on a float32 scan ``[..., 2]``: integer rows and columns (0 where skipped) and the valid mask."""
    ip = np.trunc(np.asarray(scan, dtype=np.float32))
    valid = ~((ip[..., 0] < 0) | (ip[..., 1] < 0))
    sy = np.where(valid, ip[..., 0], 0).astype(np.int64)
    sx = np.where(valid, ip[..., 1], 0).astype(np.int64)
    return sy, sx, valid


def sorted_order(scan, sort_chunks=1):
    """Processing order of ``k_rank_positions``: chunk * ntheta + angle, then column bucket, then row; skipped positions last
    in their (chunk, angle) group; ties by index."""
    ntheta, nscan = scan.shape[:2]
    sy, sx, valid = (a.reshape(-1) for a in decode(scan))
    total = ntheta * nscan
    p = np.arange(total)
    pc = (total + sort_chunks - 1) // sort_chunks
    u = (p // pc) * ntheta + p // nscan
    keys = [(int(u[i]), 0 if valid[i] else 1, int(sx[i]) // BUCKET if valid[i] else 0, int(sy[i]) if valid[i] else 0, i)
            for i in range(total)]
    return [k[-1] for k in sorted(keys)]


def events(scan, geometry, C, T, n_cu, wg_mult, chunk=0):
    """Counters of what the window update does over all runs of one operator call.  ``geometry`` starts with ``(ndet, nprb)``;
    ``chunk``: positions per launch of the adjoints (option "chunk"; 0: one launch).  Also returns ``runs``, the run lengths."""
    ndet, nprb = geometry[:2]
    H, WC, NT = ndet + 8, C + BUCKET, T * C
    r = NT // WC
    nscan = scan.shape[1]
    sy, sx, valid = (a.reshape(-1) for a in decode(scan))
    order = sorted_order(scan)
    total = len(order)
    _, nstrips = strip_range(ndet, nprb, C)
    ev = dict.fromkeys(COUNTERS, 0)
    runs = []
    step = chunk if chunk > 0 else total
    for k0 in range(0, total, step):
        k1 = min(k0 + step, total)
        _, seglen = run_split(k1 - k0, nstrips, n_cu, wg_mult)
        for kb in range(k0, k1, seglen):
            ke = min(kb + seglen, k1)
            runs.append(ke - kb)
            t_w, bucket, ylo, yhi = -1, 0, 0, 0
            for k in range(kb, ke):
                p = order[k]
                if not valid[p]:
                    if t_w >= 0 and any(valid[order[j]] for j in range(k + 1, ke)):
                        ev["skipped_inside"] += 1
                    continue
                t = p // nscan
                ra, rb = int(sy[p]), int(sy[p]) + nprb + 1
                live = t_w >= 0
                if t != t_w or int(sx[p]) // BUCKET != bucket:          # colfit false
                    if live:
                        ev["reanchor_angle" if t != t_w else "reanchor_cols"] += 1
                    t_w, bucket, ylo, yhi = t, int(sx[p]) // BUCKET, ra, ra
                elif ra < ylo or ra > yhi:
                    ev["reanchor_rows"] += live
                    ylo = yhi = ra
                else:
                    ev["ra_eq_yhi"] += live and ra == yhi
                    ylo = ra
                if rb > yhi:
                    cnt = (rb - yhi) * WC
                    path = "thread" if cnt <= NT else "loop"
                    if live:
                        ev[path] += 1
                        ev["thread_max"] += cnt == r * WC
                        ev["loop_min"] += cnt == (r + 1) * WC
                        ev["mirror_" + path] += any(y % H == 0 for y in range(yhi, rb))
                        ev["lastslot_" + path] += any(y % H == H - 1 for y in range(yhi, rb))
                    yhi = rb
                else:
                    ev["nothing_new"] += live
    ev = {k: int(v) for k, v in ev.items()}
    ev["runs"] = runs
    return ev


def _fractions(rng, count, zero_from):
    """multiples of 1/256 (exact in float32 beside an integer part below 2^15), every fifth exactly 0"""
    f = rng.integers(1, 256, count) / 256.0
    f[zero_from::5] = 0.0
    return f


def rows(ndet, nprb, C):
    """One angle, one column bucket, ascending rows: ``(ndet, nprb, ntheta, nz, n, scan)``, scan float32.

    With ``r = NT // WC`` rows per trip of the per-thread load path (``NT = T C`` threads, ``WC = C + 4`` window columns) the row
    gaps are 0, 1, r, r + 1 (the boundary between the load paths), nprb - 1, nprb, nprb + 1 (``Ra == Yhi``), nprb + 2
    (re-anchor), H - 1, H, H + 1 (the same slots, other rows) and 2 H + 3, each twice in succession, then the sequence
    reversed.  Two "cross" segments follow, ten positions one row apart whose last cached row steps over a multiple of H
    (slots H - 1 and 0, and so the mirror row, through the per-thread path); one position between them puts the two
    segments at different offsets to the run boundaries, so that no run length hides both.  Six positions five rows apart
    end the scan; the last two hang over the bottom edge."""
    T, H, WC = PLAN_T[ndet], ndet + 8, C + BUCKET
    r = (T * C) // WC
    gaps = [0, 1, r, r + 1, nprb - 1, nprb, nprb + 1, nprb + 2, H - 1, H, H + 1, 2 * H + 3]
    steps = [g for g in gaps for _ in range(2)]
    sy = [3]
    for g in steps + steps[::-1]:
        sy.append(sy[-1] + g)
    for seg in range(2):
        a = sy[-1] + 2 * H
        a += (H - 5 - (a + nprb)) % H              # last cached row a + nprb at slot H - 5: rows H - 4 .. H - 1, 0 .. 4 slide in
        sy += [a + i for i in range(10)]
        if seg == 0:
            sy.append(sy[-1] + 7)
    sy += [sy[-1] + 5 * (i + 1) for i in range(6)]
    sy = np.array(sy, dtype=np.float64)
    rng = np.random.default_rng(1000 + ndet + C)
    count = len(sy)
    ycoord = sy + _fractions(rng, count, 0)
    xcoord = 8.0 + rng.integers(0, BUCKET, count) + _fractions(rng, count, 2)
    nz = int(sy[-3]) + nprb + 3                     # the last two positions end 3 and 8 rows below the object
    scan = np.stack([ycoord, xcoord], -1)[None].astype(np.float32)
    return ndet, nprb, 1, nz, ndet + 32, scan


# Positions per angle and skipped positions of angle 0 of cols().  The last valid position of angle 0, its skipped positions
# and the first position of angle 1 must share a run under every launcher the case goes through: with runs of 4, 5, 6 and 11
# positions on 256 CUs that leaves few counts, and 43 with two skipped positions is the one below 56 that serves all four
# detector sizes (tests/test_gatherwin_cases_cpu.py holds it to that).
COLS_NSCAN = 43
COLS_NSKIP0 = 2


def cols(ndet, nprb):
    """Two angles, ``nprb < ndet`` with a padding that is no multiple of the strip width (the first strip starts inside the
    padding): ``(ndet, nprb, ntheta, nz, n, scan)``.  Rows ascend by 3 to 9 in scan order; the columns fall into five buckets
    with every offset 0..3 inside a bucket and ``fx`` exactly 0 on some; the taps of the eight positions of the last bucket
    fall off the right edge.  Skipped positions (negative row, negative column or both): two in angle 0, three in angle 1;
    the position at row -0.25 is not skipped and has a negative fraction.  Skipped positions sort last in their angle, so
    those of angle 0 sit inside the run that continues into angle 1."""
    assert nprb < ndet
    nscan = COLS_NSCAN
    n = nprb + 40
    rng = np.random.default_rng(2000 + ndet)
    scan = np.zeros((2, nscan, 2))
    buckets = np.array([4, 8, 12, 16, n - nprb + 4])       # first column of each; the last: sx + nprb + 1 > n
    top = 0
    for t in range(2):
        sy = 2 + np.cumsum(rng.integers(3, 10, nscan))
        b = np.arange(nscan) % 5
        edge = np.nonzero(b == 4)[0]
        b[edge[4:]] = 1                                      # four positions per angle in the edge bucket
        scan[t, :, 0] = sy + _fractions(rng, nscan, t)
        scan[t, :, 1] = buckets[b] + np.arange(nscan) // 5 % BUCKET + _fractions(rng, nscan, 3)
        top = max(top, int(sy.max()))
    assert (np.trunc(scan[..., 1]) + nprb + 1 > n).sum() == 8
    scan[0, 0] = [-0.25, 9.5]                                # trunc -> -0.0: valid, negative fraction
    skipped = {0: [(5, (-1.5, 9.25)), (20, (30.5, -2.25)), (33, (-3.0, -1.0))][:COLS_NSKIP0],
               1: [(7, (-1.5, 17.0)), (21, (44.75, -2.25)), (40, (-2.5, -0.5))]}
    for t, items in skipped.items():
        for i, v in items:
            scan[t, i] = v
    return ndet, nprb, 2, top + nprb + 2, n, scan.astype(np.float32)


# ---- the cases of tests/test_hip_gatherwin.py and the launchers each one is there for ------------------------------------
CASES = {
    "rows128": (rows, 128, 128, 32), "rows192": (rows, 192, 192, 16), "rows256": (rows, 256, 256, 16),
    "rows256w": (rows, 256, 256, SPLIT_FWD_C),              # r = 14: the 32-column strips of the split forward pass
    "rows512": (rows, 512, 512, 16),
    "cols128": (cols, 128, 100), "cols192": (cols, 192, 150), "cols256": (cols, 256, 200), "cols512": (cols, 512, 470),
}

# (case, launchers whose counters it must reach, option "chunk" of the adjoints)
PLANS = [
    ("rows256", ("adj_probe_split",), 0),
    ("rows256w", ("fwd_split",), 0),
    ("rows256", ("fwd", "adj_probe", "modes"), 0),
    ("rows256", ("adj_probe_split",), 37),                  # k_begin != 0, a chunk boundary inside the gap sequence
    ("rows512", ("fwd", "adj_probe", "modes"), 0),
    ("rows192", ("fwd", "adj_probe"), 0),
    ("rows128", ("fwd", "adj_probe"), 0),
    ("cols256", ("fwd_split", "adj_probe_split"), 0),
    ("cols256", ("fwd", "adj_probe", "modes"), 0),
    ("cols512", ("fwd", "adj_probe"), 0),
    ("cols192", ("fwd", "adj_probe"), 0),
    ("cols128", ("fwd", "adj_probe"), 0),
]


@functools.lru_cache(maxsize=None)
def case_scan(name):
    """``(ndet, nprb, ntheta, nz, n, scan)`` of a named case; the scan is shared and read-only."""
    build, *args = CASES[name]
    out = build(*args)
    out[5].setflags(write=False)
    return out


def plan_events(case, launch, n_cu, chunk=0):
    """``events`` of a case under a launcher; the forward operator is one launch whatever option "chunk" says"""
    C, T, wg_mult = launcher(launch, case[0])
    return events(case[5], case[:5], C, T, n_cu, wg_mult, 0 if launch.startswith("fwd") or launch == "modes" else chunk)


def assert_events(name, launch, ev):
    for k in ROWS_COUNTERS if name.startswith("rows") else COLS_COUNTERS:
        assert ev[k] >= 1, "%s through %s never reaches %s: %s" % (name, launch, k, {c: ev[c] for c in COUNTERS})
    assert max(ev["runs"]) <= RUN_MAX, "a run longer than RunMeta"
