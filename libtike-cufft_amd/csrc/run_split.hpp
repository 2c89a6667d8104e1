// run_split.hpp -- how a launch of a windowed column kernel is cut into runs of sorted positions.
// Plain C++ (no HIP types), so that host_runsplit.cpp can sweep it on the CPU: the clamp to kRunMax below is all that keeps
// load_run (ptycho_common.hpp) inside RunMeta's arrays.
#pragma once

namespace pty {

constexpr int kRunMax = 128;   // positions of one run = entries of RunMeta

// Shortest run a workgroup takes, given the floor the launchers ask for (host_ops.hpp, min_seglen): problems too small to
// give every CU a workgroup at that floor take shorter runs, down to 4.
inline int min_run(int np, int nstrips, int n_cu, int floor_len) {
    int m = floor_len < 1 ? 1 : floor_len;
    const long long fill = (long long)np * nstrips / (n_cu > 0 ? n_cu : 1);   // run length that gives one workgroup per CU
    if (fill < m) m = fill < 4 ? 4 : (int)fill;
    return m;
}

struct RunSplit {
    int nseg, seglen;   // nseg runs of seglen positions (the last one may be shorter); grid = nstrips * nseg
};

// np > 0 positions for each of nstrips > 0 strips, about wg_target workgroups in all, runs of min_seg .. kRunMax positions
inline RunSplit split_runs(int np, int nstrips, int wg_target, int min_seg) {
    int nseg = (wg_target + nstrips - 1) / nstrips;
    if (nseg < 1) nseg = 1;
    int seglen = (np + nseg - 1) / nseg;
    if (seglen < min_seg) seglen = min_seg;
    if (seglen > kRunMax) seglen = kRunMax;
    return RunSplit{(np + seglen - 1) / seglen, seglen};
}

}  // namespace pty
