// Host sweep of split_runs / min_run (run_split.hpp): the split of a windowed column launch into runs of sorted positions,
// at every np in 1 .. 5000, strips per launch {1, 2, 3, 16, 17, 32}, CUs {1, 8, 256, 304} and the workgroup targets the
// launchers ask for (2, 4 and 6 per CU: launch_adjwin, launch_gatherwin[_modes], do_adj_generic).  Checked: a run fits
// RunMeta (1 <= seglen <= kRunMax), the runs cover the positions (nseg * seglen >= np), none is empty ((nseg - 1) * seglen
// < np), and the result is that of the formula the four launch sites used to write out, kept below as the reference.
// No GPU involved; exit status 1 on an error.
#include <cstdio>

#include "run_split.hpp"

using namespace pty;

static int old_min_seglen(int np, int nstrips, int n_cu) {
    int m = 16;
    const long long fill = (long long)np * nstrips / (n_cu > 0 ? n_cu : 1);
    if (fill < m) m = fill < 4 ? 4 : (int)fill;
    return m;
}

static void old_split(int np, int nstrips, int n_cu, int wg_target, int& nseg, int& seglen) {
    nseg = (wg_target + nstrips - 1) / nstrips;
    if (nseg < 1) nseg = 1;
    seglen = (np + nseg - 1) / nseg;
    if (seglen < old_min_seglen(np, nstrips, n_cu)) seglen = old_min_seglen(np, nstrips, n_cu);
    if (seglen > kRunMax) seglen = kRunMax;
    nseg = (np + seglen - 1) / seglen;
}

int main() {
    const int strips[] = {1, 2, 3, 16, 17, 32}, cus[] = {1, 8, 256, 304}, per_cu[] = {2, 4, 6};
    long long cases = 0, errors = 0;
    int longest = 0;
    for (int n_cu : cus)
        for (int mult : per_cu)
            for (int nstrips : strips) {
                long long bad = 0;
                for (int np = 1; np <= 5000; ++np) {
                    const RunSplit rs = split_runs(np, nstrips, n_cu * mult, min_run(np, nstrips, n_cu, 16));
                    int nseg, seglen;
                    old_split(np, nstrips, n_cu, n_cu * mult, nseg, seglen);
                    bad += rs.seglen < 1 || rs.seglen > kRunMax;
                    bad += (long long)rs.nseg * rs.seglen < np;
                    bad += (long long)(rs.nseg - 1) * rs.seglen >= np;
                    bad += rs.nseg != nseg || rs.seglen != seglen;
                    if (rs.seglen > longest) longest = rs.seglen;
                    ++cases;
                }
                if (bad) std::printf("n_cu %d, %d workgroups per CU, %d strips: %lld errors\n", n_cu, mult, nstrips, bad);
                errors += bad;
            }
    std::printf("host_runsplit: %lld cases, longest run %d of %d, %lld errors\n", cases, longest, kRunMax, errors);
    return errors ? 1 : 0;
}
