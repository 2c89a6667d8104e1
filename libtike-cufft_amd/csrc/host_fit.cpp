// Host build of the partition of k_fit_frames / k_fit_fold (FitPart, k_fit.hpp), walked as the kernels walk it
// (frame_part_walk.hpp).  Built by tests/test_fit_cpu.py with clang++ (no GPU involved).  argv: "ptheta nscan npix";
// stdout: "errors words cap nranges nwt", where errors is the walk's count, words is what ptycho_fit_work_words returns
// and cap the most it may be, max(1 MiB, bytes of data / 4) / 8.
#include <cstdio>
#include <cstdlib>

#include "frame_part_walk.hpp"
#include "k_fit.hpp"

using namespace pty;

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const unsigned long long ptheta = std::strtoull(argv[1], nullptr, 10), nscan = std::strtoull(argv[2], nullptr, 10),
                             npix = std::strtoull(argv[3], nullptr, 10);
    if (!fit_sizes_ok(ptheta, nscan, npix)) return 2;
    FramePlan p;
    FrameWalkHook<FitPart> hook;   // lane 8 e stores sum e
    const long long errors = walk_frame_part<FitPart>((long long)ptheta, (long long)nscan, (long long)npix, p, hook);
    const unsigned long long quarter = ptheta * nscan * npix, mib = 1ull << 20;
    const unsigned long long cap = (quarter > mib ? quarter : mib) / 8;
    std::printf("%lld %lld %llu %lld %lld\n", errors, p.fwords + p.pwords, cap, p.nranges, p.nwt);
    return 0;
}
