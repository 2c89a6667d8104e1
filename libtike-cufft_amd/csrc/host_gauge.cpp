// Host build of the index logic of k_illumination (k_gauge.hpp): the walk of illum_walk.hpp with one channel and every
// position kept.  Built by tests/test_gauge_cpu.py with clang++ (no GPU involved).  stdin: "ptheta nscan nprb nz n", then
// ptheta * nscan pairs (row, column) as the bit patterns of the float32 values; stdout: "errors visits skipped", where
// errors counts the (position, tap, probe pixel) contributions visited a number of times other than 1 (target pixel
// inside the object, position not skipped) or 0 (otherwise), visits in a tile that the overlap test had rejected
// included, visits is the number of contributions visited and skipped the number of positions the split rejects.
#include <cstdio>
#include <cstring>
#include <vector>

#include "illum_walk.hpp"

using namespace pty;

int main() {
    int ptheta = 0, nscan = 0, nprb = 0, nz = 0, n = 0;
    if (std::scanf("%d %d %d %d %d", &ptheta, &nscan, &nprb, &nz, &n) != 5) return 2;
    if (ptheta < 1 || nscan < 1 || nprb < 1 || nz < 1 || n < 1) return 2;
    std::vector<float> scan((size_t)ptheta * nscan * 2);
    for (float& v : scan) {
        unsigned bits = 0;
        if (std::scanf("%u", &bits) != 1) return 2;
        std::memcpy(&v, &bits, sizeof v);
    }
    const IllumWalk w = walk_illum(ptheta, nscan, nprb, nz, n, 1, scan.data(), nullptr);
    std::printf("%lld %lld %lld\n", w.errors, w.visits, w.skipped);
    return 0;
}
