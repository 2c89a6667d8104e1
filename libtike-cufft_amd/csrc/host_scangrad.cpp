// Host build of the index logic of k_scangrad.hpp, walked as the kernel walks it (sg_walk).  Built by
// tests/test_scan_grad_cpu.py with clang++ (no GPU involved).
//   host_scangrad walk nprb sy sx nz n   one position: "errors visits outside", errors counting the probe pixels visited a
//                                        number of times other than 1 and the taps whose element or in-object flag differs
//                                        from the plain statement psi[sy + i + a][sx + j + b], outside the taps that read 0
//   host_scangrad                        sweeps the probe sizes 1 .. 1024 of the test over positions inside the object,
//                                        overhanging every edge and corner, and wholly outside:
//                                        "host_scangrad: E errors, S shapes, V visits"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "k_scangrad.hpp"

using namespace pty;

struct SgCount { long long errors, visits, outside; };

static SgCount walk_position(int nprb, int sy, int sx, int nz, int n) {
    SgCount c{0, 0, 0};
    std::vector<int> seen((size_t)nprb * nprb, 0);
    const SgMap m = sg_map(nprb);
    if (m.cw * m.slots != kSgThreads || m.band_rows < 1 || m.band_rows > kSgBandRows || m.items != m.ncb * m.nband ||
        m.ncb * m.cw < nprb || m.nband * m.band_rows < nprb || (m.nband - 1) * m.band_rows >= nprb)
        ++c.errors;
    sg_walk(nprb, sy, sx, nz, n, [&](int i, int j, SgTapAt t00, SgTapAt t01, SgTapAt t10, SgTapAt t11) {
        ++c.visits;
        if (i < 0 || i >= nprb || j < 0 || j >= nprb) { ++c.errors; return; }
        ++seen[(size_t)i * nprb + j];
        const SgTapAt got[4] = {t00, t01, t10, t11};
        for (int k = 0; k < 4; ++k) {
            const long long Y = (long long)sy + i + k / 2, X = (long long)sx + j + k % 2;   // the plain statement
            const bool inside = Y >= 0 && Y < nz && X >= 0 && X < n;
            if (got[k].ok != inside) ++c.errors;
            else if (inside && got[k].at != (size_t)(Y * n + X)) ++c.errors;
            if (!inside) ++c.outside;
        }
    });
    for (int s : seen) c.errors += s != 1;
    return c;
}

int main(int argc, char** argv) {
    if (argc == 7 && !std::strcmp(argv[1], "walk")) {
        const int nprb = std::atoi(argv[2]), sy = std::atoi(argv[3]), sx = std::atoi(argv[4]), nz = std::atoi(argv[5]),
                  n = std::atoi(argv[6]);
        if (nprb < 1 || nprb > 2048 || sy < 0 || sx < 0 || nz < 1 || n < 1) return 2;
        const SgCount c = walk_position(nprb, sy, sx, nz, n);
        std::printf("%lld %lld %lld\n", c.errors, c.visits, c.outside);
        return c.errors ? 1 : 0;
    }
    if (argc != 1) return 2;
    long long errors = 0, shapes = 0, visits = 0;
    for (int nprb : {1, 2, 3, 15, 16, 17, 63, 64, 65, 255, 256, 257, 512, 1024}) {
        const int nz = nprb + 9, n = nprb + 14;   // the patch with its taps spans nprb + 1 rows and columns
        const int ys[] = {0, 3, nz - nprb - 1, nz - nprb, nz - 2, nz - 1, nz, nz + 5};   // inside, flush, over the bottom edge, outside
        const int xs[] = {0, 5, n - nprb - 1, n - nprb, n - 2, n - 1, n, n + 7};
        for (int sy : ys)
            for (int sx : xs) {
                if (sy < 0 || sx < 0) continue;
                if (nprb >= 512 && (sy == 3 || sx == 5 || sy == nz - 2 || sx == n - 2)) continue;   // keep the sweep short
                const SgCount c = walk_position(nprb, sy, sx, nz, n);
                errors += c.errors;
                visits += c.visits;
                ++shapes;
            }
    }
    std::printf("host_scangrad: %lld errors, %lld shapes, %lld visits\n", errors, shapes, visits);
    return errors ? 1 : 0;
}
