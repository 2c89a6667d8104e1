// Host build of the index logic of k_illumination (k_gauge.hpp): tiles, the split and the overlap test of every position,
// the packed list in position order, and per thread the probe index of every tap, walked exactly as the kernel walks
// them.  Built by tests/test_gauge_cpu.py with clang++ (no GPU involved).  stdin: "ptheta nscan nprb nz n", then
// ptheta * nscan pairs (row, column) as the bit patterns of the float32 values; stdout: "errors visits skipped", where
// errors counts the (position, tap, probe pixel) contributions visited a number of times other than 1 (target pixel
// inside the object, position not skipped) or 0 (otherwise), visits in a tile that the overlap test had rejected
// included, visits is the number of contributions visited and skipped the number of positions the split rejects.
#include <cstdio>
#include <cstring>
#include <vector>

#include "k_gauge.hpp"

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
    long long errors = 0, nvisits = 0, skipped = 0;
    const size_t per_pos = (size_t)4 * nprb * nprb;
    for (int t = 0; t < ptheta; ++t) {
        const float* sc = scan.data() + (size_t)t * nscan * 2;
        std::vector<unsigned char> visits((size_t)nscan * per_pos, 0);
        for (int y0 = 0; y0 < nz; y0 += kIllTileH) {
            for (int x0 = 0; x0 < n; x0 += kIllTileW) {
                for (int c0 = 0; c0 < nscan; c0 += kIllChunk) {
                    // the packed list of this chunk: threads in order, i.e. positions in order
                    int l_j[kIllChunk], l_sy[kIllChunk], l_sx[kIllChunk], total = 0;
                    for (int tid = 0; tid < kIllChunk && c0 + tid < nscan; ++tid) {
                        int sy, sx;
                        float fy, fx;
                        const size_t p = (size_t)(c0 + tid);
                        const bool vy = illum_split(sc[2 * p], sy, fy), vx = illum_split(sc[2 * p + 1], sx, fx);
                        if (vy && vx && illum_overlaps(sy, sx, nprb, y0, x0, nz, n)) {
                            l_j[total] = c0 + tid; l_sy[total] = sy; l_sx[total] = sx;
                            ++total;
                        }
                    }
                    for (int i = 0; i < total; ++i) {
                        for (int tid = 0; tid < 256; ++tid) {
                            const int lane = tid & 63, wave = tid >> 6;
                            const int X = x0 + lane, Y0 = y0 + wave * kIllRows;
                            int iy0, ix;
                            (void)illum_src(Y0, X, l_sy[i], l_sx[i], 0, 0, nprb, iy0, ix);
                            for (int r = 0; r < kIllRows; ++r) {
                                if (!(X < n && Y0 + r < nz)) continue;   // the kernel does not write this pixel
                                for (int a = 0; a < 2; ++a)
                                    for (int b = 0; b < 2; ++b) {
                                        const int iy = iy0 + r - a, jx = ix - b;
                                        if (!illum_inside(iy, jx, nprb)) continue;
                                        unsigned char& v = visits[(size_t)l_j[i] * per_pos + ((size_t)(2 * a + b) * nprb + iy) * nprb + jx];
                                        if (v < 255) ++v;
                                        ++nvisits;
                                    }
                            }
                        }
                    }
                }
            }
        }
        for (int j = 0; j < nscan; ++j) {
            int sy, sx;
            float fy, fx;
            const bool vy = illum_split(sc[2 * (size_t)j], sy, fy), vx = illum_split(sc[2 * (size_t)j + 1], sx, fx);
            const bool valid = vy && vx;
            if (!valid) ++skipped;
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b)
                    for (int iy = 0; iy < nprb; ++iy)
                        for (int ix = 0; ix < nprb; ++ix) {
                            const long long Y = (long long)sy + iy + a, X = (long long)sx + ix + b;
                            const int want = valid && Y < nz && X < n ? 1 : 0;
                            if (visits[(size_t)j * per_pos + ((size_t)(2 * a + b) * nprb + iy) * nprb + ix] != want) ++errors;
                        }
        }
    }
    std::printf("%lld %lld %lld\n", errors, nvisits, skipped);
    return 0;
}
