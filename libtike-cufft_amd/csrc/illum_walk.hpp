// illum_walk.hpp -- host walk of the illumination walk of k_illumination (k_gauge.hpp) and k_scan_map (k_dpc.hpp): the
// 64 x 16 tiles, the chunks of kIllChunk positions split and tested against the tile as illum_stage does it, the packed
// list in position order, and per thread the probe index of every tap of every channel, walked exactly as the kernels
// walk them.  No GPU involved: host_gauge.cpp (one channel, every position kept) and host_dpc.cpp map call it.
//
// errors counts the (position, tap, probe pixel, channel) contributions visited a number of times other than 1 (target
// pixel inside the object, position neither skipped by the split nor excluded by keep) or 0 (otherwise), visits in a
// tile that the overlap test had rejected included; visits is the number of contributions visited, skipped the number
// of positions that the split rejects or keep excludes.
#pragma once

#include <limits>
#include <vector>

#include "k_gauge.hpp"

namespace pty {

struct IllumWalk {
    long long errors = 0, visits = 0, skipped = 0;
};

// scan_in: [ptheta][nscan][2]; keep: [ptheta][nscan] flags, nullptr: every position kept
inline IllumWalk walk_illum(const int ptheta, const int nscan, const int nprb, const int nz, const int n, const int nval,
                            const float* scan_in, const unsigned char* keep) {
    IllumWalk w;
    const size_t npos = (size_t)ptheta * nscan;
    // k_scan_keep: NaN at the positions that keep excludes, so that the split skips them
    std::vector<float> scan(scan_in, scan_in + 2 * npos);
    for (size_t i = 0; keep && i < npos; ++i)
        if (!keep[i]) scan[2 * i] = scan[2 * i + 1] = std::numeric_limits<float>::quiet_NaN();
    const size_t per_pos = (size_t)4 * nprb * nprb * nval;
    auto slot = [&](int j, int a, int b, int iy, int ix, int c) {
        return (size_t)j * per_pos + (((size_t)(2 * a + b) * nprb + iy) * nprb + ix) * nval + c;
    };
    for (int t = 0; t < ptheta; ++t) {
        const float* sc = scan.data() + (size_t)t * nscan * 2;
        std::vector<unsigned char> visits((size_t)nscan * per_pos, 0);
        for (int y0 = 0; y0 < nz; y0 += kIllTileH)
            for (int x0 = 0; x0 < n; x0 += kIllTileW)
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
                    for (int i = 0; i < total; ++i)
                        for (int tid = 0; tid < 256; ++tid) {
                            const int lane = tid & 63, wave = tid >> 6;
                            const int X = x0 + lane, Y0 = y0 + wave * kIllRows;
                            int iy0, ix;
                            (void)illum_src(Y0, X, l_sy[i], l_sx[i], 0, 0, nprb, iy0, ix);
                            for (int r = 0; r < kIllRows; ++r) {
                                if (!(X < n && Y0 + r < nz)) continue;   // the kernels do not write this pixel
                                for (int a = 0; a < 2; ++a)
                                    for (int b = 0; b < 2; ++b) {
                                        const int iy = iy0 + r - a, jx = ix - b;
                                        if (!illum_inside(iy, jx, nprb)) continue;   // illum_amp2's zero, map_tap's select
                                        for (int c = 0; c < nval; ++c) {
                                            unsigned char& v = visits[slot(l_j[i], a, b, iy, jx, c)];
                                            if (v < 255) ++v;
                                            ++w.visits;
                                        }
                                    }
                            }
                        }
                }
        for (int j = 0; j < nscan; ++j) {
            int sy, sx;
            float fy, fx;
            const size_t p = (size_t)t * nscan + j;
            const bool vy = illum_split(scan_in[2 * p], sy, fy), vx = illum_split(scan_in[2 * p + 1], sx, fx);
            const bool valid = vy && vx && (!keep || keep[p]);
            if (!valid) ++w.skipped;
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b)
                    for (int iy = 0; iy < nprb; ++iy)
                        for (int ix = 0; ix < nprb; ++ix) {
                            const long long Y = (long long)sy + iy + a, X = (long long)sx + ix + b;
                            const int want = valid && Y < nz && X < n ? 1 : 0;
                            for (int c = 0; c < nval; ++c)
                                if (visits[slot(j, a, b, iy, ix, c)] != want) ++w.errors;
                        }
        }
    }
    return w;
}

}  // namespace pty
