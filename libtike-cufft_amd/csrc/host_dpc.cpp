// Host build of the index logic of k_dpc.hpp, walked as the kernels walk it.  Built by tests/test_dpc_cpu.py with clang++
// (no GPU involved).
//   host_dpc moments ptheta nscan ndet   the partition of k_frame_moments (frame_part_walk.hpp) and the signed frequencies
//                                        of every pixel a lane visits: "errors nwt nranges words sum_ky2 sum_kx2 sum_kykx",
//                                        the three sums over one frame's pixels as the walk met them
//   host_dpc map                         stdin "ptheta nscan nprb nz n nval", then ptheta * nscan pairs (row, column) as
//                                        the bit patterns of the float32 values, then ptheta * nscan keep flags (0 / 1):
//                                        k_scan_keep's replacement and k_scan_map's tiles, packed list and taps:
//                                        "errors visits skipped", errors counting the (position, tap, probe pixel, channel)
//                                        contributions visited a number of times other than 1 (target pixel inside the
//                                        object, position neither skipped nor excluded) or 0 (otherwise)
//   host_dpc edges nz n                  k_unwrap_setup<UnwGradSrc>'s edges: "errors tiles visits", errors counting the
//                                        edges whose d_e is not taken exactly once from each end, from the slots of its
//                                        two pixels in the order (p, q) and from the plane that unwrap_grad_field (the
//                                        helper UnwGradSrc::diff calls) names for the edge's direction: gy (plane 0) when
//                                        the two pixels differ in their row, gx (plane 1) when in their column.  The four
//                                        (a, b, vertical) triples are restated from the kernel, not shared with it: that
//                                        the kernel passes these triples, and gy as plane 0, is what the planted surfaces
//                                        of tests/test_hip_dpc.py check on the device
//   host_dpc                             sweeps the three over small shapes: "host_dpc: E errors, S shapes"
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

#include "frame_part_walk.hpp"
#include "k_dpc.hpp"

using namespace pty;

// ---- moments ---------------------------------------------------------------------------------------------------------------
struct MomHook : FrameWalkHook<MomPart> {
    int ndet;
    long long bad = 0, sky2 = 0, skx2 = 0, skykx = 0;
    std::vector<long long> freq;   // np.fft.fftfreq(ndet) * ndet, stated on its own
    explicit MomHook(int ndet_) : ndet(ndet_), freq((size_t)ndet_) {
        for (int r = 0; r < ndet; ++r) freq[(size_t)r] = r <= (ndet - 1) / 2 ? r : r - ndet;
    }
    void pixel(long long t, long long px) {
        const int row = (int)(px / ndet), col = (int)(px % ndet);
        const long long ky = moment_k(row, ndet), kx = moment_k(col, ndet);
        if (ky != freq[(size_t)row] || kx != freq[(size_t)col]) ++bad;
        if (t == 0) { sky2 += ky * ky; skx2 += kx * kx; skykx += ky * kx; }
    }
    long long errors() { return bad; }
};

static long long walk_moments(long long ptheta, long long nscan, int ndet, bool print) {
    MomHook hook(ndet);
    FramePlan p;
    long long errors = walk_frame_part<MomPart>(ptheta, nscan, (long long)ndet * ndet, p, hook);
    if (p.pwords != 0) ++errors;   // no pixel part
    if (print)
        std::printf("%lld %lld %lld %lld %lld %lld %lld\n", errors, p.nwt, p.nranges, p.fwords + p.pwords, hook.sky2, hook.skx2,
                    hook.skykx);
    return errors;
}

// ---- scan map ----------------------------------------------------------------------------------------------------------------
static long long walk_map(int ptheta, int nscan, int nprb, int nz, int n, int nval, const std::vector<float>& scan_in,
                          const std::vector<unsigned char>& keep, long long& nvisits, long long& skipped) {
    long long errors = 0;
    nvisits = skipped = 0;
    // k_scan_keep
    std::vector<float> scan(scan_in);
    for (size_t i = 0; i < (size_t)ptheta * nscan; ++i)
        if (!keep[i]) scan[2 * i] = scan[2 * i + 1] = std::numeric_limits<float>::quiet_NaN();
    const size_t per_pos = (size_t)4 * nprb * nprb * nval;
    for (int t = 0; t < ptheta; ++t) {
        const float* sc = scan.data() + (size_t)t * nscan * 2;
        std::vector<unsigned char> visits((size_t)nscan * per_pos, 0);
        for (int y0 = 0; y0 < nz; y0 += kIllTileH)
            for (int x0 = 0; x0 < n; x0 += kIllTileW)
                for (int c0 = 0; c0 < nscan; c0 += kIllChunk) {
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
                                if (!(X < n && Y0 + r < nz)) continue;   // the kernel does not write this pixel
                                const int iy = iy0 + r;
                                for (int a = 0; a < 2; ++a)
                                    for (int b = 0; b < 2; ++b) {
                                        if (!illum_inside(iy - a, ix - b, nprb)) continue;   // map_tap's select
                                        for (int c = 0; c < nval; ++c) {
                                            unsigned char& v = visits[(size_t)l_j[i] * per_pos +
                                                                      (((size_t)(2 * a + b) * nprb + (iy - a)) * nprb + (ix - b)) * nval + c];
                                            if (v < 255) ++v;
                                            ++nvisits;
                                        }
                                    }
                            }
                        }
                }
        for (int j = 0; j < nscan; ++j) {
            int sy, sx;
            float fy, fx;
            const float* raw = scan_in.data() + ((size_t)t * nscan + j) * 2;
            const bool vy = illum_split(raw[0], sy, fy), vx = illum_split(raw[1], sx, fx);
            const bool valid = vy && vx && keep[(size_t)t * nscan + j];
            if (!valid) ++skipped;
            for (int a = 0; a < 2; ++a)
                for (int b = 0; b < 2; ++b)
                    for (int iy = 0; iy < nprb; ++iy)
                        for (int ix = 0; ix < nprb; ++ix) {
                            const long long Y = (long long)sy + iy + a, X = (long long)sx + ix + b;
                            const int want = valid && Y < nz && X < n ? 1 : 0;
                            for (int c = 0; c < nval; ++c)
                                if (visits[(size_t)j * per_pos + (((size_t)(2 * a + b) * nprb + iy) * nprb + ix) * nval + c] != want)
                                    ++errors;
                        }
        }
    }
    return errors;
}

// ---- gradient edges ----------------------------------------------------------------------------------------------------------
static long long walk_edges(int nz, int n, long long& tiles, long long& visits) {
    long long errors = 0;
    visits = 0;
    const size_t plane = (size_t)nz * n;
    // visit of the edge e (0 left, 1 right, 2 up, 3 down) of pixel p from p's end
    std::vector<unsigned char> seen(plane * 4, 0);
    const int ntx = unwrap_tiles_x(n);
    tiles = unwrap_tiles(nz, n);
    const int slots = kUnwLdsH * kUnwLdsW;
    const int dy[4] = {0, 0, -1, 1}, dx[4] = {-1, 1, 0, 0};
    for (long long b = 0; b < tiles; ++b) {
        const int by = (int)(b / ntx), bx = (int)(b % ntx);
        std::vector<long long> lds(slots, -2);   // the pixel a slot holds, -1: outside the image, -2: not staged
        auto stage = [&](int y, int x) {
            const int s = unwrap_slot(y, x, by, bx);
            if (s < 0 || s >= slots) { ++errors; return; }
            lds[s] = unwrap_inside(y, x, nz, n) ? (long long)y * n + x : -1;
        };
        for (int tid = 0; tid < 256; ++tid) {
            int y, x, hy, hx;
            unwrap_own(tid, by, bx, y, x);
            for (int k = 0; k < kUnwVec; ++k) stage(y, x + k);
            if (unwrap_halo(tid, by, bx, hy, hx)) stage(hy, hx);
        }
        for (int tid = 0; tid < 256; ++tid) {
            int y, x;
            unwrap_own(tid, by, bx, y, x);
            const int have = !(y < nz) ? 0 : (n - x >= kUnwVec ? kUnwVec : (n - x > 0 ? n - x : 0));
            for (int k = 0; k < have; ++k) {
                const int c = unwrap_slot(y, x + k, by, bx);
                const size_t p = (size_t)y * n + (x + k);
                // the four calls of k_unwrap_setup, in its order: (a, b, vertical)
                const int call[4][3] = {{c - 1, c, 0}, {c, c + 1, 0}, {c - kUnwLdsW, c, 1}, {c, c + kUnwLdsW, 1}};
                for (int e = 0; e < 4; ++e) {
                    const int a = call[e][0], b2 = call[e][1];
                    const bool vertical = call[e][2] != 0;
                    if (a < 0 || b2 >= slots || lds[a] == -2 || lds[b2] == -2) { ++errors; continue; }
                    if (!unwrap_inside(y + dy[e], x + k + dx[e], nz, n)) {   // weight 0: the kernel takes no difference
                        if ((e == 0 || e == 2 ? lds[a] : lds[b2]) != -1) ++errors;
                        continue;
                    }
                    // the edge runs from its left / upper pixel to its right / lower one
                    const long long q = (long long)(y + dy[e]) * n + (x + k + dx[e]);
                    const long long lo = e == 0 || e == 2 ? q : (long long)p, hi = e == 0 || e == 2 ? (long long)p : q;
                    if (lds[a] != lo || lds[b2] != hi) ++errors;
                    const bool rows_differ = hi / n != lo / n, cols_differ = hi % n != lo % n;
                    if (rows_differ == cols_differ || vertical != rows_differ) ++errors;   // neighbours along one axis
                    if (unwrap_grad_field(vertical) != (rows_differ ? 0 : 1)) ++errors;    // gy across rows, gx across columns
                    if (seen[p * 4 + e] < 255) ++seen[p * 4 + e];
                    ++visits;
                }
            }
        }
    }
    for (int y = 0; y < nz; ++y)
        for (int x = 0; x < n; ++x)
            for (int e = 0; e < 4; ++e)
                if (seen[((size_t)y * n + x) * 4 + e] != (unwrap_inside(y + dy[e], x + dx[e], nz, n) ? 1 : 0)) ++errors;
    if (visits != 2 * ((long long)nz * (n - 1) + (long long)(nz - 1) * n)) ++errors;
    return errors;
}

int main(int argc, char** argv) {
    if (argc == 5 && !std::strcmp(argv[1], "moments")) {
        const long long ptheta = std::atoll(argv[2]), nscan = std::atoll(argv[3]);
        const int ndet = std::atoi(argv[4]);
        if (ptheta < 1 || nscan < 1 || ndet < 1) return 2;
        return walk_moments(ptheta, nscan, ndet, true) ? 1 : 0;
    }
    if (argc == 2 && !std::strcmp(argv[1], "map")) {
        int ptheta = 0, nscan = 0, nprb = 0, nz = 0, n = 0, nval = 0;
        if (std::scanf("%d %d %d %d %d %d", &ptheta, &nscan, &nprb, &nz, &n, &nval) != 6) return 2;
        if (ptheta < 1 || nscan < 1 || nprb < 1 || nz < 1 || n < 1 || nval < 1 || nval > kMapMaxVal) return 2;
        std::vector<float> scan((size_t)ptheta * nscan * 2);
        for (float& v : scan) {
            unsigned bits = 0;
            if (std::scanf("%u", &bits) != 1) return 2;
            std::memcpy(&v, &bits, sizeof v);
        }
        std::vector<unsigned char> keep((size_t)ptheta * nscan);
        for (unsigned char& k : keep) {
            int v = 0;
            if (std::scanf("%d", &v) != 1) return 2;
            k = (unsigned char)(v != 0);
        }
        long long visits, skipped;
        const long long errors = walk_map(ptheta, nscan, nprb, nz, n, nval, scan, keep, visits, skipped);
        std::printf("%lld %lld %lld\n", errors, visits, skipped);
        return errors ? 1 : 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "edges")) {
        const int nz = std::atoi(argv[2]), n = std::atoi(argv[3]);
        if (nz < 2 || n < 2) return 2;
        long long tiles, visits;
        const long long errors = walk_edges(nz, n, tiles, visits);
        std::printf("%lld %lld %lld\n", errors, tiles, visits);
        return errors ? 1 : 0;
    }
    if (argc != 1) return 2;
    long long errors = 0, shapes = 0;
    for (int ndet : {1, 2, 3, 15, 16, 18, 32, 48})
        for (long long nscan : {1LL, 33LL, 600LL}) {
            errors += walk_moments(2, nscan, ndet, false);
            ++shapes;
        }
    for (int nz = 2; nz <= 2 * kUnwTileH + 1; nz += 3)
        for (int n = 2; n <= 2 * kUnwTileW + 1; ++n) {
            long long tiles, visits;
            errors += walk_edges(nz, n, tiles, visits);
            ++shapes;
        }
    std::printf("host_dpc: %lld errors, %lld shapes\n", errors, shapes);
    return errors ? 1 : 0;
}
