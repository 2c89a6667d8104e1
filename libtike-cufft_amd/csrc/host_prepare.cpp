// Host build of the partition of k_prepare / k_prepare_fold (PrepPart, walked by frame_part_walk.hpp as the kernels walk
// it) and of the crop / shift index map (k_prepare.hpp).  No GPU involved.
//
//   host_prepare                              the walk and the map at a list of shapes of its own; exit status 1 on an error
//   host_prepare walk ptheta nscan ndet       stdout "errors words nranges nwt": errors counts the (frame, pixel) pairs
//                                             visited a number of times other than 1, the words of `work` written or folded
//                                             a number of times other than 1, the words of frames / pixels / mask without
//                                             exactly one writer and the centred pixels not hit exactly once by the shift
//   host_prepare map ndet bin H W y0 x0       stdout one line per output pixel in the layout of data: "oy ox first last
//                                             aligned": the centred pixel it holds, the offsets of the first and the last
//                                             raw pixel of its bin in the frame (-1: outside), and whether the vector
//                                             loads apply to this geometry
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "frame_part_walk.hpp"
#include "k_prepare.hpp"

using namespace pty;

// what preparation adds to the walk: the shift hits every centred pixel once, range 0 of angle 0 writes the mask, and lanes
// 0, 16, 32, 48 store the frame's four figures in the order of prep_lane_col
struct PrepWalkHook : FrameWalkHook<PrepPart> {
    static constexpr int kStoreStride = 16;
    const int ndet;
    long long bad = 0;
    std::vector<unsigned> cvis;
    std::vector<unsigned char> mask;
    explicit PrepWalkHook(const int n) : ndet(n), cvis((size_t)n * n, 0), mask((size_t)n * n, 0) {}
    int col(const int lane) const { return prep_lane_col(lane); }
    void pixel(const long long t, const long long px) {
        int oy, ox;
        prep_centred(px, ndet, oy, ox);
        if (oy < 0 || oy >= ndet || ox < 0 || ox >= ndet) ++bad;
        else ++cvis[(size_t)oy * ndet + ox];
        if (t == 0) ++mask[(size_t)px];
    }
    long long angle_errors() {
        long long e = 0;
        for (unsigned& v : cvis) { e += v != 1; v = 0; }
        return e;
    }
    long long errors() const {
        long long e = bad;
        for (unsigned char v : mask) e += v != 1;
        return e;
    }
};

static long long walk(const long long ptheta, const long long nscan, const int ndet, FramePlan& p) {
    PrepWalkHook hook(ndet);
    return walk_frame_part<PrepPart>(ptheta, nscan, (long long)ndet * ndet, p, hook);
}

// the index map against its definition written out: data[r][c] = v[(r + ndet / 2) % ndet][(c + ndet / 2) % ndet], and a raw
// pixel inside the frame or not
static long long check_map(const PrepGeom& g) {
    long long errors = 0;
    const int n = g.ndet;
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            int oy, ox;
            prep_centred((long long)r * n + c, n, oy, ox);
            errors += oy != (r + n / 2) % n || ox != (c + n / 2) % n;
            for (int by = 0; by < g.bin; ++by)
                for (int bx = 0; bx < g.bin; ++bx) {
                    const long long y = g.y0 + (long long)oy * g.bin + by, x = g.x0 + (long long)ox * g.bin + bx;
                    const bool in = y >= 0 && y < g.H && x >= 0 && x < g.W;
                    errors += prep_raw_offset(g, oy, ox, by, bx) != (in ? y * g.W + x : -1);
                }
            // with the vector loads a run of four raw elements from the first of a lane's group is inside or outside as a
            // whole and starts on a multiple of four elements
            if (prep_runs_aligned(g) && c % PrepPart::kLanePix == 0)
                for (int by = 0; by < g.bin; ++by)
                    for (int u = 0; u < g.bin; ++u) {
                        const long long x = g.x0 + (long long)ox * g.bin + 4 * u;
                        errors += ((x % 4) + 4) % 4 != 0 || (x >= 0) != (x + 3 >= 0) || (x < g.W) != (x + 3 < g.W);
                        errors += ox + PrepPart::kLanePix > n;   // the group does not wrap
                    }
        }
    return errors;
}

int main(int argc, char** argv) {
    if (argc == 5 && !std::strcmp(argv[1], "walk")) {
        const unsigned long long ptheta = std::strtoull(argv[2], nullptr, 10), nscan = std::strtoull(argv[3], nullptr, 10),
                                 ndet = std::strtoull(argv[4], nullptr, 10);
        if (ndet == 0 || ndet > kPrepMaxNdet || !prep_sizes_ok(ptheta, nscan, ndet * ndet)) return 2;
        FramePlan p;
        const long long errors = walk((long long)ptheta, (long long)nscan, (int)ndet, p);
        std::printf("%lld %lld %lld %lld\n", errors, p.fwords + p.pwords, p.nranges, p.nwt);
        return 0;
    }
    if (argc == 8 && !std::strcmp(argv[1], "map")) {
        const PrepGeom g{std::atoll(argv[4]), std::atoll(argv[5]), std::atoll(argv[6]), std::atoll(argv[7]),
                         std::atoi(argv[3]), std::atoi(argv[2])};
        if (g.ndet < 1 || g.ndet > (int)kPrepMaxNdet || (g.bin != 1 && g.bin != 2 && g.bin != 4) || g.H < 1 || g.W < 1) return 2;
        for (long long p = 0; p < (long long)g.ndet * g.ndet; ++p) {
            int oy, ox;
            prep_centred(p, g.ndet, oy, ox);
            std::printf("%d %d %lld %lld %d\n", oy, ox, prep_raw_offset(g, oy, ox, 0, 0),
                        prep_raw_offset(g, oy, ox, g.bin - 1, g.bin - 1), prep_runs_aligned(g) ? 1 : 0);
        }
        return 0;
    }
    if (argc != 1) return 2;
    // no arguments: shapes of its own -- one wave tile, partial tiles, several ranges with a short last one, odd and
    // tiny detectors, the flagship size; windows inside, overhanging every edge and wholly outside
    const long long shapes[][3] = {{1, 1, 16}, {2, 3, 24}, {1, 300, 16}, {1, 7, 15}, {1, 2, 32}, {1, 7, 64}, {1, 1, 1},
                                   {3, 129, 2}, {1, 5, 3}, {2, 1000, 33}, {1, 4096, 256}, {1, 257, 45}};
    long long errors = 0;
    for (const auto& s : shapes) {
        FramePlan p;
        const long long e = walk(s[0], s[1], (int)s[2], p);
        std::printf("walk %lld x %lld x %lld^2: %lld ranges, %lld wave tiles, %lld words, %lld errors\n", s[0], s[1], s[2],
                    p.nranges, p.nwt, p.fwords + p.pwords, e);
        errors += e;
    }
    const PrepGeom geoms[] = {{16, 16, 0, 0, 1, 16},   {40, 36, 7, 5, 1, 24},   {32, 32, 0, 0, 2, 16},  {20, 21, 3, 3, 1, 15},
                              {100, 90, -44, 16, 4, 32}, {80, 83, 8, 9, 1, 64}, {80, 84, 8, 12, 1, 64}, {512, 512, 0, 0, 2, 256},
                              {8, 8, -100, 3, 2, 8},   {5, 7, 2, 3, 1, 1},      {5, 7, 2, 3, 4, 2},     {9, 9, 8, -1, 2, 3},
                              {64, 64, -8, -4, 4, 24}};
    for (const PrepGeom& g : geoms) {
        const long long e = check_map(g);
        std::printf("map ndet %d bin %d raw %lld x %lld origin (%lld, %lld): vector loads %d, %lld errors\n", g.ndet, g.bin,
                    g.H, g.W, g.y0, g.x0, prep_runs_aligned(g) ? 1 : 0, e);
        errors += e;
    }
    std::printf("host_prepare: %lld errors\n", errors);
    return errors ? 1 : 0;
}
