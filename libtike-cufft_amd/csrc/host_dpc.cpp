// Host build of the index logic of k_dpc.hpp, walked as the kernels walk it.  Built by tests/test_dpc_cpu.py with clang++
// (no GPU involved).
//   host_dpc moments ptheta nscan ndet   the partition of k_frame_moments (frame_part_walk.hpp) and the signed frequencies
//                                        of every pixel a lane visits: "errors nwt nranges words sum_ky2 sum_kx2 sum_kykx",
//                                        the three sums over one frame's pixels as the walk met them
//   host_dpc map                         stdin "ptheta nscan nprb nz n nval", then ptheta * nscan pairs (row, column) as
//                                        the bit patterns of the float32 values, then ptheta * nscan keep flags (0 / 1):
//                                        k_scan_keep's replacement and k_scan_map's tiles, packed list and taps
//                                        (illum_walk.hpp): "errors visits skipped", errors counting the (position, tap,
//                                        probe pixel, channel) contributions visited a number of times other than 1 (target
//                                        pixel inside the object, position neither skipped nor excluded) or 0 (otherwise)
//   host_dpc edges nz n                  k_unwrap_setup<UnwGradSrc>'s edges (unwrap_walk.hpp): "errors tiles visits",
//                                        errors counting the edges whose d_e is not taken exactly once from each end, from
//                                        the slots of its two pixels in the order (p, q) and from the plane that
//                                        unwrap_grad_field (the helper UnwGradSrc::diff calls) names for the edge's
//                                        direction: gy (plane 0) when the two pixels differ in their row, gx (plane 1)
//                                        when in their column.  That the first two of the kernel's four calls are the
//                                        horizontal ones is restated here, not shared with it: that the kernel passes
//                                        them so, and gy as plane 0, is what the planted surfaces of
//                                        tests/test_hip_dpc.py check on the device
//   host_dpc                             sweeps the three over small shapes: "host_dpc: E errors, S shapes"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "frame_part_walk.hpp"
#include "illum_walk.hpp"
#include "k_dpc.hpp"
#include "unwrap_walk.hpp"

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

// ---- gradient edges ----------------------------------------------------------------------------------------------------------
static UnwWalk walk_edges(int nz, int n) {
    return walk_unwrap_tiles(nz, n, [n](int e, long long lo, long long hi) {
        const bool vertical = e >= 2;   // k_unwrap_setup's four calls: left, right (horizontal), up, down (vertical)
        const bool rows_differ = hi / n != lo / n, cols_differ = hi % n != lo % n;
        int bad = !(lo < hi);           // the edge runs from its left / upper pixel to its right / lower one
        if (rows_differ == cols_differ || vertical != rows_differ) ++bad;   // neighbours along one axis
        if (unwrap_grad_field(vertical) != (rows_differ ? 0 : 1)) ++bad;    // gy across rows, gx across columns
        return bad;
    });
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
        const IllumWalk w = walk_illum(ptheta, nscan, nprb, nz, n, nval, scan.data(), keep.data());
        std::printf("%lld %lld %lld\n", w.errors, w.visits, w.skipped);
        return w.errors ? 1 : 0;
    }
    if (argc == 4 && !std::strcmp(argv[1], "edges")) {
        const int nz = std::atoi(argv[2]), n = std::atoi(argv[3]);
        if (nz < 2 || n < 2) return 2;
        const UnwWalk w = walk_edges(nz, n);
        std::printf("%lld %lld %lld\n", w.errors, w.tiles, w.visits);
        return w.errors ? 1 : 0;
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
            errors += walk_edges(nz, n).errors;
            ++shapes;
        }
    std::printf("host_dpc: %lld errors, %lld shapes\n", errors, shapes);
    return errors ? 1 : 0;
}
