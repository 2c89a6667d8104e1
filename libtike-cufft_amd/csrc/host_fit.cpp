// Host build of the partition of k_fit_frames / k_fit_fold (k_fit.hpp): workgroup tiles, waves, lanes and their pixel
// groups, the frame ranges, and the words of `work` that the pass writes and the fold reads, walked as the kernels walk
// them.  Built by tests/test_fit_cpu.py with clang++ (no GPU involved).  argv: "ptheta nscan npix"; stdout:
// "errors words cap nranges nwt", where errors counts the (frame, pixel) pairs visited a number of times other than 1,
// plus the words of `work` below `words` written or folded a number of times other than 1, plus the words of frames /
// pixels left without exactly one writer; words is what ptycho_fit_work_words returns and cap the most it may be,
// max(1 MiB, bytes of data / 4) / 8.
//
// A workgroup is (tile, range, angle) and visits the pairs {pixels of the tile} x {frames of the range}, so the number
// of visits of the pair (j, p) is the product of the visits of j over the ranges and of p over the tiles: the walk counts
// the two factors and multiplies, which keeps 4096 x 256^2 within a second.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "k_fit.hpp"

using namespace pty;

int main(int argc, char** argv) {
    if (argc != 4) return 2;
    const unsigned long long ptheta = std::strtoull(argv[1], nullptr, 10), nscan = std::strtoull(argv[2], nullptr, 10),
                             npix = std::strtoull(argv[3], nullptr, 10);
    if (!fit_sizes_ok(ptheta, nscan, npix)) return 2;
    const FitPlan p = fit_plan((long long)ptheta, (long long)nscan, (long long)npix);
    const long long words = p.fwords + p.pwords;
    long long errors = 0;
    std::vector<unsigned char> wrote((size_t)words, 0), folded((size_t)words, 0);
    for (long long t = 0; t < (long long)ptheta; ++t) {
        std::vector<unsigned> fvis((size_t)nscan, 0), pvis((size_t)npix, 0);
        std::vector<unsigned char> fout((size_t)nscan * kFitCols, 0), pout((size_t)kFitMaps * npix, 0);
        for (long long r = 0; r < p.nranges; ++r) {
            const long long j0 = r * p.flen, j1 = j0 + p.flen < (long long)nscan ? j0 + p.flen : (long long)nscan;
            if (j0 >= j1) ++errors;   // an empty range would be a workgroup with nothing to do
            for (long long j = j0; j < j1; ++j) ++fvis[(size_t)j];
        }
        for (long long tile = 0; tile < p.ntiles; ++tile)
            for (int wave = 0; wave < kFitWaves; ++wave) {
                const long long wt = tile * kFitWaves + wave;
                if (wt >= p.nwt) continue;
                bool any = false;
                for (int lane = 0; lane < 64; ++lane)
                    for (int q = 0; q < kFitSlots; ++q) {
                        const long long px = fit_pixel(wt, lane, q / kFitLanePix) + q % kFitLanePix;
                        if (px >= (long long)npix) continue;
                        ++pvis[(size_t)px];
                        any = true;
                        // the pass stores this pixel's four sums once per range
                        for (long long r = 0; r < p.nranges; ++r)
                            for (int m = 0; m < kFitMaps; ++m) {
                                if (p.pwords) ++wrote[(size_t)(p.fwords + fit_pixel_word(t, r, m, p.nranges, npix) + px)];
                                else ++pout[(size_t)m * npix + px];
                            }
                    }
                if (!any) ++errors;   // a live wave tile holds at least one pixel
                // lane 8 e of the wave stores sum e of every frame of every range
                for (long long r = 0; r < p.nranges; ++r)
                    for (long long j = r * p.flen; j < (r + 1) * p.flen && j < (long long)nscan; ++j)
                        for (int e = 0; e < kFitCols; ++e) {
                            if (p.fwords) ++wrote[(size_t)(fit_frame_word(t * nscan + j, wt, p.nwt) + e)];
                            else ++fout[(size_t)j * kFitCols + e];
                        }
            }
        // the fold: one thread per output word
        if (p.fwords)
            for (long long i = 0; i < (long long)nscan * kFitCols; ++i) {
                const long long frame = t * nscan + i / kFitCols, e = i % kFitCols;
                for (long long w = 0; w < p.nwt; ++w) ++folded[(size_t)(fit_frame_word(frame, w, p.nwt) + e)];
                ++fout[(size_t)i];
            }
        if (p.pwords) {
            const long long slab = kFitMaps * (long long)npix;
            for (long long rem = 0; rem < slab; ++rem) {
                for (long long r = 0; r < p.nranges; ++r) ++folded[(size_t)(p.fwords + (t * p.nranges + r) * slab + rem)];
                ++pout[(size_t)rem];
            }
        }
        long long f1 = 0, p1 = 0;
        for (unsigned v : fvis) f1 += v == 1;
        for (unsigned v : pvis) p1 += v == 1;
        errors += (long long)nscan * (long long)npix - f1 * p1;
        for (unsigned char v : fout) errors += v != 1;
        for (unsigned char v : pout) errors += v != 1;
    }
    for (long long i = 0; i < words; ++i) errors += (wrote[(size_t)i] != 1) + (folded[(size_t)i] != 1);
    const unsigned long long quarter = ptheta * nscan * npix, mib = 1ull << 20;
    const unsigned long long cap = (quarter > mib ? quarter : mib) / 8;
    std::printf("%lld %lld %llu %lld %lld\n", errors, words, cap, p.nranges, p.nwt);
    return 0;
}
