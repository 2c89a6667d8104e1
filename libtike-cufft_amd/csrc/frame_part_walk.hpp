// frame_part_walk.hpp -- host walk of a FramePart (frame_part.hpp): workgroup tiles, waves, lanes and their pixel groups,
// the frame ranges, the lanes that store a frame's figures, and the words of `work` that the pass writes and the fold
// reads, walked as the kernels walk them.  No GPU involved: host_fit.cpp and host_prepare.cpp call it.
//
// walk_frame_part returns the number of errors: the (frame, pixel) pairs visited a number of times other than 1, the
// words of `work` written or folded a number of times other than 1, the words of frames / pixels left without exactly one
// writer, and what the hook counts.
//
// A workgroup is (tile, range, angle) and visits the pairs {pixels of the tile} x {frames of the range}, so the number
// of visits of the pair (j, p) is the product of the visits of j over the ranges and of p over the tiles: the walk counts
// the two factors and multiplies, which keeps 4096 x 256^2 within a second.
#pragma once

#include <vector>

#include "frame_part.hpp"

namespace pty {

// what a user of the partition adds to the walk; the defaults: lane (64 / kCols) e of a wave stores figure e of a frame
// (k_fit_frames), nothing else to count
template <class Part>
struct FrameWalkHook {
    static constexpr int kStoreStride = 64 / Part::kCols;   // every kStoreStride-th lane stores one figure
    int col(const int lane) const { return lane / kStoreStride; }
    void pixel(long long /*t*/, long long /*px*/) {}         // a pixel inside the detector, once per visit by a lane
    long long angle_errors() { return 0; }                   // after each angle
    long long errors() { return 0; }                         // at the end
};

template <class Part, class Hook>
long long walk_frame_part(const long long ptheta, const long long nscan, const long long npix, FramePlan& p, Hook& hook) {
    p = Part::plan(ptheta, nscan, npix);
    const long long words = p.fwords + p.pwords;
    long long errors = 0;
    std::vector<unsigned char> wrote((size_t)words, 0), folded((size_t)words, 0);
    for (long long t = 0; t < ptheta; ++t) {
        std::vector<unsigned> fvis((size_t)nscan, 0), pvis((size_t)npix, 0);
        std::vector<unsigned char> fout((size_t)nscan * Part::kCols, 0), pout((size_t)Part::kMaps * npix, 0);
        for (long long r = 0; r < p.nranges; ++r) {
            const long long j0 = r * p.flen, j1 = j0 + p.flen < nscan ? j0 + p.flen : nscan;
            if (j0 >= j1) ++errors;   // an empty range would be a workgroup with nothing to do
            for (long long j = j0; j < j1; ++j) ++fvis[(size_t)j];
        }
        for (long long tile = 0; tile < p.ntiles; ++tile)
            for (int wave = 0; wave < Part::kWaves; ++wave) {
                const long long wt = tile * Part::kWaves + wave;
                if (wt >= p.nwt) continue;
                bool any = false;
                for (int lane = 0; lane < 64; ++lane)
                    for (int q = 0; q < Part::kSlots; ++q) {
                        const long long px = Part::pixel(wt, lane, q / Part::kLanePix) + q % Part::kLanePix;
                        if (px >= npix) continue;
                        ++pvis[(size_t)px];
                        any = true;
                        hook.pixel(t, px);
                        // the pass stores this pixel's figures once per range
                        for (long long r = 0; r < p.nranges; ++r)
                            for (int m = 0; m < Part::kMaps; ++m) {
                                if (p.pwords) ++wrote[(size_t)(p.fwords + Part::pixel_word(t, r, m, p.nranges, npix) + px)];
                                else ++pout[(size_t)m * npix + px];
                            }
                    }
                if (!any) ++errors;   // a live wave tile holds at least one pixel
                // the store lanes of the wave store the figures of every frame of every range
                for (long long r = 0; r < p.nranges; ++r)
                    for (long long j = r * p.flen; j < (r + 1) * p.flen && j < nscan; ++j)
                        for (int lane = 0; lane < 64; lane += Hook::kStoreStride) {
                            const int e = hook.col(lane);
                            if (e < 0 || e >= Part::kCols) { ++errors; continue; }
                            if (p.fwords) ++wrote[(size_t)(Part::frame_word(t * nscan + j, wt, p.nwt) + e)];
                            else ++fout[(size_t)j * Part::kCols + e];
                        }
            }
        // the fold: one thread per output word
        if (p.fwords)
            for (long long i = 0; i < nscan * Part::kCols; ++i) {
                const long long frame = t * nscan + i / Part::kCols, e = i % Part::kCols;
                for (long long w = 0; w < p.nwt; ++w) ++folded[(size_t)(Part::frame_word(frame, w, p.nwt) + e)];
                ++fout[(size_t)i];
            }
        if (p.pwords) {
            const long long slab = Part::kMaps * npix;
            for (long long rem = 0; rem < slab; ++rem) {
                for (long long r = 0; r < p.nranges; ++r) ++folded[(size_t)(p.fwords + (t * p.nranges + r) * slab + rem)];
                ++pout[(size_t)rem];
            }
        }
        long long f1 = 0, p1 = 0;
        for (unsigned v : fvis) f1 += v == 1;
        for (unsigned v : pvis) p1 += v == 1;
        errors += nscan * npix - f1 * p1;
        for (unsigned char v : fout) errors += v != 1;
        for (unsigned char v : pout) errors += v != 1;
        errors += hook.angle_errors();
    }
    for (long long i = 0; i < words; ++i) errors += (wrote[(size_t)i] != 1) + (folded[(size_t)i] != 1);
    return errors + hook.errors();
}

}  // namespace pty
