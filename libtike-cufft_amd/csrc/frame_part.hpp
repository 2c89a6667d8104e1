// frame_part.hpp -- what the analysis kernels share: PTY_HD, the (frame, pixel) partition of a deterministic two-launch
// reduction (k_fit.hpp, k_prepare.hpp) and the block sum of the one-workgroup reductions (k_gauge.hpp, k_unwrap.hpp).
//
// The partition: a workgroup of four independent waves (no barrier) owns a tile of pixels and one range of frames of its
// angle; a lane owns GROUPS groups of LANE_PIX consecutive pixels (one 16-byte access per group).  The pass leaves COLS
// figures per (frame, wave tile) and MAPS figures per (range, pixel) in `work`, and a fold kernel combines the wave tiles
// of every frame and the ranges of every pixel in index order; with one wave tile (one range) the pass writes `frames`
// (`pixels`) itself and that half of the fold is not launched.  A frame's partials depend on that frame's values and the
// pixel -> (wave tile, lane, slot) map alone, never on the range or on the other frames.
//
// Everything outside the __HIPCC__ guards is plain C++: frame_part_walk.hpp walks it on the CPU.
#pragma once

#if defined(__HIPCC__)
#define PTY_HD __host__ __device__
#else
#define PTY_HD inline
#endif

namespace pty {

struct FramePlan {
    long long nwt;       // wave tiles per frame
    long long ntiles;    // workgroup tiles per frame
    long long nranges;   // frame ranges per angle
    long long flen;      // frames per range (the last one may be shorter)
    long long fwords;    // float64 words of per-(frame, wave tile) partials, 0: the kernel writes `frames` itself
    long long pwords;    // float64 words of per-(range, map, pixel) partials, 0: the kernel writes `pixels` itself
};

#if defined(__HIPCC__)
typedef float vec4f __attribute__((ext_vector_type(4)));

__device__ __forceinline__ double sum_or_max(const double keep, const double recv, const bool is_max) {
    return is_max ? fmax(keep, recv) : keep + recv;
}
#endif

template <int LANE_PIX, int GROUPS, int COLS, int MAPS>
struct FramePart {
    static constexpr int kLanePix = LANE_PIX;                   // consecutive pixels of one 16-byte access
    static constexpr int kGroups = GROUPS;                      // such groups per lane
    static constexpr int kSlots = kLanePix * kGroups;           // pixels per lane
    static constexpr int kGroupSpan = 64 * kLanePix;            // pixels one access instruction of a wave covers
    static constexpr int kWaveTile = kGroupSpan * kGroups;      // pixels per wave
    static constexpr int kWaves = 4;
    static constexpr int kTile = kWaveTile * kWaves;            // pixels per workgroup
    static constexpr int kCols = COLS, kMaps = MAPS;            // figures per frame, maps per angle
    static constexpr long long kMinRange = 128;                 // frames: at most ceil(nscan / 128) ranges
    static constexpr long long kTargetGroups = 2048;            // workgroups wanted: 256 compute units, eight each

    // sizes must have passed the user's own limits (fit_sizes_ok, prep_sizes_ok)
    PTY_HD static FramePlan plan(const long long ptheta, const long long nscan, const long long npix) {
        FramePlan p;
        p.nwt = (npix + kWaveTile - 1) / kWaveTile;
        p.ntiles = (npix + kTile - 1) / kTile;
        const long long per_range = ptheta * p.ntiles;
        long long nr = (kTargetGroups + per_range - 1) / per_range;
        const long long most = (nscan + kMinRange - 1) / kMinRange;
        if (nr > most) nr = most;
        p.flen = (nscan + nr - 1) / nr;
        p.nranges = (nscan + p.flen - 1) / p.flen;
        p.fwords = p.nwt > 1 ? ptheta * nscan * p.nwt * kCols : 0;
        p.pwords = p.nranges > 1 ? ptheta * p.nranges * kMaps * npix : 0;
        return p;
    }
    // first pixel of group h of lane `lane` of wave tile wt; the group is the kLanePix pixels from there
    PTY_HD static long long pixel(const long long wt, const int lane, const int h) {
        return wt * kWaveTile + (long long)h * kGroupSpan + (long long)lane * kLanePix;
    }
    // word of the partials of (frame, wave tile) in the frame part of `work` (frame counts over all angles)
    PTY_HD static long long frame_word(const long long frame, const long long wt, const long long nwt) {
        return (frame * nwt + wt) * kCols;
    }
    // word of pixel 0 of (angle, range, map) in the pixel part of `work`
    PTY_HD static long long pixel_word(const long long t, const long long r, const int map, const long long nranges,
                                       const long long npix) {
        return ((t * nranges + r) * kMaps + map) * npix;
    }

#if defined(__HIPCC__)
    // body of a fold kernel, grid fblocks + pblocks, 256 threads: the first fblocks workgroups combine the wave tiles of
    // ptheta * nscan * kCols frame figures, the others the ranges of ptheta * kMaps * npix pixel figures (slab = kMaps
    // npix: the maps of one angle and range), both in index order.  Column / map MAXCOL is folded with max, every other
    // one with +; MAXCOL < 0: all of them with +
    template <int MAXCOL>
    __device__ __forceinline__ static void fold(double* __restrict__ frames, double* __restrict__ pixels,
                                                const double* __restrict__ fpart, const double* __restrict__ ppart,
                                                const long long nfout, const long long nwt, const long long npout,
                                                const long long slab, const long long nranges, const unsigned fblocks) {
        // a plain sum starts from 0.0; one with a max column from the first partial: fmax(-inf, NaN) = -inf would lose a NaN
        constexpr long long first = MAXCOL < 0 ? 0 : 1;
        if (blockIdx.x < fblocks) {
            const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
            if (i >= nfout) return;
            const long long frame = i / kCols, e = i % kCols;
            double s = 0.0;
            if constexpr (MAXCOL >= 0) s = fpart[frame_word(frame, 0, nwt) + e];
            for (long long w = first; w < nwt; ++w)
                s = sum_or_max(s, fpart[frame_word(frame, w, nwt) + e], MAXCOL >= 0 && e == MAXCOL);
            frames[i] = s;
        } else {
            const long long i = (long long)(blockIdx.x - fblocks) * 256 + threadIdx.x;
            if (i >= npout) return;
            const long long t = i / slab, rem = i % slab;
            double s = 0.0;
            if constexpr (MAXCOL >= 0) s = ppart[t * nranges * slab + rem];
            for (long long r = first; r < nranges; ++r)
                s = sum_or_max(s, ppart[(t * nranges + r) * slab + rem], MAXCOL >= 0 && rem / (slab / kMaps) == MAXCOL);
            pixels[i] = s;
        }
    }
#endif
};

#if defined(__HIPCC__)

// v[0 .. NV) of the 256 threads -> dst[0 .. NV): a shuffle tree per wave, then the four waves in order.  part: 4 NV doubles
template <int NV>
__device__ __forceinline__ void block_sum(double (&v)[NV], double* __restrict__ dst, double* part) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int e = 0; e < NV; ++e) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[e] += __shfl_xor(v[e], o);
    }
    __syncthreads();
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < NV; ++e) part[wave * NV + e] = v[e];
    }
    __syncthreads();
    if (tid < NV) dst[tid] = ((part[tid] + part[NV + tid]) + part[2 * NV + tid]) + part[3 * NV + tid];
}

#endif  // __HIPCC__

}  // namespace pty
