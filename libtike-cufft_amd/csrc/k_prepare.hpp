// k_prepare.hpp -- raw detector frames to the solver's data (ptycho_prepare_frames, libtike.hipfft.prepare): crop around a
// beam centre, bin, subtract the dark frame, multiply by the gain, drop bad pixels, clip, scale, move the centre to
// [0, 0] (ifftshift), and per-frame / per-pixel statistics, in one pass that reads every raw byte once.  No handle, no
// atomics, every sum in a fixed order: the same inputs give the same bits.
//
//   k_prepare       A workgroup (four independent waves, no barrier) owns a tile of PrepPart::kTile OUTPUT pixels (indices
//                   in the layout of `data`) and one range of frames of its angle; a lane owns one group of four consecutive
//                   output pixels: one 16-byte store of data per frame.  VEC (ndet % 8 == 0, W % 4 == 0,
//                   x0 % 4 == 0, raw aligned to four elements): the shift leaves the four pixels of a group consecutive in
//                   the raw row and a run of four raw elements wholly inside or outside the frame, so a group reads
//                   bin vector loads of four elements per raw row; otherwise one load per raw element.  Nothing is
//                   predicated: an element outside the frame, or of a frame whose index is out of range, reads element 0
//                   of a frame that exists, and the value is dropped by a select.  bin 1 and 2: the offsets, the dark and
//                   gain values and the validity of the lane's raw elements stay in registers over the range, and the
//                   next frame's loads are issued before this frame's arithmetic; bin 4: they are formed again per frame, one
//                   output pixel (sixteen raw elements) at a time.
//                   Per pixel: sum, sum of squares (float64), maximum and saturation count over the frames of the range,
//                   in registers, stored once at the end.  Per frame: the same four over the lane's four pixels, then
//                   over the wave: the four vectors are reduced TOGETHER (two exchanges halve the number of vectors a
//                   lane carries, four more finish the one that is left) and lanes 0, 16, 32, 48 store them.
//   k_prepare_fold  combines the wave tiles of every frame and the ranges of every pixel in index order: sums and counts
//                   are added, maxima taken.
//
// The partition and the words of `work` are PrepPart, an instance of frame_part.hpp's plain C++, over OUTPUT pixels; the
// store lanes (prep_lane_col) and the crop / shift index map (prep_centred, prep_raw_offset) are plain C++ too:
// host_prepare.cpp walks them on the CPU.
#pragma once

#include "frame_part.hpp"

namespace pty {

// one group of four output pixels per lane: 256 pixels per wave, 1024 per workgroup; per frame and per pixel the sum,
// the sum of squares, the maximum and the saturation count
using PrepPart = FramePart<4, 1, 4, 4>;
constexpr int kPrepMaxCol = 2;                                 // the column / map that is folded with max, not +
constexpr unsigned long long kPrepMaxAngles = 65535;           // gridDim.z
constexpr unsigned long long kPrepMaxFrames = 0x7fffffffull;   // nraw, nscan
constexpr unsigned long long kPrepMaxFrame = 0x7fffffffull;    // H * W: an offset inside a raw frame fits an int
constexpr unsigned long long kPrepMaxNdet = 32768;             // npix <= 2^30
constexpr long long kPrepMaxOrigin = 1ll << 30;                // |y0|, |x0|
constexpr unsigned long long kPrepMaxElems = 1ull << 59;       // elements of raw and of data: byte offsets stay in 64 bits

enum PrepDtype { kPrepU16 = 0, kPrepU32 = 1, kPrepI32 = 2, kPrepF32 = 3, kPrepDtypes = 4 };

struct PrepGeom {
    long long H, W;      // raw frame
    long long y0, x0;    // raw row and column of the first pixel of the crop window
    int bin, ndet;
};

PTY_HD bool prep_sizes_ok(const unsigned long long ptheta, const unsigned long long nscan, const unsigned long long npix) {
    if (ptheta == 0 || nscan == 0 || npix == 0) return false;
    if (ptheta > kPrepMaxAngles || nscan > kPrepMaxFrames || npix > kPrepMaxNdet * kPrepMaxNdet) return false;
    if (ptheta * nscan > kPrepMaxElems / npix) return false;   // ptheta * nscan < 2^47: no overflow on the left
    return true;
}

// the raw side: ptheta * nraw frames of H x W
PTY_HD bool prep_raw_ok(const unsigned long long ptheta, const unsigned long long nraw, const unsigned long long H,
                        const unsigned long long W) {
    if (nraw == 0 || H == 0 || W == 0 || nraw > kPrepMaxFrames) return false;
    if (H > kPrepMaxFrame || W > kPrepMaxFrame || H > kPrepMaxFrame / W) return false;
    if (ptheta * nraw > kPrepMaxElems / (H * W)) return false;
    return true;
}

// lane (lane & 15 == 0) -> the column it stores after prep_wave_reduce: 0 sum, 1 sum of squares, 3 count, 2 maximum
PTY_HD int prep_lane_col(const int lane) { return (lane >> 4) == 2 ? 3 : (lane >> 4) == 3 ? 2 : (lane >> 4); }

// output pixel p = r * ndet + c of the layout of `data` -> the centred pixel (oy, ox) it holds: ifftshift
PTY_HD void prep_centred(const long long p, const int ndet, int& oy, int& ox) {
    const int r = (int)(p / ndet), c = (int)(p % ndet), half = ndet / 2;
    oy = (r + half) % ndet;
    ox = (c + half) % ndet;
}
// offset inside its frame of raw pixel (by, bx) of the bin of centred pixel (oy, ox); -1: outside the frame
PTY_HD long long prep_raw_offset(const PrepGeom& g, const int oy, const int ox, const int by, const int bx) {
    const long long y = g.y0 + (long long)oy * g.bin + by, x = g.x0 + (long long)ox * g.bin + bx;
    return (y < 0 || y >= g.H || x < 0 || x >= g.W) ? -1 : y * g.W + x;
}
// the vector loads apply: a lane's run of 4 * bin raw elements starts on a multiple of four elements in every frame
PTY_HD bool prep_runs_aligned(const PrepGeom& g) {
    return g.ndet % 8 == 0 && g.W % 4 == 0 && ((g.x0 % 4) + 4) % 4 == 0;
}

#if defined(__HIPCC__)

struct PrepArgs {
    float* data;
    unsigned char* mask;
    double* fpart;         // [ptheta * nscan][nwt][4]: the frame part of work, or frames itself (nwt == 1)
    double* ppart;         // [ptheta][nranges][4][npix]: the pixel part of work, or pixels itself (nranges == 1)
    const void* raw;
    const long long* index;
    const float* dark;
    const float* gain;
    const unsigned char* bad;
    PrepGeom g;
    long long npix, nwt, nraw;
    int nscan, flen;
    float sat, scale;      // sat NaN: no pixel counts as saturated
    int clip, vst, pix;    // vst: 16-byte stores of data; pix: the per-pixel sums are wanted
};

// offsets, dark and gain of the BIN * BIN raw elements of one output pixel; returns whether the pixel is measured.  An
// element outside the frame gets offset 0, dark 0 and gain 1 (its value is dropped with the pixel)
template <int BIN>
__device__ __forceinline__ bool prep_cal(const PrepArgs& a, const int oy, const int ox, const bool live,
                                         int (&off)[BIN * BIN], float (&dk)[BIN * BIN], float (&gn)[BIN * BIN]) {
    bool meas = live;
#pragma unroll
    for (int by = 0; by < BIN; ++by)
#pragma unroll
        for (int bx = 0; bx < BIN; ++bx) {
            const int e = by * BIN + bx;
            const long long o = live ? prep_raw_offset(a.g, oy, ox, by, bx) : -1;
            const bool in = o >= 0;
            off[e] = in ? (int)o : 0;
            dk[e] = in && a.dark ? a.dark[o] : 0.0f;
            gn[e] = in && a.gain ? a.gain[o] : 1.0f;
            meas = meas && in && !(a.bad && a.bad[off[e]] != 0);
        }
    return meas;
}

// the raw elements of the four pixels of one group.  VEC: per raw row, BIN loads of four consecutive elements from the
// first element of the run, which is element 0 of pixel 0 (a run is inside or outside as a whole)
template <typename T, int BIN, bool VEC>
__device__ __forceinline__ void prep_load_group(const T* __restrict__ frame, const int (*off)[BIN * BIN],
                                                T (*rw)[BIN * BIN]) {
    typedef T vec4 __attribute__((ext_vector_type(4)));
    if constexpr (VEC) {
#pragma unroll
        for (int by = 0; by < BIN; ++by)
#pragma unroll
            for (int u = 0; u < BIN; ++u) {
                const int k0 = (4 * u) / BIN, b0 = (4 * u) % BIN;
                const vec4 v = __builtin_nontemporal_load((const vec4*)(frame + off[k0][by * BIN + b0]));
#pragma unroll
                for (int c = 0; c < 4; ++c) rw[(4 * u + c) / BIN][by * BIN + (4 * u + c) % BIN] = v[c];
            }
    } else {
#pragma unroll
        for (int k = 0; k < PrepPart::kLanePix; ++k)
#pragma unroll
            for (int e = 0; e < BIN * BIN; ++e) rw[k][e] = __builtin_nontemporal_load(frame + off[k][e]);
    }
}

// the raw elements of one pixel of bin 4: per raw row, one load of four elements (VEC) or four loads
template <typename T, int BIN, bool VEC>
__device__ __forceinline__ void prep_load_pixel(const T* __restrict__ frame, const int (&off)[BIN * BIN], T (&rw)[BIN * BIN]) {
    typedef T vec4 __attribute__((ext_vector_type(4)));
    static_assert(BIN % 4 == 0, "a pixel's raw row is a whole number of vector loads");
#pragma unroll
    for (int e = 0; e < BIN * BIN; e += 4) {
        if constexpr (VEC) {
            const vec4 v = __builtin_nontemporal_load((const vec4*)(frame + off[e]));
#pragma unroll
            for (int c = 0; c < 4; ++c) rw[e + c] = v[c];
        } else {
#pragma unroll
            for (int c = 0; c < 4; ++c) rw[e + c] = __builtin_nontemporal_load(frame + off[e + c]);
        }
    }
}

// one output pixel: v = scale * clip(sum over the bin of (float(raw) - dark) * gain), every operation rounded, the sum in
// the order by outer, bx inner from the first term; nsat: raw elements at or above the saturation level
template <typename T, int BIN>
__device__ __forceinline__ float prep_value(const T (&rw)[BIN * BIN], const float (&dk)[BIN * BIN],
                                            const float (&gn)[BIN * BIN], const float sat, const int clip,
                                            const float scale, int& nsat) {
#pragma clang fp contract(off)
    float v = 0.0f;
    nsat = 0;
#pragma unroll
    for (int e = 0; e < BIN * BIN; ++e) {
        const float x = (float)rw[e];
        const float t = (x - dk[e]) * gn[e];
        v = e == 0 ? t : v + t;
        nsat += x >= sat ? 1 : 0;
    }
    if (clip) v = v < 0.0f ? 0.0f : v;   // a NaN stays
    return v * scale;
}

// f = {sum, sum of squares, count, maximum} of the lane -> the same over the wave, in lanes 0, 16, 32, 48
// (prep_lane_col): bits 5 and 4 of the lane pick the half of the vectors that is kept
__device__ __forceinline__ double prep_wave_reduce(const double (&f)[PrepPart::kCols], const int lane) {
    const bool hi = (lane & 32) != 0, hi2 = (lane & 16) != 0, is_max = hi && hi2;
    const double k0 = hi ? f[2] : f[0], s0 = hi ? f[0] : f[2], k1 = hi ? f[3] : f[1], s1 = hi ? f[1] : f[3];
    const double a0 = k0 + __shfl_xor(s0, 32);
    const double a1 = sum_or_max(k1, __shfl_xor(s1, 32), hi);
    double v = sum_or_max(hi2 ? a1 : a0, __shfl_xor(hi2 ? a0 : a1, 16), is_max);
    v = sum_or_max(v, __shfl_xor(v, 8), is_max);
    v = sum_or_max(v, __shfl_xor(v, 4), is_max);
    v = sum_or_max(v, __shfl_xor(v, 2), is_max);
    v = sum_or_max(v, __shfl_xor(v, 1), is_max);
    return v;
}

// grid (ntiles, nranges, ptheta), 256 threads
template <typename T, int BIN, bool VEC>
__global__ __launch_bounds__(256) void k_prepare(const PrepArgs a) {
    constexpr int E = BIN * BIN, S = PrepPart::kSlots, G = PrepPart::kGroups, L = PrepPart::kLanePix;
    constexpr bool KEEP = BIN <= 2;          // calibration in registers over the range, and the next frame's loads early
    constexpr int KS = KEEP ? S : 1;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long wt = (long long)blockIdx.x * PrepPart::kWaves + wave;
    if (wt >= a.nwt) return;   // waves are independent: no barrier below
    const long long r = blockIdx.y, t = blockIdx.z, npix = a.npix;
    long long p0[G];
    int oy[S], ox[S], off[KS][E];
    float dk[KS][E], gn[KS][E];
    bool live[S], meas[S];
#pragma unroll
    for (int h = 0; h < G; ++h) p0[h] = PrepPart::pixel(wt, lane, h);
#pragma unroll
    for (int q = 0; q < S; ++q) {
        const long long p = p0[q / L] + q % L;
        live[q] = p < npix;
        prep_centred(live[q] ? p : 0, a.g.ndet, oy[q], ox[q]);
        if constexpr (KEEP) {
            meas[q] = prep_cal<BIN>(a, oy[q], ox[q], live[q], off[q], dk[q], gn[q]);
        } else {
            int o[E];
            float d[E], g[E];
            meas[q] = prep_cal<BIN>(a, oy[q], ox[q], live[q], o, d, g);
        }
        if (r == 0 && t == 0 && live[q]) a.mask[p] = meas[q] ? 1 : 0;
    }
    const int j0 = (int)r * a.flen, j1 = j0 + a.flen < a.nscan ? j0 + a.flen : a.nscan;
    const size_t frame0 = (size_t)t * (size_t)a.nscan, fsz = (size_t)(a.g.H * a.g.W);
    const T* const rawt = (const T*)a.raw + (size_t)t * (size_t)a.nraw * fsz;
    double ps[S], ps2[S];
    float pm[S];
    int pc[S];
#pragma unroll
    for (int q = 0; q < S; ++q) {
        ps[q] = 0.0;
        ps2[q] = 0.0;
        pm[q] = -__builtin_inff();
        pc[q] = 0;
    }

    // raw frame of output frame j; valid: its index is in range (otherwise frame 0, dropped by the caller)
    auto source = [&](const int j, bool& valid) __attribute__((always_inline)) {
        const long long idx = a.index ? a.index[frame0 + (size_t)j] : (long long)j;
        valid = idx >= 0 && idx < a.nraw;
        return rawt + (size_t)(valid ? idx : 0) * fsz;
    };
    // one frame of one wave: data, the lane's pixels into the per-pixel and the per-frame statistics, the frame's over the
    // wave, the store of the partials
    auto frame = [&](const T* __restrict__ src, const T (*pre)[E], const bool valid, const int j) __attribute__((always_inline)) {
        double f[PrepPart::kCols] = {0.0, 0.0, 0.0, -(double)__builtin_inff()};
        float fm = -__builtin_inff();
        int fc = 0;
        float* const out = a.data + (frame0 + (size_t)j) * (size_t)npix;
#pragma unroll
        for (int h = 0; h < G; ++h) {
            float v4[L];
#pragma unroll
            for (int k = 0; k < L; ++k) {
#pragma clang fp contract(off)
                const int q = h * L + k;
                int ns;
                float v;
                if constexpr (KEEP) {
                    v = prep_value<T, BIN>(pre[q], dk[q], gn[q], a.sat, a.clip, a.scale, ns);
                } else {   // pixel by pixel, so that one pixel's sixteen elements are live at a time
                    T now[E];
                    int o[E];
                    float d[E], g[E];
                    int oyq = oy[q], oxq = ox[q];
                    asm volatile("" : "+v"(oyq), "+v"(oxq));   // formed again per frame: not hoisted out of the frame loop
                    prep_cal<BIN>(a, oyq, oxq, live[q], o, d, g);
                    prep_load_pixel<T, BIN, VEC>(src, o, now);
                    v = prep_value<T, BIN>(now, d, g, a.sat, a.clip, a.scale, ns);
                    __builtin_amdgcn_sched_barrier(0);
                }
                const bool ok = meas[q] && valid;
                v = ok ? v : 0.0f;
                ns = ok ? ns : 0;
                const float v2 = v * v;
                v4[k] = v;
                f[0] += (double)v;
                f[1] += (double)v2;
                fm = ok ? fmaxf(fm, v) : fm;
                fc += ns;
                ps[q] += (double)v;
                ps2[q] += (double)v2;
                pm[q] = ok ? fmaxf(pm[q], v) : pm[q];
                pc[q] += ns > 0 ? 1 : 0;
            }
            if (VEC || a.vst) {   // npix % 4 == 0: a group is inside or outside the detector as a whole
                if (live[h * L]) __builtin_nontemporal_store(vec4f{v4[0], v4[1], v4[2], v4[3]}, (vec4f*)(out + p0[h]));
            } else {
#pragma unroll
                for (int k = 0; k < L; ++k)
                    if (live[h * L + k]) out[p0[h] + k] = v4[k];
            }
        }
        f[2] = (double)fc;
        f[3] = (double)fm;
        const double v = prep_wave_reduce(f, lane);
        if ((lane & 15) == 0)
            a.fpart[PrepPart::frame_word((long long)(frame0 + (size_t)j), wt, a.nwt) + prep_lane_col(lane)] =
                valid ? v : 0.0;
    };

    if constexpr (KEEP) {
        // two buffers, frames alternate between them: a frame's loads are issued before the arithmetic of the frame before
        T ra[S][E], rb[S][E];
        bool va, vb = false;
        const T* sa = source(j0, va);
        const T* sb = sa;
#pragma unroll
        for (int h = 0; h < G; ++h) prep_load_group<T, BIN, VEC>(sa, off + h * L, ra + h * L);
        for (int j = j0; j < j1; j += 2) {
            if (j + 1 < j1) {
                sb = source(j + 1, vb);
#pragma unroll
                for (int h = 0; h < G; ++h) prep_load_group<T, BIN, VEC>(sb, off + h * L, rb + h * L);
            }
            frame(sa, ra, va, j);
            if (j + 1 >= j1) break;
            if (j + 2 < j1) {
                sa = source(j + 2, va);
#pragma unroll
                for (int h = 0; h < G; ++h) prep_load_group<T, BIN, VEC>(sa, off + h * L, ra + h * L);
            }
            frame(sb, rb, vb, j + 1);
        }
    } else {
        for (int j = j0; j < j1; ++j) {
            bool valid;
            const T* src = source(j, valid);
            frame(src, nullptr, valid, j);
        }
    }
    if (a.pix) {
        double* const dst = a.ppart + PrepPart::pixel_word(t, r, 0, gridDim.y, npix);
#pragma unroll
        for (int q = 0; q < S; ++q) {
            if (!live[q]) continue;
            const long long p = p0[q / L] + q % L;
            dst[p] = ps[q];
            dst[npix + p] = ps2[q];
            dst[2 * npix + p] = meas[q] ? (double)pm[q] : 0.0;   // an unmeasured pixel: every map is 0
            dst[3 * npix + p] = (double)pc[q];
        }
    }
}

// FramePart::fold, the maxima taken and the rest added
__global__ __launch_bounds__(256) void k_prepare_fold(double* __restrict__ frames, double* __restrict__ pixels,
                                                      const double* __restrict__ fpart, const double* __restrict__ ppart,
                                                      const long long nfout, const long long nwt, const long long npout,
                                                      const long long npix, const long long nranges,
                                                      const unsigned fblocks) {
    PrepPart::fold<kPrepMaxCol>(frames, pixels, fpart, ppart, nfout, nwt, npout, PrepPart::kMaps * npix, nranges, fblocks);
}

#endif  // __HIPCC__

}  // namespace pty
