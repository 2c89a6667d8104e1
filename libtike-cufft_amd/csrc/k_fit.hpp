// k_fit.hpp -- per-frame and per-pixel fit residuals of a reconstruction (ptycho_fit_accumulate / ptycho_fit_frames,
// libtike.hipfft.fit).  No handle, no float atomics, every sum in a fixed order: the same inputs give the same bits.
//
//   k_fit_accumulate  inten = |g|^2 or inten += |g|^2, four elements per thread (16-byte loads where the pointers allow).
//   k_fit_frames      one pass over farplane / intensity and data.  A workgroup (four independent waves, no barrier) owns
//                     a tile of FitPart::kTile pixels and one range of frames of its angle; a lane owns two groups of four
//                     consecutive pixels (one 16-byte load of data / intensity, two of the farplane, per group and
//                     frame), the next frame's loads issued before this frame's arithmetic.  An unmeasured pixel gets
//                     I = d = 0 by a select.  Terms in float32, every accumulation in float64:
//                       per pixel   four sums over the frames of the range, in registers, stored once at the end into
//                                   the range's slab of `work` (or into `pixels` when there is one range);
//                       per frame   eight sums over the lane's eight pixels, then over the wave: the eight vectors are
//                                   reduced TOGETHER -- each of the first three exchanges halves the number of vectors
//                                   a lane carries (8 -> 4 -> 2 -> 1), three more finish the one that is left: 10
//                                   float64 exchanges instead of 48 -- and lane 8 e stores sum e of the wave's 512
//                                   pixels into `work` (or into `frames` when the detector has one wave tile).
//                     A frame's partial sums depend on that frame's values and the pixel -> (wave tile, lane, slot) map
//                     alone, never on the range or on the other frames.
//   k_fit_fold        adds the wave tiles of every frame and the ranges of every pixel in index order.
//
// The partition and the words of `work` are FitPart, an instance of frame_part.hpp's plain C++: tests/test_fit_cpu.py
// builds host_fit.cpp with the host compiler and checks that every (frame, pixel) pair and every word of `work` is
// visited exactly once.
#pragma once

#include "frame_part.hpp"

namespace pty {

// two groups of four pixels per lane: 512 pixels per wave, 2048 per workgroup; eight sums per frame, four maps
using FitPart = FramePart<4, 2, 8, 4>;
constexpr unsigned long long kFitMaxAngles = 65535;          // gridDim.z
constexpr unsigned long long kFitMaxDim = 0x7fffffffull;     // nscan, npix
constexpr unsigned long long kFitMaxElems = 1ull << 59;      // ptheta * nscan * npix: byte offsets stay in 64 bits

PTY_HD bool fit_sizes_ok(const unsigned long long ptheta, const unsigned long long nscan, const unsigned long long npix) {
    if (ptheta == 0 || nscan == 0 || npix == 0) return false;
    if (ptheta > kFitMaxAngles || nscan > kFitMaxDim || npix > kFitMaxDim) return false;
    if (ptheta * nscan > kFitMaxElems / npix) return false;   // ptheta * nscan < 2^47: no overflow on the left
    return true;
}

#if defined(__HIPCC__)

// v_sqrt_f32 / v_log_f32 (1 ulp), as k_rows.hpp
__device__ __forceinline__ float fit_sqrt(const float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float fit_ln(const float x) { return 0.693147180559945309f * __builtin_amdgcn_logf(x); }

// |g|^2 = re re + im im with both products rounded: no fused multiply-add, so that a NumPy float32 restatement and
// every caller of this function get the same bits
__device__ __forceinline__ float fit_abs2(const c32 v) {
#pragma clang fp contract(off)
    const float a = v.x * v.x, b = v.y * v.y;
    return a + b;
}

// grid ceil(count / 1024), 256 threads; vec: inten and g are 16-byte aligned
__global__ __launch_bounds__(256) void k_fit_accumulate(float* __restrict__ inten, const c32* __restrict__ g,
                                                        const size_t count, const int add, const int vec) {
    const size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= count) return;
    if (vec && i + 4 <= count) {
        const vec4f g0 = *(const vec4f*)(g + i), g1 = *(const vec4f*)(g + i + 2);
        vec4f v = vec4f{fit_abs2(c32{g0.x, g0.y}), fit_abs2(c32{g0.z, g0.w}), fit_abs2(c32{g1.x, g1.y}),
                        fit_abs2(c32{g1.z, g1.w})};
        if (add) {
#pragma clang fp contract(off)
            v = *(const vec4f*)(inten + i) + v;
        }
        *(vec4f*)(inten + i) = v;
    } else {
        for (size_t k = i; k < i + 4 && k < count; ++k) {
#pragma clang fp contract(off)
            const float v = fit_abs2(g[k]);
            inten[k] = add ? inten[k] + v : v;
        }
    }
}

struct FitArgs {
    double* fpart;         // [ptheta * nscan][nwt][8]: the frame part of work, or frames itself (nwt == 1)
    double* ppart;         // [ptheta][nranges][4][npix]: the pixel part of work, or pixels itself (nranges == 1)
    const float* inten;
    const c32* g;
    const float* data;
    const unsigned char* mask;
    const double* ab;
    long long npix, nwt;
    int nscan, flen;
};

struct FitRaw {
    float in[FitPart::kSlots];   // intensity of the other modes
    c32 g[FitPart::kSlots];
    float d[FitPart::kSlots];
};

// the lane's eight pixels of the frame that starts at element `base`.  Nothing is predicated: a pixel past the end of the
// detector (live[q] false; with VEC, npix % 4 == 0, a group is inside or outside as a whole) reads pixel 0 of the frame
// instead, and the caller drops it as it drops an unmeasured pixel
template <bool VEC>
__device__ __forceinline__ FitRaw fit_load(const FitArgs& a, const size_t base, const long long (&p0)[FitPart::kGroups],
                                           const bool (&live)[FitPart::kSlots]) {
    FitRaw r;
#pragma unroll
    for (int q = 0; q < FitPart::kSlots; ++q) {
        r.in[q] = 0.0f;
        r.g[q] = c32{0.0f, 0.0f};
    }
#pragma unroll
    for (int h = 0; h < FitPart::kGroups; ++h) {
        if constexpr (VEC) {
            const size_t at = base + (size_t)(live[h * FitPart::kLanePix] ? p0[h] : 0);
            const vec4f d = __builtin_nontemporal_load((const vec4f*)(a.data + at));
            r.d[4 * h] = d.x; r.d[4 * h + 1] = d.y; r.d[4 * h + 2] = d.z; r.d[4 * h + 3] = d.w;
            if (a.inten) {
                const vec4f v = __builtin_nontemporal_load((const vec4f*)(a.inten + at));
                r.in[4 * h] = v.x; r.in[4 * h + 1] = v.y; r.in[4 * h + 2] = v.z; r.in[4 * h + 3] = v.w;
            }
            if (a.g) {
                const vec4f g0 = __builtin_nontemporal_load((const vec4f*)(a.g + at));
                const vec4f g1 = __builtin_nontemporal_load((const vec4f*)(a.g + at + 2));
                r.g[4 * h] = c32{g0.x, g0.y}; r.g[4 * h + 1] = c32{g0.z, g0.w};
                r.g[4 * h + 2] = c32{g1.x, g1.y}; r.g[4 * h + 3] = c32{g1.z, g1.w};
            }
        } else {
#pragma unroll
            for (int k = 0; k < FitPart::kLanePix; ++k) {
                const int q = h * FitPart::kLanePix + k;
                const size_t at = base + (size_t)(live[q] ? p0[h] + k : 0);
                r.d[q] = a.data[at];
                if (a.inten) r.in[q] = a.inten[at];
                if (a.g) r.g[q] = a.g[at];
            }
        }
    }
    return r;
}

// the eight terms of one pixel (the table of include/ptycho_hip.h) and the signed amplitude residual, in float32.  An
// unmeasured pixel is given I = 0 and d = 0 by a select, not a product (it may hold anything), which makes every term
// an exact zero
__device__ __forceinline__ void fit_terms(const float inten, const c32 g, const float data, const float s2,
                                          const bool meas, float (&t)[FitPart::kCols], float& diff) {
#pragma clang fp contract(off)
    const float I = meas ? (inten + fit_abs2(g)) * s2 : 0.0f, d = meas ? data : 0.0f;
    const float sI = fit_sqrt(I), sd = fit_sqrt(d);
    diff = sI - sd;
    t[0] = I;
    t[1] = d;
    t[2] = fit_sqrt(I * d);
    t[3] = diff * diff;
    t[4] = I - d * fit_ln(I + 1e-32f);
    t[5] = d - d * fit_ln(d + 1e-32f);
    t[6] = fabsf(diff);
    t[7] = sd;
}

// of f[0 .. N): keep = f[k] or f[k + N / 2] by `hi`, the other half goes to the lane at distance `o` and its counterpart
// comes back
template <int N>
__device__ __forceinline__ void fit_halve(double (&f)[FitPart::kCols], const bool hi, const int o) {
#pragma unroll
    for (int k = 0; k < N / 2; ++k) {
        const double keep = hi ? f[k + N / 2] : f[k], send = hi ? f[k] : f[k + N / 2];
        f[k] = keep + __shfl_xor(send, o);
    }
}

// 8 vectors of 64 lanes -> lane 8 e stores sum e to dst[e]: bits 5, 4, 3 of the lane pick the half that is kept
__device__ __forceinline__ void fit_wave_sums(double (&f)[FitPart::kCols], const int lane, double* __restrict__ dst) {
    fit_halve<8>(f, (lane & 32) != 0, 32);
    fit_halve<4>(f, (lane & 16) != 0, 16);
    fit_halve<2>(f, (lane & 8) != 0, 8);
    double v = f[0];
    v += __shfl_xor(v, 4);
    v += __shfl_xor(v, 2);
    v += __shfl_xor(v, 1);
    if ((lane & 7) == 0) dst[lane >> 3] = v;
}

// one frame of one wave: the lane's pixels into pacc and into the eight sums, the sums over the wave, the store to dst
template <bool PIX>
__device__ __forceinline__ void fit_frame(const FitRaw& raw, const float s2, const bool (&meas)[FitPart::kSlots],
                                          double (&pacc)[PIX ? FitPart::kMaps : 1][FitPart::kSlots], const int lane,
                                          double* __restrict__ dst) {
    double f[FitPart::kCols];
#pragma unroll
    for (int e = 0; e < FitPart::kCols; ++e) f[e] = 0.0;
#pragma unroll
    for (int q = 0; q < FitPart::kSlots; ++q) {
        float tm[FitPart::kCols], diff;
        fit_terms(raw.in[q], raw.g[q], raw.d[q], s2, meas[q], tm, diff);
#pragma unroll
        for (int e = 0; e < FitPart::kCols; ++e) f[e] += (double)tm[e];
        if constexpr (PIX) {
            pacc[0][q] += (double)tm[0];
            pacc[1][q] += (double)tm[1];
            pacc[2][q] += (double)diff;
            pacc[3][q] += (double)tm[3];
        }
    }
    fit_wave_sums(f, lane, dst);
}

// grid (ntiles, nranges, ptheta), 256 threads
template <bool VEC, bool PIX>
__global__ __launch_bounds__(256) void k_fit_frames(const FitArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long wt = (long long)blockIdx.x * FitPart::kWaves + wave;
    if (wt >= a.nwt) return;   // waves are independent: no barrier below
    const long long r = blockIdx.y, t = blockIdx.z, npix = a.npix;
    long long p0[FitPart::kGroups];
    bool live[FitPart::kSlots], meas[FitPart::kSlots];
#pragma unroll
    for (int h = 0; h < FitPart::kGroups; ++h) p0[h] = FitPart::pixel(wt, lane, h);
#pragma unroll
    for (int q = 0; q < FitPart::kSlots; ++q) {
        const long long p = p0[q / FitPart::kLanePix] + q % FitPart::kLanePix;
        live[q] = p < npix;
        meas[q] = live[q] && (a.mask == nullptr || a.mask[p] != 0);
    }
    float s2 = 1.0f;
    if (a.ab) {
        const double s = a.ab[0] / a.ab[1];
        s2 = (float)(s * s);
    }
    const int j0 = (int)r * a.flen, j1 = j0 + a.flen < a.nscan ? j0 + a.flen : a.nscan;
    const size_t frame0 = (size_t)t * (size_t)a.nscan, snpix = (size_t)npix;
    double pacc[PIX ? FitPart::kMaps : 1][FitPart::kSlots];
#pragma unroll
    for (int m = 0; m < (PIX ? FitPart::kMaps : 1); ++m)
#pragma unroll
        for (int q = 0; q < FitPart::kSlots; ++q) pacc[m][q] = 0.0;

    // two buffers, frames alternate between them: a frame's loads are issued before the arithmetic of the frame before it
    FitRaw ra = fit_load<VEC>(a, (frame0 + (size_t)j0) * snpix, p0, live), rb = ra;
    for (int j = j0; j < j1; j += 2) {
        const size_t frame = frame0 + (size_t)j;
        if (j + 1 < j1) rb = fit_load<VEC>(a, (frame + 1) * snpix, p0, live);
        fit_frame<PIX>(ra, s2, meas, pacc, lane, a.fpart + FitPart::frame_word((long long)frame, wt, a.nwt));
        if (j + 1 >= j1) break;
        if (j + 2 < j1) ra = fit_load<VEC>(a, (frame + 2) * snpix, p0, live);
        fit_frame<PIX>(rb, s2, meas, pacc, lane, a.fpart + FitPart::frame_word((long long)frame + 1, wt, a.nwt));
    }
    if constexpr (PIX) {
#pragma unroll
        for (int m = 0; m < FitPart::kMaps; ++m) {
            double* dst = a.ppart + FitPart::pixel_word(t, r, m, gridDim.y, npix);
#pragma unroll
            for (int q = 0; q < FitPart::kSlots; ++q)
                if (live[q]) dst[p0[q / FitPart::kLanePix] + q % FitPart::kLanePix] = pacc[m][q];
        }
    }
}

// FramePart::fold, every column a sum; slab = 4 npix
__global__ __launch_bounds__(256) void k_fit_fold(double* __restrict__ frames, double* __restrict__ pixels,
                                                  const double* __restrict__ fpart, const double* __restrict__ ppart,
                                                  const long long nfout, const long long nwt, const long long npout,
                                                  const long long slab, const long long nranges,
                                                  const unsigned fblocks) {
    FitPart::fold<-1>(frames, pixels, fpart, ppart, nfout, nwt, npout, slab, nranges, fblocks);
}

#endif  // __HIPCC__

}  // namespace pty
