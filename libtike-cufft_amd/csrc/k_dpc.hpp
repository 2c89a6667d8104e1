// k_dpc.hpp -- a first look at a scan before any reconstruction (ptycho_frame_moments / ptycho_scan_map /
// ptycho_integrate_*, libtike.hipfft.dpc): the moments of every diffraction pattern, per-position values spread over the
// object grid with the illumination's weights, and the integration of a gradient field.  No handle, no float atomics,
// every sum in a fixed order: the same inputs give the same bits.  include/ptycho_hip.h and DESIGN.md section 18 state
// the definitions.
//
//   k_frame_moments     one pass over data, the partition of k_fit_frames (MomPart, an instance of frame_part.hpp): a
//                       workgroup of four independent waves owns a tile of pixels and one range of frames, a lane two
//                       groups of four consecutive pixels (one 16-byte load per group and frame), the next frame's loads
//                       issued before this frame's arithmetic.  The signed frequencies (k_y, k_x) of the lane's eight
//                       pixels, whether each is measured and whether it lies outside the dark-field radius are formed
//                       once; per frame the eight terms (double) I k are added in float64 over the lane's pixels, then
//                       over the wave (fit_wave_sums, k_fit.hpp).  An unmeasured pixel gets I = 0 by a select.
//   k_frame_moments_fold  adds the wave tiles of every frame in index order.
//   k_scan_keep         a copy of scan with NaN at the positions that keep excludes: every walk skips them.
//   k_scan_map          k_illumination's tile and walk (k_gauge.hpp) over its index helpers and its staging itself
//                       (illum_stage), with the NVAL values of every position stored beside the packed list in LDS at the
//                       slot that illum_stage returns: per channel num += (w_ab A) v_j, every operation rounded, taps
//                       outside the probe dropped by a select; out = num / weight where weight > 0, else 0.  The weight is
//                       not formed again: the launcher runs k_illumination itself on the same scan first and this kernel
//                       reads its result -- the compiler fuses some of that kernel's multiply-adds and not others, so only
//                       the kernel itself gives ptycho_illumination's bits, which is also why the two kernels share the
//                       staging and not the walk (k_gauge.hpp's header).  map_amp2 / illum_amp2 stay two functions: their
//                       contraction differs on purpose.
//   k_integrate_offset  flat: parts of sum w' [D > 0] x and sum w' [D > 0] in float64.
//   k_integrate_mean    one workgroup per angle: adds the parts in index order, c = sum w' x / sum w' -> state.
//   k_integrate_finish  flat: out = x - c where D > 0, else 0.
// The setup of the integration is k_unwrap_setup<VEC, UnwGradSrc> (k_unwrap.hpp) and its iterations are the unwrapper's.
//
// The index logic (moment_k, the partition, the walk's helpers, the tile / halo slots) is plain C++: tests/test_dpc_cpu.py
// builds host_dpc.cpp with the host compiler and walks it (frame_part_walk.hpp, illum_walk.hpp, unwrap_walk.hpp).
#pragma once

#include "frame_part.hpp"
#include "k_fit.hpp"
#include "k_gauge.hpp"
#include "k_unwrap.hpp"

namespace pty {

// two groups of four pixels per lane, eight sums per frame, no per-pixel map
using MomPart = FramePart<4, 2, 8, 0>;
constexpr int kMapMaxVal = 4;   // channels of one ptycho_scan_map call

// signed frequency index of row / column r of an ndet-point transform with DC at 0: np.fft.fftfreq(ndet) * ndet
PTY_HD int moment_k(const int r, const int ndet) { return r < ndet - ndet / 2 ? r : r - ndet; }

#if defined(__HIPCC__)

struct MomArgs {
    double* fpart;         // [ptheta * nscan][nwt][8]: work, or moments itself (nwt == 1)
    const float* data;
    const unsigned char* mask;
    double r2;             // dark-field radius squared; negative: no dark field
    long long npix, nwt;
    int nscan, flen, ndet;
};

struct MomRaw {
    float d[MomPart::kSlots];
};

// the lane's eight pixels of the frame that starts at element `base`, as fit_load: a pixel past the end of the detector
// reads pixel 0 and the caller drops it
template <bool VEC>
__device__ __forceinline__ MomRaw mom_load(const float* __restrict__ data, const size_t base,
                                           const long long (&p0)[MomPart::kGroups], const bool (&live)[MomPart::kSlots]) {
    MomRaw r;
#pragma unroll
    for (int h = 0; h < MomPart::kGroups; ++h) {
        if constexpr (VEC) {
            const size_t at = base + (size_t)(live[h * MomPart::kLanePix] ? p0[h] : 0);
            const vec4f d = __builtin_nontemporal_load((const vec4f*)(data + at));
            r.d[4 * h] = d.x; r.d[4 * h + 1] = d.y; r.d[4 * h + 2] = d.z; r.d[4 * h + 3] = d.w;
        } else {
#pragma unroll
            for (int k = 0; k < MomPart::kLanePix; ++k) {
                const int q = h * MomPart::kLanePix + k;
                r.d[q] = data[base + (size_t)(live[q] ? p0[h] + k : 0)];
            }
        }
    }
    return r;
}

// one frame of one wave: the eight terms of the lane's pixels, the sums over the wave, the store to dst
__device__ __forceinline__ void mom_frame(const MomRaw& raw, const float (&ky)[MomPart::kSlots],
                                          const float (&kx)[MomPart::kSlots], const bool (&meas)[MomPart::kSlots],
                                          const bool (&dark)[MomPart::kSlots], const int lane, double* __restrict__ dst) {
#pragma clang fp contract(off)
    double f[MomPart::kCols];
#pragma unroll
    for (int e = 0; e < MomPart::kCols; ++e) f[e] = 0.0;
#pragma unroll
    for (int q = 0; q < MomPart::kSlots; ++q) {
        const double I = meas[q] ? (double)raw.d[q] : 0.0, y = (double)ky[q], x = (double)kx[q];
        f[0] += I;
        f[1] += I * y;
        f[2] += I * x;
        f[3] += I * (y * y);   // the frequencies are integers below 2^16: their products are exact
        f[4] += I * (x * x);
        f[5] += I * (y * x);
        f[6] += dark[q] ? I : 0.0;
    }
    fit_wave_sums(f, lane, dst);
}

// grid (ntiles, nranges, ptheta), 256 threads
template <bool VEC>
__global__ __launch_bounds__(256) void k_frame_moments(const MomArgs a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const long long wt = (long long)blockIdx.x * MomPart::kWaves + wave;
    if (wt >= a.nwt) return;   // waves are independent: no barrier below
    const long long r = blockIdx.y, t = blockIdx.z, npix = a.npix;
    long long p0[MomPart::kGroups];
    bool live[MomPart::kSlots], meas[MomPart::kSlots], dark[MomPart::kSlots];
    float ky[MomPart::kSlots], kx[MomPart::kSlots];
#pragma unroll
    for (int h = 0; h < MomPart::kGroups; ++h) p0[h] = MomPart::pixel(wt, lane, h);
#pragma unroll
    for (int q = 0; q < MomPart::kSlots; ++q) {
        const long long p = p0[q / MomPart::kLanePix] + q % MomPart::kLanePix;
        live[q] = p < npix;
        meas[q] = live[q] && (a.mask == nullptr || a.mask[p] != 0);
        const int row = live[q] ? (int)(p / a.ndet) : 0, col = live[q] ? (int)(p % a.ndet) : 0;
        const int iy = moment_k(row, a.ndet), ix = moment_k(col, a.ndet);
        ky[q] = (float)iy;
        kx[q] = (float)ix;
        dark[q] = meas[q] && a.r2 >= 0.0 && (double)iy * iy + (double)ix * ix > a.r2;
    }
    const int j0 = (int)r * a.flen, j1 = j0 + a.flen < a.nscan ? j0 + a.flen : a.nscan;
    const size_t frame0 = (size_t)t * (size_t)a.nscan, snpix = (size_t)npix;

    // two buffers, frames alternate between them: a frame's loads are issued before the arithmetic of the frame before it
    MomRaw ra = mom_load<VEC>(a.data, (frame0 + (size_t)j0) * snpix, p0, live), rb = ra;
    for (int j = j0; j < j1; j += 2) {
        const size_t frame = frame0 + (size_t)j;
        if (j + 1 < j1) rb = mom_load<VEC>(a.data, (frame + 1) * snpix, p0, live);
        mom_frame(ra, ky, kx, meas, dark, lane, a.fpart + MomPart::frame_word((long long)frame, wt, a.nwt));
        if (j + 1 >= j1) break;
        if (j + 2 < j1) ra = mom_load<VEC>(a.data, (frame + 2) * snpix, p0, live);
        mom_frame(rb, ky, kx, meas, dark, lane, a.fpart + MomPart::frame_word((long long)frame + 1, wt, a.nwt));
    }
}

// FramePart::fold, every column a sum, no pixel part
__global__ __launch_bounds__(256) void k_frame_moments_fold(double* __restrict__ frames, double* __restrict__ pixels,
                                                            const double* __restrict__ fpart,
                                                            const double* __restrict__ ppart, const long long nfout,
                                                            const long long nwt, const long long npout,
                                                            const long long slab, const long long nranges,
                                                            const unsigned fblocks) {
    MomPart::fold<-1>(frames, pixels, fpart, ppart, nfout, nwt, npout, slab, nranges, fblocks);
}

// sum_m |probe_m[iy, ix]|^2 as illum_amp2 (k_gauge.hpp) states it, zero outside the probe, with both squares and every
// sum rounded (no fused multiply-add): the float32 restatement in NumPy forms the same bits
__device__ __forceinline__ float map_amp2(const c32* __restrict__ prb, const int nmodes, const int nprb, const int iy,
                                          const int ix) {
#pragma clang fp contract(off)
    float a = 0.0f;
    if (illum_inside(iy, ix, nprb)) {
        const size_t plane = (size_t)nprb * nprb, at = (size_t)iy * nprb + ix;
        for (int m = 0; m < nmodes; ++m) {
            const c32 p = prb[m * plane + at];
            const float re2 = p.x * p.x, im2 = p.y * p.y;
            a = a + (re2 + im2);
        }
    }
    return a;
}

// num += (w A) v for every channel where the tap lies inside the probe (a select: outside, v may hold anything)
template <int NVAL>
__device__ __forceinline__ void map_tap(float (&num)[NVAL], const bool in, const float w, const float A,
                                        const float (&val)[NVAL]) {
#pragma clang fp contract(off)
    const float wa = w * A;
#pragma unroll
    for (int c = 0; c < NVAL; ++c) {
        const float term = wa * val[c];
        num[c] = in ? num[c] + term : num[c];
    }
}

// grid (ceil(ptheta nscan / 256)), 256 threads: out = scan with (NaN, NaN) at every position whose keep byte is zero -- a
// position that every walk skips, so that what is left is the kept subset in its order
__global__ __launch_bounds__(256) void k_scan_keep(float* __restrict__ out, const float* __restrict__ scan,
                                                   const unsigned char* __restrict__ keep, const size_t count) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const bool on = keep[i] != 0;
    out[2 * i] = on ? scan[2 * i] : NAN;
    out[2 * i + 1] = on ? scan[2 * i + 1] : NAN;
}

// grid (ceil(n / 64), ceil(nz / 16), ptheta), 256 threads: k_illumination's tile and walk (k_gauge.hpp) over its index
// helpers and illum_stage.  weight: [ptheta][nz][n], written by the launch of k_illumination on the same scan before this one;
// out: [ptheta][NVAL][nz][n], num / weight or, with raw, num itself; values: [ptheta][nscan][NVAL], staged beside the packed list
template <int NVAL>
__global__ __launch_bounds__(256) void k_scan_map(float* __restrict__ out, const float* __restrict__ weight,
                                                  const float* __restrict__ values, const float* __restrict__ scan,
                                                  const c32* __restrict__ probe, const int nscan, const int nmodes,
                                                  const int nprb, const int nz, const int n, const int raw) {
    __shared__ int l_sy[kIllChunk], l_sx[kIllChunk];
    __shared__ float l_fy[kIllChunk], l_fx[kIllChunk], l_v[kIllChunk][NVAL];
    __shared__ int l_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.z, y0 = blockIdx.y * kIllTileH, x0 = blockIdx.x * kIllTileW;
    const int X = x0 + lane, Y0 = y0 + wave * kIllRows;
    const float* sc = scan + (size_t)t * nscan * 2;
    const float* vals = values + (size_t)t * nscan * NVAL;
    const c32* prb = probe + (size_t)t * nmodes * nprb * nprb;
    float num[kIllRows][NVAL];
#pragma unroll
    for (int r = 0; r < kIllRows; ++r)
#pragma unroll
        for (int c = 0; c < NVAL; ++c) num[r][c] = 0.0f;
    for (int c0 = 0; c0 < nscan; c0 += kIllChunk) {
        int at;
        const int total = illum_stage(sc, nscan, c0, nprb, y0, x0, nz, n, l_sy, l_sx, l_fy, l_fx, l_cnt, at);
        if (at >= 0) {   // the position's values beside it in the packed list
#pragma unroll
            for (int c = 0; c < NVAL; ++c) l_v[at][c] = vals[(size_t)(c0 + tid) * NVAL + c];
        }
        __syncthreads();
        for (int i = 0; i < total; ++i) {
            const int py = __builtin_amdgcn_readfirstlane(l_sy[i]), px = __builtin_amdgcn_readfirstlane(l_sx[i]);
            float w00, w01, w10, w11;
            {
#pragma clang fp contract(off)
                const float qy = l_fy[i], qx = l_fx[i], wx0 = 1.0f - qx, wy0 = 1.0f - qy;
                w00 = wx0 * wy0; w01 = qx * wy0; w10 = wx0 * qy; w11 = qx * qy;
            }
            int iy0, ix;   // tap (0, 0) at the thread's first row; tap (a, b) of row r reads A[iy0 + r - a, ix - b]
            (void)illum_src(Y0, X, py, px, 0, 0, nprb, iy0, ix);
            // v[k] = A[iy0 - 1 + k, ix]; l[k] = A[iy0 - 1 + k, ix - 1]: the lane to the left holds it as its own v[k]
            float v[kIllRows + 1], l[kIllRows + 1], val[NVAL];
#pragma unroll
            for (int k = 0; k <= kIllRows; ++k) v[k] = map_amp2(prb, nmodes, nprb, iy0 - 1 + k, ix);
#pragma unroll
            for (int k = 0; k <= kIllRows; ++k) l[k] = __shfl_up(v[k], 1);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k <= kIllRows; ++k) l[k] = map_amp2(prb, nmodes, nprb, iy0 - 1 + k, ix - 1);
            }
#pragma unroll
            for (int c = 0; c < NVAL; ++c) val[c] = l_v[i][c];
#pragma unroll
            for (int r = 0; r < kIllRows; ++r) {
                const int iy = iy0 + r;   // tap (a, b) reads A[iy - a, ix - b]
                map_tap<NVAL>(num[r], illum_inside(iy, ix, nprb), w00, v[r + 1], val);
                map_tap<NVAL>(num[r], illum_inside(iy, ix - 1, nprb), w01, l[r + 1], val);
                map_tap<NVAL>(num[r], illum_inside(iy - 1, ix, nprb), w10, v[r], val);
                map_tap<NVAL>(num[r], illum_inside(iy - 1, ix - 1, nprb), w11, l[r], val);
            }
        }
    }
    if (X < n) {
        const size_t plane = (size_t)nz * (size_t)n;
#pragma unroll
        for (int r = 0; r < kIllRows; ++r) {
            if (Y0 + r >= nz) continue;
            const size_t at = (size_t)(Y0 + r) * (size_t)n + (size_t)X;
            const float w = weight[(size_t)t * plane + at];
#pragma unroll
            for (int c = 0; c < NVAL; ++c)
                out[((size_t)t * NVAL + c) * plane + at] = raw ? num[r][c] : (w > 0.0f ? __fdiv_rn(num[r][c], w) : 0.0f);
        }
    }
}

// grid (ceil(nz n / 1024), ptheta), 256 threads: parts of sum w' [D > 0] x and sum w' [D > 0]
template <bool VEC>
__global__ __launch_bounds__(256) void k_integrate_offset(const float* __restrict__ buf, const float* __restrict__ weight,
                                                          const size_t plane, const long long tiles,
                                                          double* __restrict__ work) {
    __shared__ double part[4 * 2];
    const int t = blockIdx.y;
    const float* base = buf + (size_t)t * kUnwPlanes * plane;
    size_t idx;
    const int have = unwrap_flat(plane, idx);
    double v[2] = {0.0, 0.0};
    if (have > 0) {
        float x[kUnwVec], mi[kUnwVec], w[kUnwVec] = {1.0f, 1.0f, 1.0f, 1.0f};
        unwrap_load4<VEC>(x, base, idx, have);
        unwrap_load4<VEC>(mi, base + 5 * plane, idx, have);
        if (weight) unwrap_load4<VEC>(w, weight + (size_t)t * plane, idx, have);
#pragma unroll
        for (int k = 0; k < kUnwVec; ++k) {
#pragma clang fp contract(off)
            const float wk = unwrap_wsel(w[k]);
            if (k < have && wk > 0.0f && mi[k] > 0.0f) {
                v[0] += (double)wk * (double)x[k];
                v[1] += (double)wk;
            }
        }
    }
    block_sum<2>(v, work + ((size_t)t * (size_t)tiles + blockIdx.x) * kUnwPart, part);
}

// grid (ptheta), 256 threads: the `rows` parts of k_integrate_offset in index order; c -> state[UNW_C]
__global__ __launch_bounds__(256) void k_integrate_mean(double* __restrict__ state, const double* __restrict__ work,
                                                        const long long rows, const long long tiles) {
    __shared__ double part[4 * 2];
    __shared__ double tot[2];
    const int t = blockIdx.x, tid = threadIdx.x;
    const double* w = work + (size_t)t * (size_t)tiles * kUnwPart;
    double v[2] = {0.0, 0.0};
    for (long long b = tid; b < rows; b += 256) {
        v[0] += w[(size_t)b * kUnwPart];
        v[1] += w[(size_t)b * kUnwPart + 1];
    }
    block_sum<2>(v, tot, part);
    __syncthreads();
    if (tid == 0) state[(size_t)t * kUnwStateWords + UNW_C] = tot[1] > 0.0 ? tot[0] / tot[1] : 0.0;
}

// grid (ceil(nz n / 1024), ptheta), 256 threads
template <bool VEC>
__global__ __launch_bounds__(256) void k_integrate_finish(float* __restrict__ out, const double* __restrict__ state,
                                                          const float* __restrict__ buf, const size_t plane) {
    const int t = blockIdx.y;
    const double c = state[(size_t)t * kUnwStateWords + UNW_C];
    const float* base = buf + (size_t)t * kUnwPlanes * plane;
    size_t idx;
    const int have = unwrap_flat(plane, idx);
    if (have == 0) return;
    float x[kUnwVec], mi[kUnwVec], o[kUnwVec];
    unwrap_load4<VEC>(x, base, idx, have);
    unwrap_load4<VEC>(mi, base + 5 * plane, idx, have);
#pragma unroll
    for (int k = 0; k < kUnwVec; ++k) o[k] = mi[k] > 0.0f ? (float)((double)x[k] - c) : 0.0f;   // no weighted edge: 0
    unwrap_store4<VEC>(out + (size_t)t * plane, idx, o, have);
}

#endif  // __HIPCC__

}  // namespace pty
