// k_gauge.hpp -- illumination map and gauge fixing (ptycho_illumination / ptycho_gauge_fit / ptycho_gauge_apply,
// libtike.hipfft.gauge).  No handle, no float atomics, every sum in a fixed order: the same inputs give the same bits.
//
//   k_illumination   one 256-thread workgroup per 64 x 16 tile of the object (wave w owns rows 4 w .. 4 w + 3, lane l
//                    column l).  The angle's positions go through LDS in chunks of 128: a thread splits one position
//                    (illum_split, the modff split of decode_xy), tests its (nprb + 1)^2 footprint against the tile
//                    (illum_overlaps) and the survivors are packed IN POSITION ORDER (ballot + popcount, wave totals
//                    through LDS).  Every thread then walks the packed list and adds, per position, the four taps of
//                    each of its four pixels in registers: out[Y, X] += w_ab A[Y - sy - a, X - sx - b], taps in the
//                    order (0,0) (0,1) (1,0) (1,1), w_ab the bilinear weights of kernels.cu:73-80.  A = sum_m |probe_m|^2
//                    is formed on the fly (the ABI has no scratch to hold it): five rows of the thread's column, the
//                    column to the left taken from the neighbouring lane (lane 0 loads its own), i.e. 1.25 M complex
//                    loads per pixel and position, all L1 / L2 hits.  Each pixel is written once: no zeroing pass.
//   k_gauge_sums     pass 1 of the fit: workgroup b of angle t owns rows b, b + nb, ..; per thread float64 sums of
//                    {Cx, Cy, W, sum w y, sum w x, sum w |psi|^2, sum w |ref|^2}, a shuffle tree per wave, the four
//                    waves added in order (block_sum, frame_part.hpp), one row of `work` per workgroup.
//   k_gauge_finish   stage 1: adds the rows in a fixed order and writes (gy, gx, 0, s, yc, xc) to gauge[t];
//                    stage 2: the same for pass 2's rows and writes phi0.
//   k_gauge_offset   pass 2: Z = sum w u exp(-i (gy (y - yc) + gx (x - xc))), the ramp read from gauge[t] on the device,
//                    the phase formed in float64 turns and reduced before sincospi.
//   k_gauge_apply    one thread per element, the phase as in pass 2.
//
// The staging of a chunk (barrier, split, overlap test, ballot, wave totals, packed store) is illum_stage, which
// k_scan_map (k_dpc.hpp) calls too.  Nothing else of k_illumination is shared with that kernel, on purpose: its low bits are
// whatever the compiler makes of its multiply-adds -- 6 packed FMAs and two packed multiply / add pairs left unfused in
// today's build -- and moving the walk of the packed list into a shared function (the taps as a lambda, the LDS arrays in a
// struct or as pointers, the weights formed inside or outside) made it 8 packed FMAs, i.e. another rounding; sharing the
// column gather (the v[k] / l[k] loads with __shfl_up) changed the float sequence as well.  With illum_stage alone the
// ordered list of float instructions, the registers, LDS and occupancy are those of the kernel written out in full
// (profiles/r18/walks_refactor.txt).  So: share what touches no float, and compare the listing after any change here
// (tools/isa_compare.py --float=k_illumination).
//
// The index logic of k_illumination (split, overlap test, tap -> probe index) is plain C++: illum_walk.hpp walks it on the
// host as the kernels do, and tests/test_gauge_cpu.py builds host_gauge.cpp with the host compiler and checks that every
// (position, tap, pixel) contribution is visited exactly once.
#pragma once

#include <cmath>

#include "frame_part.hpp"

namespace pty {

constexpr int kIllTileW = 64, kIllTileH = 16;   // one wave per 64 x 4 block of pixels
constexpr int kIllRows = 4;                     // rows per thread
constexpr int kIllChunk = 128;                  // positions staged per pass through LDS, as load_run's kRunMax
constexpr unsigned long long kGaugeMaxAngles = 65535;          // gridDim.y / gridDim.z
constexpr unsigned long long kGaugeMaxSide = 1ull << 30;       // object / probe sides: pixel indices stay in int
constexpr int kGaugeMaxBlocks = 1024;           // workgroups per angle of the two reduction passes
constexpr int kGaugeStride = 16;                // float64 words per workgroup row of `work`: 0..8 pass 1, 9..10 pass 2
// include/ptycho_hip.h: PTYCHO_GAUGE_WORK_PER_ANGLE == kGaugeMaxBlocks * kGaugeStride

// modff split of one scan coordinate, exactly as decode_xy (ptycho_common.hpp) does it; false: the position is skipped
PTY_HD bool illum_split(const float p, int& s, float& f) {
    float ip;
    f = modff(p, &ip);
    const bool valid = !(ip < 0.0f) && (ip < 1.0e9f) && (ip == ip);
    s = valid ? (int)ip : 0;
    return valid;
}

// does the footprint rows sy .. sy + nprb, columns sx .. sx + nprb meet the tile at (y0, x0), clipped to the object?
PTY_HD bool illum_overlaps(const int sy, const int sx, const int nprb, const int y0, const int x0, const int nz,
                           const int n) {
    const int y1 = (y0 + kIllTileH < nz ? y0 + kIllTileH : nz) - 1, x1 = (x0 + kIllTileW < n ? x0 + kIllTileW : n) - 1;
    return sy <= y1 && sy + nprb >= y0 && sx <= x1 && sx + nprb >= x0;
}

PTY_HD bool illum_inside(const int iy, const int ix, const int nprb) { return iy >= 0 && iy < nprb && ix >= 0 && ix < nprb; }

// probe index of the value that tap (a, b) of the position at (sy, sx) adds to pixel (Y, X); false: none
PTY_HD bool illum_src(const int Y, const int X, const int sy, const int sx, const int a, const int b, const int nprb,
                      int& iy, int& ix) {
    iy = Y - sy - a;
    ix = X - sx - b;
    return illum_inside(iy, ix, nprb);
}

// workgroups per angle of the reduction passes
PTY_HD int gauge_blocks(const long long nz) { return nz < kGaugeMaxBlocks ? (int)nz : kGaugeMaxBlocks; }

#if defined(__HIPCC__)

// sum_m |probe_m[iy, ix]|^2, zero outside the probe; prb: the angle's [nmodes][nprb][nprb]
__device__ __forceinline__ float illum_amp2(const c32* __restrict__ prb, const int nmodes, const int nprb, const int iy,
                                            const int ix) {
    float a = 0.0f;
    if (illum_inside(iy, ix, nprb)) {
        const size_t plane = (size_t)nprb * nprb, at = (size_t)iy * nprb + ix;
        for (int m = 0; m < nmodes; ++m) {
            const c32 p = prb[m * plane + at];
            a += p.x * p.x + p.y * p.y;
        }
    }
    return a;
}

// One chunk of kIllChunk positions from c0 on, staged for the tile at (y0, x0): thread tid < kIllChunk splits position
// c0 + tid and tests its footprint against the tile, and the survivors are packed IN POSITION ORDER into l_sy / l_sx /
// l_fy / l_fx (ballot + popcount within a wave, the wave totals through l_cnt).  Returns the number packed; at: the slot
// of the thread's own position, -1 if it was dropped -- a kernel that carries more per position stores it at that slot.
// Opens with the barrier that ends the walk of the chunk before; the caller places the barrier that ends the staging.
__device__ __forceinline__ int illum_stage(const float* __restrict__ sc, const int nscan, const int c0, const int nprb,
                                           const int y0, const int x0, const int nz, const int n, int* l_sy, int* l_sx,
                                           float* l_fy, float* l_fx, int* l_cnt, int& at) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    __syncthreads();   // the list of the chunk before has been walked by every wave
    int sy = 0, sx = 0;
    float fy = 0.0f, fx = 0.0f;
    bool keep = false;
    if (tid < kIllChunk && c0 + tid < nscan) {
        const size_t p = (size_t)(c0 + tid);
        const bool vy = illum_split(sc[2 * p], sy, fy), vx = illum_split(sc[2 * p + 1], sx, fx);
        keep = vy && vx && illum_overlaps(sy, sx, nprb, y0, x0, nz, n);
    }
    const unsigned long long m = __ballot(keep);
    if (lane == 0) l_cnt[wave] = __popcll(m);
    __syncthreads();
    int base = 0, total = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        const int c = l_cnt[w];
        base += w < wave ? c : 0;
        total += c;
    }
    at = -1;
    if (keep) {
        at = base + __popcll(m & ((1ull << lane) - 1ull));
        l_sy[at] = sy; l_sx[at] = sx; l_fy[at] = fy; l_fx[at] = fx;
    }
    return total;
}

// grid (ceil(n / 64), ceil(nz / 16), ptheta), 256 threads
__global__ __launch_bounds__(256) void k_illumination(float* __restrict__ out, const float* __restrict__ scan,
                                                      const c32* __restrict__ probe, const int nscan, const int nmodes,
                                                      const int nprb, const int nz, const int n) {
    __shared__ int l_sy[kIllChunk], l_sx[kIllChunk];
    __shared__ float l_fy[kIllChunk], l_fx[kIllChunk];
    __shared__ int l_cnt[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int t = blockIdx.z, y0 = blockIdx.y * kIllTileH, x0 = blockIdx.x * kIllTileW;
    const int X = x0 + lane, Y0 = y0 + wave * kIllRows;
    const float* sc = scan + (size_t)t * nscan * 2;
    const c32* prb = probe + (size_t)t * nmodes * nprb * nprb;
    float acc[kIllRows] = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int c0 = 0; c0 < nscan; c0 += kIllChunk) {
        int at;
        const int total = illum_stage(sc, nscan, c0, nprb, y0, x0, nz, n, l_sy, l_sx, l_fy, l_fx, l_cnt, at);
        __syncthreads();
        for (int i = 0; i < total; ++i) {
            const int py = __builtin_amdgcn_readfirstlane(l_sy[i]), px = __builtin_amdgcn_readfirstlane(l_sx[i]);
            const float qy = l_fy[i], qx = l_fx[i];
            // kernels.cu:73-80: (1 - sxf) (1 - syf), sxf (1 - syf), (1 - sxf) syf, sxf syf
            const float wx0 = 1.0f - qx, wy0 = 1.0f - qy;
            const float w00 = wx0 * wy0, w01 = qx * wy0, w10 = wx0 * qy, w11 = qx * qy;
            int iy0, ix;   // tap (0, 0) at the thread's first row; tap (a, b) of row r reads A[iy0 + r - a, ix - b]
            (void)illum_src(Y0, X, py, px, 0, 0, nprb, iy0, ix);
            // v[k] = A[iy0 - 1 + k, ix]; l[k] = A[iy0 - 1 + k, ix - 1]: the lane to the left holds it as its own v[k]
            float v[kIllRows + 1], l[kIllRows + 1];
#pragma unroll
            for (int k = 0; k <= kIllRows; ++k) v[k] = illum_amp2(prb, nmodes, nprb, iy0 - 1 + k, ix);
#pragma unroll
            for (int k = 0; k <= kIllRows; ++k) l[k] = __shfl_up(v[k], 1);
            if (lane == 0) {
#pragma unroll
                for (int k = 0; k <= kIllRows; ++k) l[k] = illum_amp2(prb, nmodes, nprb, iy0 - 1 + k, ix - 1);
            }
#pragma unroll
            for (int r = 0; r < kIllRows; ++r) {
                acc[r] += w00 * v[r + 1];
                acc[r] += w01 * l[r + 1];
                acc[r] += w10 * v[r];
                acc[r] += w11 * l[r];
            }
        }
    }
    if (X < n) {
#pragma unroll
        for (int r = 0; r < kIllRows; ++r)
            if (Y0 + r < nz) out[((size_t)t * nz + (size_t)(Y0 + r)) * (size_t)n + (size_t)X] = acc[r];
    }
}

// ---- gauge fit ----------------------------------------------------------------------------------------------------------
struct GaugePix {
    double ur, ui, w, p2, r2;
};
// element idx: u = psi conj(ref) (psi without ref), the weight (1 without weight), |psi|^2 and |ref|^2 (1 without ref)
__device__ __forceinline__ GaugePix gauge_pix(const c32* __restrict__ psi, const c32* __restrict__ ref,
                                              const float* __restrict__ weight, const size_t idx) {
    GaugePix g;
    g.w = weight ? (double)weight[idx] : 1.0;
    const c32 p = psi[idx];
    const double pr = p.x, pi = p.y;
    g.ur = pr;
    g.ui = pi;
    g.p2 = pr * pr + pi * pi;
    g.r2 = 1.0;
    if (ref) {
        const c32 r = ref[idx];
        const double rr = r.x, ri = r.y;
        g.ur = pr * rr + pi * ri;
        g.ui = pi * rr - pr * ri;
        g.r2 = rr * rr + ri * ri;
    }
    return g;
}

// grid (nb, ptheta), 256 threads; work: float64 [ptheta][kGaugeMaxBlocks][kGaugeStride]
__global__ __launch_bounds__(256) void k_gauge_sums(double* __restrict__ work, const c32* __restrict__ psi,
                                                    const c32* __restrict__ ref, const float* __restrict__ weight,
                                                    const int nz, const int n) {
    __shared__ double part[4 * 9];
    const int t = blockIdx.y, nb = gridDim.x, tid = threadIdx.x;
    // Re Cx, Im Cx, Re Cy, Im Cy, W, sum w y, sum w x, sum w |psi|^2, sum w |ref|^2
    double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int y = blockIdx.x; y < nz; y += nb) {
        const size_t row = ((size_t)t * nz + (size_t)y) * (size_t)n;
        for (int x = tid; x < n; x += 256) {
            const size_t idx = row + (size_t)x;
            const GaugePix g = gauge_pix(psi, ref, weight, idx);
            if (!(g.w > 0.0)) continue;   // a pixel of no weight enters no sum: it may hold anything
            v[4] += g.w;
            v[5] += g.w * y;
            v[6] += g.w * x;
            v[7] += g.w * g.p2;
            v[8] += g.w * g.r2;
            if (x + 1 < n) {
                const GaugePix h = gauge_pix(psi, ref, weight, idx + 1);
                if (h.w > 0.0) {   // u[y, x + 1] conj(u[y, x])
                    const double ww = g.w * h.w;
                    v[0] += ww * (h.ur * g.ur + h.ui * g.ui);
                    v[1] += ww * (h.ui * g.ur - h.ur * g.ui);
                }
            }
            if (y + 1 < nz) {
                const GaugePix h = gauge_pix(psi, ref, weight, idx + (size_t)n);
                if (h.w > 0.0) {
                    const double ww = g.w * h.w;
                    v[2] += ww * (h.ur * g.ur + h.ui * g.ui);
                    v[3] += ww * (h.ui * g.ur - h.ur * g.ui);
                }
            }
        }
    }
    block_sum<9>(v, work + ((size_t)t * kGaugeMaxBlocks + blockIdx.x) * kGaugeStride, part);
}

// exp(2 pi i turns), turns reduced to [-1/2, 1/2] first
__device__ __forceinline__ void gauge_cis_turns(double turns, double& cs, double& sn) {
    turns -= rint(turns);
    sincospi(2.0 * turns, &sn, &cs);
}
// (gy (y - yc) + gx (x - xc)) / (2 pi) in turns, each term reduced
__device__ __forceinline__ double gauge_ramp_turns(const double gy, const double gx, const double dy, const double dx) {
    constexpr double inv2pi = 0.15915494309189533577;
    double a = gy * dy * inv2pi, b = gx * dx * inv2pi;
    a -= rint(a);
    b -= rint(b);
    return a + b;
}

// grid (nb, ptheta), 256 threads: Z of angle t with the ramp and the centre of gauge[t] (k_gauge_finish, stage 1)
__global__ __launch_bounds__(256) void k_gauge_offset(double* __restrict__ work, const c32* __restrict__ psi,
                                                      const c32* __restrict__ ref, const float* __restrict__ weight,
                                                      const int nz, const int n, const double* __restrict__ gauge) {
    __shared__ double part[4 * 2];
    const int t = blockIdx.y, nb = gridDim.x, tid = threadIdx.x;
    const double gy = gauge[6 * t], gx = gauge[6 * t + 1], yc = gauge[6 * t + 4], xc = gauge[6 * t + 5];
    double v[2] = {0.0, 0.0};
    for (int y = blockIdx.x; y < nz; y += nb) {
        const size_t row = ((size_t)t * nz + (size_t)y) * (size_t)n;
        for (int x = tid; x < n; x += 256) {
            const GaugePix g = gauge_pix(psi, ref, weight, row + (size_t)x);
            if (!(g.w > 0.0)) continue;
            double cs, sn;
            gauge_cis_turns(gauge_ramp_turns(gy, gx, (double)y - yc, (double)x - xc), cs, sn);
            v[0] += g.w * (g.ur * cs + g.ui * sn);   // w u exp(-i ph)
            v[1] += g.w * (g.ui * cs - g.ur * sn);
        }
    }
    block_sum<2>(v, work + ((size_t)t * kGaugeMaxBlocks + blockIdx.x) * kGaugeStride + 9, part);
}

__device__ __forceinline__ double gauge_arg(const double re, const double im) {
    return (re == 0.0 && im == 0.0) ? 0.0 : atan2(im, re);
}

// grid (ptheta), 256 threads.  stage 1: rows of pass 1 -> gauge[t] = (gy, gx, 0, s, yc, xc); stage 2: rows of pass 2 -> phi0
__global__ __launch_bounds__(256) void k_gauge_finish(double* __restrict__ gauge, const double* __restrict__ work,
                                                      const int nb, const int stage) {
    __shared__ double part[4 * 9];
    __shared__ double tot[9];
    const int t = blockIdx.x, tid = threadIdx.x;
    const double* rows = work + (size_t)t * kGaugeMaxBlocks * kGaugeStride;
    double* g = gauge + 6 * (size_t)t;
    if (stage == 1) {
        double v[9] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int b = tid; b < nb; b += 256) {
#pragma unroll
            for (int e = 0; e < 9; ++e) v[e] += rows[(size_t)b * kGaugeStride + e];
        }
        block_sum<9>(v, tot, part);
        __syncthreads();
        if (tid == 0) {
            const double W = tot[4];
            if (W > 0.0) {
                g[0] = gauge_arg(tot[2], tot[3]);
                g[1] = gauge_arg(tot[0], tot[1]);
                g[2] = 0.0;
                g[3] = (tot[7] > 0.0 && tot[8] > 0.0) ? sqrt(tot[7] / tot[8]) : 1.0;
                g[4] = tot[5] / W;
                g[5] = tot[6] / W;
            } else {
                g[0] = 0.0; g[1] = 0.0; g[2] = 0.0; g[3] = 1.0; g[4] = 0.0; g[5] = 0.0;
            }
        }
    } else {
        double v[2] = {0.0, 0.0};
        for (int b = tid; b < nb; b += 256) {
            v[0] += rows[(size_t)b * kGaugeStride + 9];
            v[1] += rows[(size_t)b * kGaugeStride + 10];
        }
        block_sum<2>(v, tot, part);
        __syncthreads();
        if (tid == 0) g[2] = gauge_arg(tot[0], tot[1]);
    }
}

// grid (ceil(nx / 256) ny, ptheta), 256 threads; xb = ceil(nx / 256)
__global__ __launch_bounds__(256) void k_gauge_apply(c32* __restrict__ x, const double* __restrict__ gauge, const int ny,
                                                     const int nx, const int xb, const int which) {
    const int t = blockIdx.y, y = blockIdx.x / xb, col = (blockIdx.x % xb) * 256 + threadIdx.x;
    if (col >= nx) return;
    constexpr double inv2pi = 0.15915494309189533577;
    const double* g = gauge + 6 * (size_t)t;
    const double gy = g[0], gx = g[1], s = g[3];
    double turns, scale;
    if (which == 0) {   // object: exp(-i (phi0 + gy (y - yc) + gx (x - xc))) / s
        double p0 = g[2] * inv2pi;
        p0 -= rint(p0);
        turns = -(p0 + gauge_ramp_turns(gy, gx, (double)y - g[4], (double)col - g[5]));
        scale = 1.0 / s;
    } else {            // probe companion: s exp(+i (gy y + gx x)), local coordinates
        turns = gauge_ramp_turns(gy, gx, (double)y, (double)col);
        scale = s;
    }
    double cs, sn;
    gauge_cis_turns(turns, cs, sn);
    const size_t idx = ((size_t)t * ny + (size_t)y) * (size_t)nx + (size_t)col;
    const c32 v = x[idx];
    const double vr = v.x, vi = v.y;
    x[idx] = c32{(float)((vr * cs - vi * sn) * scale), (float)((vr * sn + vi * cs) * scale)};
}

#endif  // __HIPCC__

}  // namespace pty
