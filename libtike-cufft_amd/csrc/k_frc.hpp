// k_frc.hpp -- Fourier ring correlation of two images (ptycho_frc_prepare / ptycho_frc_rings, libtike.hipfft.frc).
//
// Two launches around the project's own FFT (ptycho_fft2 on a handle of detector size S):
//
//   k_frc_prepare   the S x S crops of a and b at (y0, x0), times the separable window w(y) w(x) (float32), into the
//                   complex64 scratch [2][ptheta][S][S] (a's crops, then b's); one thread per pixel, coalesced by row;
//   k_frc_rings     one 256-thread workgroup per (ring k, angle): per thread, float64 sums over the rows
//                   fy = fy_lo + t + 256 j of ring k, each row's one or two fx intervals walked in order; B is multiplied
//                   by the alignment ramp exp(-2 pi i (fy dy + fx dx) / S) on the fly (shift read from device memory, the
//                   phase reduced in float64); then a shuffle tree per wave and the four waves added in order, as in
//                   k_mode_gram_eig: no atomics, the same inputs give the same bits.  Output per (angle, ring):
//                   {Re C, Im C, PA, PB, n} with C = sum A conj(B), PA = sum |A|^2, PB = sum |B|^2.
//
// Ring k holds the integer frequencies (fy, fx) with round(sqrt(fy^2 + fx^2)) = k, i.e. r2 = fy^2 + fx^2 in
// [k^2 - k + 1, k^2 + k] (r2 = 0 for k = 0); only frequencies of numpy.fft.fftfreq(S) * S exist, and rings beyond S / 2
// are not formed.  frc_ring_row is plain C++, so tests/test_frc_cpu.py builds it on the host (host_frc.cpp) and checks
// that every pixel of every ring is visited exactly once.
#pragma once

#include <cmath>

#include "frame_part.hpp"

namespace pty {

constexpr int kFrcThreads = 256;
constexpr unsigned long long kFrcMaxAngles = 32767;   // 2 ptheta crops along gridDim.z of k_frc_prepare

// supported crop sides: those of ptycho_fft2 from 16 up
PTY_HD constexpr bool frc_size_ok(long long s) { return (s >= 16 && s <= 1024) || s == 2048; }

PTY_HD constexpr int frc_rings(int s) { return s / 2 + 1; }

// smallest and largest integer frequency of an S-point DFT (numpy.fft.fftfreq(S) * S)
PTY_HD constexpr int frc_fmin(int s) { return -(s / 2); }
PTY_HD constexpr int frc_fmax(int s) { return s - 1 - s / 2; }

// floor(sqrt(x)), x >= 0, exact for every x this file forms (< 2^40)
PTY_HD long long frc_isqrt(long long x) {
    long long m = (long long)std::sqrt((double)x);
    while (m * m > x) --m;
    while ((m + 1) * (m + 1) <= x) ++m;
    return m;
}

// The fx of row fy that lie in ring k, as the intervals [a0, b0] (fx >= 0) and [a1, b1] (fx < 0), clipped to the
// frequencies an S-point DFT has; an interval with a > b is empty.  fx = 0 belongs to the first interval only.
PTY_HD void frc_ring_row(const int k, const int fy, const int s, int& a0, int& b0, int& a1, int& b1) {
    a0 = a1 = 1;
    b0 = b1 = 0;
    const long long kk = k, fy2 = (long long)fy * fy;
    const long long rmin = k == 0 ? 0 : kk * kk - kk + 1, rmax = kk * kk + kk;
    if (fy2 > rmax) return;
    const long long hi = frc_isqrt(rmax - fy2);
    const long long lo2 = rmin > fy2 ? rmin - fy2 : 0;
    long long lo = frc_isqrt(lo2);
    if (lo * lo < lo2) ++lo;   // ceil(sqrt(lo2))
    if (lo > hi) return;
    const int fmax = frc_fmax(s), fmin = frc_fmin(s);
    a0 = (int)lo;
    b0 = hi < fmax ? (int)hi : fmax;
    a1 = -hi > fmin ? (int)-hi : fmin;
    b1 = lo > 0 ? (int)-lo : -1;
}

#if defined(__HIPCC__)

// grid (ceil(S / 256), S, 2 ptheta): thread x of row y of crop z (z < ptheta: a's angle z, else b's angle z - ptheta)
__global__ __launch_bounds__(256) void k_frc_prepare(c32* __restrict__ out, const c32* __restrict__ a,
                                                     const c32* __restrict__ b, const int ptheta, const long long nz,
                                                     const long long n, const long long y0, const long long x0,
                                                     const int s, const float* __restrict__ window) {
    const int x = blockIdx.x * 256 + threadIdx.x;
    if (x >= s) return;
    const int y = blockIdx.y, z = blockIdx.z;
    const int t = z < ptheta ? z : z - ptheta;
    const c32* src = z < ptheta ? a : b;
    c32 v = src[((size_t)t * nz + (size_t)(y0 + y)) * (size_t)n + (size_t)(x0 + x)];
    if (window) {
        const float w = window[y] * window[x];
        v = c32{v.x * w, v.y * w};
    }
    out[((size_t)z * s + y) * (size_t)s + x] = v;
}

// grid (K, ptheta), 256 threads.  spec: complex64 [2][ptheta][S][S] (A, then B); shift: float64 [ptheta][2] (dy, dx)
// or null; sums: float64 [ptheta][K][5].
__global__ __launch_bounds__(kFrcThreads) void k_frc_rings(double* __restrict__ sums, const c32* __restrict__ spec,
                                                           const int ptheta, const int s,
                                                           const double* __restrict__ shift) {
    __shared__ double part[4 * 5];
    const int k = blockIdx.x, ang = blockIdx.y;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const size_t plane = (size_t)s * s;
    const c32* A = spec + (size_t)ang * plane;
    const c32* B = spec + ((size_t)ptheta + ang) * plane;
    const bool ramp = shift != nullptr;
    const double dy = ramp ? shift[2 * ang] : 0.0, dx = ramp ? shift[2 * ang + 1] : 0.0;
    const int fmin = frc_fmin(s), fmax = frc_fmax(s);
    const int row_lo = -k > fmin ? -k : fmin, row_hi = k < fmax ? k : fmax;
    double cr = 0.0, ci = 0.0, pa = 0.0, pb = 0.0;
    int cnt = 0;
    for (int fy = row_lo + tid; fy <= row_hi; fy += kFrcThreads) {
        int iv[4];
        frc_ring_row(k, fy, s, iv[0], iv[1], iv[2], iv[3]);
        const size_t row = (size_t)(fy < 0 ? fy + s : fy) * s;
        double py = 0.0;
        if (ramp) {
            py = (double)fy * dy / s;
            py -= rint(py);
        }
        for (int h = 0; h < 2; ++h) {
            for (int fx = iv[2 * h]; fx <= iv[2 * h + 1]; ++fx) {
                const size_t idx = row + (size_t)(fx < 0 ? fx + s : fx);
                const c32 av = A[idx], bv = B[idx];
                const double ar = av.x, ai = av.y;
                double br = bv.x, bi = bv.y;
                pb += br * br + bi * bi;
                if (ramp) {
                    double px = (double)fx * dx / s;
                    px -= rint(px);
                    double ph = py + px;
                    ph -= rint(ph);
                    double sn, cs;
                    sincospi(2.0 * ph, &sn, &cs);
                    const double r = br * cs + bi * sn;   // B exp(-2 pi i ph)
                    bi = bi * cs - br * sn;
                    br = r;
                }
                cr += ar * br + ai * bi;   // A conj(B)
                ci += ai * br - ar * bi;
                pa += ar * ar + ai * ai;
                ++cnt;
            }
        }
    }
    double v[5] = {cr, ci, pa, pb, (double)cnt};
#pragma unroll
    for (int e = 0; e < 5; ++e) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) v[e] += __shfl_xor(v[e], o);
    }
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 5; ++e) part[wave * 5 + e] = v[e];
    }
    __syncthreads();
    if (tid < 5) {
        const int K = frc_rings(s);
        sums[((size_t)ang * K + k) * 5 + tid] = ((part[tid] + part[5 + tid]) + part[10 + tid]) + part[15 + tid];
    }
}

#endif  // __HIPCC__

}  // namespace pty
