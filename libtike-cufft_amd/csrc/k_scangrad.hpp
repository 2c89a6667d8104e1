// k_scangrad.hpp -- the derivative of the forward model with respect to the scan positions (ptycho_adj_scan,
// PtychoHIP.adj_scan): for every position the two sums
//     out[p][0] = c Re sum_ij conj(w_ij) prb_ij dPy_ij        dPy = (f10 - f00)(1 - fx) + (f11 - f01) fx
//     out[p][1] = c Re sum_ij conj(w_ij) prb_ij dPx_ij        dPx = (f01 - f00)(1 - fy) + (f11 - f10) fy
// over the nprb x nprb probe pixels, w the centre crop of the position's inverse-transformed detector tile (the launcher
// runs ptycho_fft2 first), f?? the four bilinear taps of the forward operator (taps outside the object read 0), c = 1/ndet.
// include/ptycho_hip.h and DESIGN.md section 19 state the definition.
//
//   k_scangrad   one workgroup of 256 threads per position of the chunk.  The probe is cut into column blocks of cw = 16,
//                32 or 64 columns and bands of at most 32 rows (sg_map); a thread owns one column of a block (consecutive
//                lanes read consecutive elements of a row of w and of the probe) and walks down the band, carrying the
//                lower pair of taps of pixel i into pixel i + 1: two object loads per pixel and two more per band.  The
//                differences, the weights and the product with the probe are float32, as the forward operator forms its
//                patch; the terms Re conj(w) q are added in float64 per thread, then over the wave by a shuffle tree and
//                over the four waves in order (block_sum, frame_part.hpp): no atomics, the same inputs give the same bits.
//                A skipped position (integer part < 0, or not finite) writes +0.0 twice.
//
// The index logic (sg_map, sg_item, sg_tap) is plain C++: tests/test_scan_grad_cpu.py builds host_scangrad.cpp with the
// host compiler and walks it as the kernel does (sg_walk).
#pragma once

#include <cstddef>

#include "fft_core.hpp"
#include "frame_part.hpp"
#include "k_gauge.hpp"

namespace pty {

constexpr int kSgThreads = 256;    // threads of a workgroup
constexpr int kSgBandRows = 32;    // most rows of a band

// the cut of an nprb x nprb probe into items (column block, band) and of the workgroup into slots of cw threads
struct SgMap {
    int cw;          // columns of a block = threads of a slot: 16, 32 or 64
    int ncb;         // column blocks
    int slots;       // kSgThreads / cw: items in flight
    int band_rows;   // rows of a band (the last band may be shorter)
    int nband;       // bands
    int items;       // ncb * nband; item it = band (it / ncb) of column block (it % ncb)
};

PTY_HD SgMap sg_map(const int nprb) {
    SgMap m;
    m.cw = nprb <= 16 ? 16 : (nprb <= 32 ? 32 : 64);
    m.ncb = (nprb + m.cw - 1) / m.cw;
    m.slots = kSgThreads / m.cw;
    int nband = (m.slots + m.ncb - 1) / m.ncb;                  // enough items for every slot ...
    const int deep = (nprb + kSgBandRows - 1) / kSgBandRows;   // ... and no band deeper than kSgBandRows
    if (nband < deep) nband = deep;
    if (nband > nprb) nband = nprb;
    m.band_rows = (nprb + nband - 1) / nband;
    m.nband = (nprb + m.band_rows - 1) / m.band_rows;
    m.items = m.ncb * m.nband;
    return m;
}

// what thread tid does in item it: column j of the probe, rows [i0, i1); live = false: the column lies past the probe
struct SgItem {
    int j, i0, i1;
    bool live;
};

PTY_HD SgItem sg_item(const SgMap& m, const int nprb, const int it, const int tid) {
    SgItem q;
    q.j = (it % m.ncb) * m.cw + tid % m.cw;
    q.i0 = (it / m.ncb) * m.band_rows;
    q.i1 = q.i0 + m.band_rows < nprb ? q.i0 + m.band_rows : nprb;
    q.live = q.j < nprb;
    return q;
}

// object element of tap (a, b) of probe pixel (i, j) for the whole-pixel position (sy, sx), sy >= 0 and sx >= 0:
// psi[sy + i + a][sx + j + b]; false: outside the object, the tap reads 0 (at = 0 then)
PTY_HD bool sg_tap(const int sy, const int sx, const int i, const int j, const int a, const int b, const int nz, const int n,
                   size_t& at) {
    const long long Y = (long long)sy + i + a, X = (long long)sx + j + b;
    const bool ok = Y < nz && X < n;
    at = ok ? (size_t)Y * (size_t)n + (size_t)X : 0;
    return ok;
}

// one tap as the walk holds it
struct SgTapAt {
    size_t at;
    bool ok;
};
PTY_HD SgTapAt sg_tap_at(const int sy, const int sx, const int i, const int j, const int a, const int b, const int nz, const int n) {
    SgTapAt t;
    t.ok = sg_tap(sy, sx, i, j, a, b, nz, n, t.at);
    return t;
}

// The walk of one workgroup, thread by thread, with the taps in place of their values: hook(i, j, t00, t01, t10, t11)
// for every pixel visited.  The kernel below runs the same loops with loads (k_scangrad); this is what the host walks.
template <class Hook>
PTY_HD void sg_walk(const int nprb, const int sy, const int sx, const int nz, const int n, Hook&& hook) {
    const SgMap m = sg_map(nprb);
    for (int tid = 0; tid < kSgThreads; ++tid)
        for (int it = tid / m.cw; it < m.items; it += m.slots) {
            const SgItem q = sg_item(m, nprb, it, tid);
            if (!q.live) continue;
            SgTapAt u0 = sg_tap_at(sy, sx, q.i0, q.j, 0, 0, nz, n), u1 = sg_tap_at(sy, sx, q.i0, q.j, 0, 1, nz, n);
            for (int i = q.i0; i < q.i1; ++i) {
                const SgTapAt l0 = sg_tap_at(sy, sx, i, q.j, 1, 0, nz, n), l1 = sg_tap_at(sy, sx, i, q.j, 1, 1, nz, n);
                hook(i, q.j, u0, u1, l0, l1);
                u0 = l0;
                u1 = l1;
            }
        }
}

#if defined(__HIPCC__)

struct SgArgs {
    float* out;          // [ptheta * nscan][2]
    const c32* w;        // the chunk's tiles after the inverse transform: [count][ndet][ndet]
    const c32* f;        // object [ptheta][nz][n]
    const float* scan;   // [ptheta * nscan][2]
    const c32* prb;      // [ptheta][nprb][nprb]
    long long p0;        // first position of the chunk
    int nscan, nz, n, ndet, nprb, pad;
};

__device__ __forceinline__ c32 sg_load(const c32* __restrict__ ft, const int sy, const int sx, const int i, const int j,
                                       const int a, const int b, const int nz, const int n) {
    size_t at;
    const bool ok = sg_tap(sy, sx, i, j, a, b, nz, n, at);
    const c32 v = ft[at];   // element 0 of the angle's object when the tap is outside: a valid address
    return ok ? v : c32{0.0f, 0.0f};
}

// grid: the positions of the chunk, 256 threads
__global__ __launch_bounds__(kSgThreads) void k_scangrad(const SgArgs a) {
    __shared__ double part[4 * 2 + 2];
    const int tid = threadIdx.x;
    const long long p = a.p0 + blockIdx.x;
    const int t = (int)(p / a.nscan);
    int sy, sx;
    float fy, fx;
    const bool vy = illum_split(a.scan[2 * (size_t)p], sy, fy), vx = illum_split(a.scan[2 * (size_t)p + 1], sx, fx);
    double v[2] = {0.0, 0.0};
    if (vy && vx) {   // the same in every thread
        const SgMap m = sg_map(a.nprb);
        const c32* __restrict__ ft = a.f + (size_t)t * a.nz * a.n;
        const c32* __restrict__ prb = a.prb + (size_t)t * a.nprb * a.nprb;
        const c32* __restrict__ w = a.w + ((size_t)blockIdx.x * a.ndet + a.pad) * a.ndet + a.pad;
        const float gy = 1.0f - fy, gx = 1.0f - fx;
        for (int it = tid / m.cw; it < m.items; it += m.slots) {
            const SgItem q = sg_item(m, a.nprb, it, tid);
            if (!q.live) continue;
            c32 u0 = sg_load(ft, sy, sx, q.i0, q.j, 0, 0, a.nz, a.n), u1 = sg_load(ft, sy, sx, q.i0, q.j, 0, 1, a.nz, a.n);
#pragma unroll 4
            for (int i = q.i0; i < q.i1; ++i) {
                const c32 l0 = sg_load(ft, sy, sx, i, q.j, 1, 0, a.nz, a.n), l1 = sg_load(ft, sy, sx, i, q.j, 1, 1, a.nz, a.n);
                const c32 wv = w[(size_t)i * a.ndet + q.j], pv = prb[(size_t)i * a.nprb + q.j];
                const c32 qy = cmul(pv, (l0 - u0) * gx + (l1 - u1) * fx);
                const c32 qx = cmul(pv, (u1 - u0) * gy + (l1 - l0) * fy);
                v[0] += (double)wv.x * (double)qy.x + (double)wv.y * (double)qy.y;   // Re conj(w) q
                v[1] += (double)wv.x * (double)qx.x + (double)wv.y * (double)qx.y;
                u0 = l0;
                u1 = l1;
            }
        }
    }
    double* tot = part + 4 * 2;
    block_sum<2>(v, tot, part);
    if (tid < 2) a.out[2 * (size_t)p + tid] = (float)(tot[tid] * (double)(1.0f / (float)a.ndet));   // written by this thread
}

#endif  // __HIPCC__

}  // namespace pty
