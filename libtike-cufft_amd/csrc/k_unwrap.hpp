// k_unwrap.hpp -- weighted least-squares phase unwrapping (ptycho_unwrap_*, libtike.hipfft.unwrap): Jacobi-preconditioned
// conjugate gradients on the pixel grid (Ghiglia & Romero 1994).  No handle, no float atomics, every sum in float64 in a
// fixed order: the same inputs give the same bits.  include/ptycho_hip.h and DESIGN.md section 15 state the mathematics.
//
// Per angle the float32 scratch `buf` holds six planes [nz][n]: x, r, p (two copies), q, 1 / D; `state` holds
// kUnwStateWords float64 (rz0, rz, pq, alpha, beta, iterations, status, relres, c); `work` holds two float64 per tile.
//
//   k_unwrap_setup    one 256-thread workgroup per 64 x 16 tile, a thread owns four pixels of one row.  phi and the
//                     effective weight w' of the tile and of its one-pixel halo (no corners) go through LDS; per pixel
//                     b -> r, D -> 1 / D, x = 0, p = r / D, and the tile's part of rz0 = r . z.  Where the difference
//                     d_e of an edge comes from is a template parameter: the wrapped difference of a phase
//                     (UnwPhaseSrc, the unwrapper) or the mean of a gradient field at the edge's two ends (UnwGradSrc,
//                     ptycho_integrate_begin of k_dpc.hpp); everything else is shared.
//   k_unwrap_apply    the same tile.  The direction of this iteration, p = z + beta p_old (beta = 0 in the first), is
//                     formed on the load for the tile AND its halo from r, 1 / D and the previous direction -- the same
//                     expression on the same operands wherever a pixel is formed, so the same bits --, written for the
//                     tile to the OTHER copy of p (no workgroup reads a neighbour's half-updated p), and q = L p with the
//                     edge weights min(w', w') recomputed from w' in LDS; the tile's part of p . q.
//   k_unwrap_update   flat, four consecutive pixels per thread: x += alpha p, r -= alpha q, part of rz' = r . (r / D).
//   k_unwrap_scalars  one workgroup per angle, in the manner of k_gauge_finish: adds the parts in index order and keeps
//                     the state: stage 0 after setup, 1 after apply (stopping tests, alpha), 2 after update (beta, the
//                     iteration count, the stopping tests), 3 after k_unwrap_offset (c), 4 the stopping tests alone.
//   k_unwrap_offset   flat: parts of sum w' [D > 0] exp(i (phi - x)) in float64.
//   k_unwrap_finish   flat: out = phi + 2 pi rint((x + c - phi) / 2 pi) or x + c, phi where D = 0.
//   k_unwrap_residues one thread per 2 x 2 loop: the charge and, with an integer atomic, the count per angle.
//
// apply, update and stages 1, 2 return at once for an angle whose status is not 0: the host enqueues iterations blindly.
//
// The tile / halo index logic is plain C++: tests/test_unwrap_cpu.py builds host_unwrap.cpp with the host compiler and
// checks that every pixel is owned once, every edge is visited once from each end and nothing outside the image is touched.
#pragma once

#include <cmath>

#include "frame_part.hpp"

namespace pty {

constexpr int kUnwTileW = 64, kUnwTileH = 16;   // pixels per workgroup: 256 threads x kUnwVec
constexpr int kUnwVec = 4;                      // consecutive pixels of one row per thread: one 16-byte access
constexpr int kUnwLdsW = kUnwTileW + 2, kUnwLdsH = kUnwTileH + 2;
constexpr int kUnwHalo = 2 * kUnwTileW + 2 * kUnwTileH;   // halo pixels of a tile (no corners: a 5-point stencil)
constexpr int kUnwPlanes = 6;                   // x, r, p, p', q, 1 / D
constexpr int kUnwPart = 2;                     // float64 words of `work` per tile (the offset sum has two)
constexpr int kUnwStateWords = 16;              // include/ptycho_hip.h: PTYCHO_UNWRAP_STATE_WORDS
constexpr unsigned long long kUnwMaxAngles = 65535;        // gridDim.y
constexpr unsigned long long kUnwMaxPixels = 1ull << 31;   // nz * n below this: pixel indices stay in int
enum { UNW_RZ0 = 0, UNW_RZ, UNW_PQ, UNW_ALPHA, UNW_BETA, UNW_ITER, UNW_STATUS, UNW_RELRES, UNW_C };
enum { UNW_RUNNING = 0, UNW_CONVERGED = 1, UNW_BREAKDOWN = 2, UNW_MAXITER = 3 };

PTY_HD int unwrap_tiles_x(const int n) { return (n + kUnwTileW - 1) / kUnwTileW; }
PTY_HD int unwrap_tiles_y(const int nz) { return (nz + kUnwTileH - 1) / kUnwTileH; }
PTY_HD long long unwrap_tiles(const int nz, const int n) { return (long long)unwrap_tiles_x(n) * unwrap_tiles_y(nz); }
PTY_HD bool unwrap_inside(const int y, const int x, const int nz, const int n) { return y >= 0 && y < nz && x >= 0 && x < n; }

// thread tid of tile (by, bx) owns the pixels (y, x .. x + kUnwVec - 1)
PTY_HD void unwrap_own(const int tid, const int by, const int bx, int& y, int& x) {
    y = by * kUnwTileH + tid / (kUnwTileW / kUnwVec);
    x = bx * kUnwTileW + kUnwVec * (tid % (kUnwTileW / kUnwVec));
}
// the halo pixel that thread tid stages: the row above, the row below, the column to the left, the column to the right;
// false for tid >= kUnwHalo
PTY_HD bool unwrap_halo(const int tid, const int by, const int bx, int& y, int& x) {
    const int y0 = by * kUnwTileH, x0 = bx * kUnwTileW;
    if (tid < kUnwTileW) { y = y0 - 1; x = x0 + tid; return true; }
    if (tid < 2 * kUnwTileW) { y = y0 + kUnwTileH; x = x0 + tid - kUnwTileW; return true; }
    if (tid < 2 * kUnwTileW + kUnwTileH) { y = y0 + tid - 2 * kUnwTileW; x = x0 - 1; return true; }
    if (tid < kUnwHalo) { y = y0 + tid - 2 * kUnwTileW - kUnwTileH; x = x0 + kUnwTileW; return true; }
    y = 0; x = 0;
    return false;
}
// LDS slot of pixel (y, x) of the tile (by, bx) or of its halo
PTY_HD int unwrap_slot(const int y, const int x, const int by, const int bx) {
    return (y - by * kUnwTileH + 1) * kUnwLdsW + (x - bx * kUnwTileW + 1);
}
// the plane of a gradient field (0: gy, along the row index; 1: gx, along the column index) that gives the difference of
// an edge: gy for an edge between a pixel and the one below it (vertical), gx for one to the right
PTY_HD int unwrap_grad_field(const bool vertical) { return vertical ? 0 : 1; }

#if defined(__HIPCC__)

constexpr float kUnwTwoPiF = 6.28318530717958647692f;
constexpr double kUnwTwoPi = 6.28318530717958647692;

// W(a) = a - 2 pi rint(a / 2 pi), every operation rounded to float32 (no contraction)
__device__ __forceinline__ float unwrap_W(const float a) {
    return __fsub_rn(a, __fmul_rn(kUnwTwoPiF, rintf(__fdiv_rn(a, kUnwTwoPiF))));
}
// the effective weight: a select, never a product
__device__ __forceinline__ float unwrap_weight(const float* __restrict__ weight, const size_t idx) {
    if (!weight) return 1.0f;
    const float w = weight[idx];
    return (w > 0.0f && w < INFINITY) ? w : 0.0f;
}
__device__ __forceinline__ float unwrap_wsel(const float w) { return (w > 0.0f && w < INFINITY) ? w : 0.0f; }
// the direction of an iteration from the residual, 1 / D and the direction before
__device__ __forceinline__ float unwrap_dir(const float r, const float minv, const float pold, const float beta) {
    return fmaf(beta, pold, __fmul_rn(minv, r));
}

struct UnwTile {
    int by, bx, y, x;    // the tile and the thread's first pixel
    bool row;            // the thread's row is inside the image
};
__device__ __forceinline__ UnwTile unwrap_tile(const int ntx, const int nz) {
    UnwTile u;
    u.by = (int)(blockIdx.x / (unsigned)ntx);
    u.bx = (int)(blockIdx.x % (unsigned)ntx);
    unwrap_own((int)threadIdx.x, u.by, u.bx, u.y, u.x);
    u.row = u.y < nz;
    return u;
}

// four consecutive floats at idx: one 16-byte access (VEC: idx % 4 == 0 and the base is 16-byte aligned) or four scalar
// ones of which only the first `have` are inside the row / plane
template <bool VEC>
__device__ __forceinline__ void unwrap_load4(float (&v)[kUnwVec], const float* __restrict__ src, const size_t idx, const int have) {
    if constexpr (VEC) {
        const float4 f = *reinterpret_cast<const float4*>(src + idx);
        v[0] = f.x; v[1] = f.y; v[2] = f.z; v[3] = f.w;
    } else {
#pragma unroll
        for (int k = 0; k < kUnwVec; ++k) v[k] = k < have ? src[idx + k] : 0.0f;
    }
}
template <bool VEC>
__device__ __forceinline__ void unwrap_store4(float* __restrict__ dst, const size_t idx, const float (&v)[kUnwVec], const int have) {
    if constexpr (VEC) {
        *reinterpret_cast<float4*>(dst + idx) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int k = 0; k < kUnwVec; ++k)
            if (k < have) dst[idx + k] = v[k];
    }
}

// Where k_unwrap_setup takes the difference d_e of an edge from: kFields planes [ptheta][nz][n] that go through LDS with
// the tile, and diff(l, a, b, vertical), the difference of the edge from slot a to slot b -- b to the right of a, or
// below it (vertical) --, every operation rounded to float32.
//   UnwPhaseSrc  the wrapped difference of a phase, W(phi_b - phi_a): ptycho_unwrap_begin
//   UnwGradSrc   the mean of a gradient field at the two ends, (g_a + g_b) / 2 of gx along a row and of gy along a column:
//                ptycho_integrate_begin
struct UnwPhaseSrc {
    static constexpr int kFields = 1;
    __device__ __forceinline__ static float diff(const float (&l)[kFields][kUnwLdsH * kUnwLdsW], const int a, const int b,
                                                 const bool /*vertical*/) {
        return unwrap_W(__fsub_rn(l[0][b], l[0][a]));
    }
};
struct UnwGradSrc {
    static constexpr int kFields = 2;   // gy, gx
    __device__ __forceinline__ static float diff(const float (&l)[kFields][kUnwLdsH * kUnwLdsW], const int a, const int b,
                                                 const bool vertical) {
#pragma clang fp contract(off)
        const int e = unwrap_grad_field(vertical);
        return 0.5f * (l[e][a] + l[e][b]);
    }
};

// grid (tiles, ptheta), 256 threads; f0, f1: the planes of Src (f1 is read only when Src has two)
template <bool VEC, class Src = UnwPhaseSrc>
__global__ __launch_bounds__(256) void k_unwrap_setup(float* __restrict__ buf, const float* __restrict__ f0,
                                                      const float* __restrict__ weight, const int nz, const int n,
                                                      const int ntx, double* __restrict__ work,
                                                      const float* __restrict__ f1) {
    __shared__ float l_f[Src::kFields][kUnwLdsH * kUnwLdsW], l_w[kUnwLdsH * kUnwLdsW];
    __shared__ double part[4];
    const int tid = threadIdx.x, t = blockIdx.y;
    const UnwTile u = unwrap_tile(ntx, nz);
    const size_t plane = (size_t)nz * (size_t)n;
    const float* wt = weight ? weight + (size_t)t * plane : nullptr;
    float* base = buf + (size_t)t * kUnwPlanes * plane;
    const int have = !u.row ? 0 : (n - u.x >= kUnwVec ? kUnwVec : (n - u.x > 0 ? n - u.x : 0));
    const size_t idx = (size_t)u.y * (size_t)n + (size_t)u.x;
    {
        float f[Src::kFields][kUnwVec], w[kUnwVec] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int e = 0; e < Src::kFields; ++e)
#pragma unroll
            for (int k = 0; k < kUnwVec; ++k) f[e][k] = 0.0f;
        if (have > 0) {
#pragma unroll
            for (int e = 0; e < Src::kFields; ++e) unwrap_load4<VEC>(f[e], (e == 0 ? f0 : f1) + (size_t)t * plane, idx, have);
            if (wt) unwrap_load4<VEC>(w, wt, idx, have);
        }
        const int s = unwrap_slot(u.y, u.x, u.by, u.bx);
#pragma unroll
        for (int k = 0; k < kUnwVec; ++k) {
#pragma unroll
            for (int e = 0; e < Src::kFields; ++e) l_f[e][s + k] = f[e][k];
            l_w[s + k] = k < have ? (wt ? unwrap_wsel(w[k]) : 1.0f) : 0.0f;
        }
        int hy, hx;
        if (unwrap_halo(tid, u.by, u.bx, hy, hx)) {
            const bool in = unwrap_inside(hy, hx, nz, n);
            const size_t hi = (size_t)(in ? hy : 0) * (size_t)n + (size_t)(in ? hx : 0);
            const int hs = unwrap_slot(hy, hx, u.by, u.bx);
#pragma unroll
            for (int e = 0; e < Src::kFields; ++e) l_f[e][hs] = in ? (e == 0 ? f0 : f1)[(size_t)t * plane + hi] : 0.0f;
            l_w[hs] = in ? unwrap_weight(wt, hi) : 0.0f;
        }
    }
    __syncthreads();
    double v[1] = {0.0};
    if (have > 0) {
        float r[kUnwVec], mi[kUnwVec], zero[kUnwVec], z[kUnwVec];
        const int s = unwrap_slot(u.y, u.x, u.by, u.bx);
#pragma unroll
        for (int k = 0; k < kUnwVec; ++k) {
            const int c = s + k;
            const float wc = l_w[c];
            // edges in the order left, right, up, down; an edge of weight 0 contributes exactly 0 (a select)
            const float wl = fminf(wc, l_w[c - 1]), wr = fminf(wc, l_w[c + 1]);
            const float wu = fminf(wc, l_w[c - kUnwLdsW]), wd = fminf(wc, l_w[c + kUnwLdsW]);
            float b = 0.0f, D = 0.0f;
            if (wl > 0.0f) { b = __fadd_rn(b, __fmul_rn(wl, Src::diff(l_f, c - 1, c, false))); D = __fadd_rn(D, wl); }
            if (wr > 0.0f) { b = __fsub_rn(b, __fmul_rn(wr, Src::diff(l_f, c, c + 1, false))); D = __fadd_rn(D, wr); }
            if (wu > 0.0f) { b = __fadd_rn(b, __fmul_rn(wu, Src::diff(l_f, c - kUnwLdsW, c, true))); D = __fadd_rn(D, wu); }
            if (wd > 0.0f) { b = __fsub_rn(b, __fmul_rn(wd, Src::diff(l_f, c, c + kUnwLdsW, true))); D = __fadd_rn(D, wd); }
            r[k] = b;
            mi[k] = D > 0.0f ? __fdiv_rn(1.0f, D) : 0.0f;
            z[k] = __fmul_rn(mi[k], b);
            zero[k] = 0.0f;
            if (k < have) v[0] += (double)b * (double)z[k];
        }
        unwrap_store4<VEC>(base, idx, zero, have);                  // x
        unwrap_store4<VEC>(base + plane, idx, r, have);             // r
        unwrap_store4<VEC>(base + 2 * plane, idx, z, have);         // p
        unwrap_store4<VEC>(base + 5 * plane, idx, mi, have);        // 1 / D
    }
    block_sum<1>(v, work + ((size_t)t * gridDim.x + blockIdx.x) * kUnwPart, part);
}

// grid (tiles, ptheta), 256 threads
template <bool VEC>
__global__ __launch_bounds__(256) void k_unwrap_apply(float* __restrict__ buf, const double* __restrict__ state,
                                                      const float* __restrict__ weight, const int nz, const int n,
                                                      const int ntx, const int maxiter, double* __restrict__ work) {
    __shared__ float l_p[kUnwLdsH * kUnwLdsW], l_w[kUnwLdsH * kUnwLdsW];
    __shared__ double part[4];
    const int tid = threadIdx.x, t = blockIdx.y;
    const double* st = state + (size_t)t * kUnwStateWords;
    if (st[UNW_STATUS] != 0.0 || st[UNW_ITER] >= (double)maxiter) return;   // the angle has stopped (or is about to)
    const int it = (int)st[UNW_ITER];
    const float beta = (float)st[UNW_BETA];
    const UnwTile u = unwrap_tile(ntx, nz);
    const size_t plane = (size_t)nz * (size_t)n;
    const float* wt = weight ? weight + (size_t)t * plane : nullptr;
    float* base = buf + (size_t)t * kUnwPlanes * plane;
    const float* r_ = base + plane;
    const float* pold = base + (size_t)(2 + (it & 1)) * plane;
    float* pnew = base + (size_t)(3 - (it & 1)) * plane;
    float* q_ = base + 4 * plane;
    const float* mi_ = base + 5 * plane;
    const int have = !u.row ? 0 : (n - u.x >= kUnwVec ? kUnwVec : (n - u.x > 0 ? n - u.x : 0));
    const size_t idx = (size_t)u.y * (size_t)n + (size_t)u.x;
    const int s = unwrap_slot(u.y, u.x, u.by, u.bx);
    float p[kUnwVec] = {0.0f, 0.0f, 0.0f, 0.0f};
    {
        float r[kUnwVec], mi[kUnwVec], po[kUnwVec], w[kUnwVec] = {0.0f, 0.0f, 0.0f, 0.0f};
        if (have > 0) {
            unwrap_load4<VEC>(r, r_, idx, have);
            unwrap_load4<VEC>(mi, mi_, idx, have);
            unwrap_load4<VEC>(po, pold, idx, have);
            if (wt) unwrap_load4<VEC>(w, wt, idx, have);
#pragma unroll
            for (int k = 0; k < kUnwVec; ++k) p[k] = unwrap_dir(r[k], mi[k], po[k], beta);
        }
#pragma unroll
        for (int k = 0; k < kUnwVec; ++k) {
            l_p[s + k] = k < have ? p[k] : 0.0f;
            l_w[s + k] = k < have ? (wt ? unwrap_wsel(w[k]) : 1.0f) : 0.0f;
        }
        int hy, hx;
        if (unwrap_halo(tid, u.by, u.bx, hy, hx)) {
            const bool in = unwrap_inside(hy, hx, nz, n);
            const size_t hi = (size_t)(in ? hy : 0) * (size_t)n + (size_t)(in ? hx : 0);
            const int hs = unwrap_slot(hy, hx, u.by, u.bx);
            l_p[hs] = in ? unwrap_dir(r_[hi], mi_[hi], pold[hi], beta) : 0.0f;
            l_w[hs] = in ? unwrap_weight(wt, hi) : 0.0f;
        }
    }
    __syncthreads();
    double v[1] = {0.0};
    if (have > 0) {
        float q[kUnwVec];
#pragma unroll
        for (int k = 0; k < kUnwVec; ++k) {
            const float pc = l_p[s + k], wc = l_w[s + k];
            const float wl = fminf(wc, l_w[s + k - 1]), wr = fminf(wc, l_w[s + k + 1]);
            const float wu = fminf(wc, l_w[s + k - kUnwLdsW]), wd = fminf(wc, l_w[s + k + kUnwLdsW]);
            float a = 0.0f;
            if (wl > 0.0f) a = __fadd_rn(a, __fmul_rn(wl, __fsub_rn(pc, l_p[s + k - 1])));
            if (wr > 0.0f) a = __fadd_rn(a, __fmul_rn(wr, __fsub_rn(pc, l_p[s + k + 1])));
            if (wu > 0.0f) a = __fadd_rn(a, __fmul_rn(wu, __fsub_rn(pc, l_p[s + k - kUnwLdsW])));
            if (wd > 0.0f) a = __fadd_rn(a, __fmul_rn(wd, __fsub_rn(pc, l_p[s + k + kUnwLdsW])));
            q[k] = a;
            if (k < have) v[0] += (double)pc * (double)a;
        }
        unwrap_store4<VEC>(pnew, idx, p, have);
        unwrap_store4<VEC>(q_, idx, q, have);
    }
    block_sum<1>(v, work + ((size_t)t * gridDim.x + blockIdx.x) * kUnwPart, part);
}

// the thread's four consecutive pixels of the flat kernels: first index and how many are inside the plane
__device__ __forceinline__ int unwrap_flat(const size_t plane, size_t& idx) {
    idx = ((size_t)blockIdx.x * 256 + threadIdx.x) * kUnwVec;
    return idx >= plane ? 0 : (plane - idx >= (size_t)kUnwVec ? kUnwVec : (int)(plane - idx));
}

// grid (ceil(nz n / 1024), ptheta), 256 threads; tiles: rows of `work` per angle
template <bool VEC>
__global__ __launch_bounds__(256) void k_unwrap_update(float* __restrict__ buf, const double* __restrict__ state,
                                                       const size_t plane, const long long tiles, double* __restrict__ work) {
    __shared__ double part[4];
    const int t = blockIdx.y;
    const double* st = state + (size_t)t * kUnwStateWords;
    if (st[UNW_STATUS] != 0.0) return;
    const int it = (int)st[UNW_ITER];
    const float alpha = (float)st[UNW_ALPHA];
    float* base = buf + (size_t)t * kUnwPlanes * plane;
    size_t idx;
    const int have = unwrap_flat(plane, idx);
    double v[1] = {0.0};
    if (have > 0) {
        float x[kUnwVec], r[kUnwVec], p[kUnwVec], q[kUnwVec], mi[kUnwVec];
        unwrap_load4<VEC>(x, base, idx, have);
        unwrap_load4<VEC>(r, base + plane, idx, have);
        unwrap_load4<VEC>(p, base + (size_t)(3 - (it & 1)) * plane, idx, have);   // the copy k_unwrap_apply wrote
        unwrap_load4<VEC>(q, base + 4 * plane, idx, have);
        unwrap_load4<VEC>(mi, base + 5 * plane, idx, have);
#pragma unroll
        for (int k = 0; k < kUnwVec; ++k) {
            x[k] = fmaf(alpha, p[k], x[k]);
            r[k] = fmaf(-alpha, q[k], r[k]);
            if (k < have) v[0] += (double)r[k] * (double)__fmul_rn(mi[k], r[k]);
        }
        unwrap_store4<VEC>(base, idx, x, have);
        unwrap_store4<VEC>(base + plane, idx, r, have);
    }
    block_sum<1>(v, work + ((size_t)t * (size_t)tiles + blockIdx.x) * kUnwPart, part);
}

// grid (ceil(nz n / 1024), ptheta), 256 threads: parts of sum w' [D > 0] exp(i (phi - x))
template <bool VEC>
__global__ __launch_bounds__(256) void k_unwrap_offset(const float* __restrict__ buf, const float* __restrict__ phase,
                                                       const float* __restrict__ weight, const size_t plane,
                                                       const long long tiles, double* __restrict__ work) {
    __shared__ double part[4 * 2];
    const int t = blockIdx.y;
    const float* base = buf + (size_t)t * kUnwPlanes * plane;
    size_t idx;
    const int have = unwrap_flat(plane, idx);
    double v[2] = {0.0, 0.0};
    if (have > 0) {
        float x[kUnwVec], f[kUnwVec], mi[kUnwVec], w[kUnwVec] = {1.0f, 1.0f, 1.0f, 1.0f};
        unwrap_load4<VEC>(x, base, idx, have);
        unwrap_load4<VEC>(mi, base + 5 * plane, idx, have);
        unwrap_load4<VEC>(f, phase + (size_t)t * plane, idx, have);
        if (weight) unwrap_load4<VEC>(w, weight + (size_t)t * plane, idx, have);
#pragma unroll
        for (int k = 0; k < kUnwVec; ++k) {
            const float wk = unwrap_wsel(w[k]);
            if (k < have && wk > 0.0f && mi[k] > 0.0f) {
                double sn, cs;
                sincos((double)f[k] - (double)x[k], &sn, &cs);
                v[0] += (double)wk * cs;
                v[1] += (double)wk * sn;
            }
        }
    }
    block_sum<2>(v, work + ((size_t)t * (size_t)tiles + blockIdx.x) * kUnwPart, part);
}

// grid (ceil(nz n / 1024), ptheta), 256 threads
template <bool VEC>
__global__ __launch_bounds__(256) void k_unwrap_finish(float* __restrict__ out, const double* __restrict__ state,
                                                       const float* __restrict__ buf, const float* __restrict__ phase,
                                                       const size_t plane, const int congruent) {
    const int t = blockIdx.y;
    const double c = state[(size_t)t * kUnwStateWords + UNW_C];
    const float* base = buf + (size_t)t * kUnwPlanes * plane;
    size_t idx;
    const int have = unwrap_flat(plane, idx);
    if (have == 0) return;
    float x[kUnwVec], f[kUnwVec], mi[kUnwVec], o[kUnwVec];
    unwrap_load4<VEC>(x, base, idx, have);
    unwrap_load4<VEC>(mi, base + 5 * plane, idx, have);
    unwrap_load4<VEC>(f, phase + (size_t)t * plane, idx, have);
#pragma unroll
    for (int k = 0; k < kUnwVec; ++k) {
        const double xc = (double)x[k] + c, fd = (double)f[k];
        const double v = congruent ? fd + kUnwTwoPi * rint((xc - fd) / kUnwTwoPi) : xc;
        o[k] = mi[k] > 0.0f ? (float)v : f[k];     // no weighted edge: the pixel stays
    }
    unwrap_store4<VEC>(out + (size_t)t * plane, idx, o, have);
}

// grid (ptheta), 256 threads; rows: parts per angle that the stage's producer wrote, tiles: rows of `work` per angle
__global__ __launch_bounds__(256) void k_unwrap_scalars(double* __restrict__ state, const double* __restrict__ work,
                                                        const long long rows, const long long tiles, const int stage,
                                                        const int maxiter, const double tol) {
    __shared__ double part[4 * 2];
    __shared__ double tot[2];
    const int t = blockIdx.x, tid = threadIdx.x;
    double* st = state + (size_t)t * kUnwStateWords;
    if ((stage == 1 || stage == 2 || stage == 4) && st[UNW_STATUS] != 0.0) return;
    if (stage != 4) {
        const double* w = work + (size_t)t * (size_t)tiles * kUnwPart;
        double v[2] = {0.0, 0.0};
        for (long long b = tid; b < rows; b += 256) {
            v[0] += w[(size_t)b * kUnwPart];
            if (stage == 3) v[1] += w[(size_t)b * kUnwPart + 1];
        }
        block_sum<2>(v, tot, part);
        __syncthreads();
    }
    if (tid != 0) return;
    const double rz0 = st[UNW_RZ0], tol2 = tol * tol;
    if (stage == 0) {
        const double rz = tot[0];
        st[UNW_RZ0] = rz; st[UNW_RZ] = rz;
        for (int e = UNW_PQ; e < kUnwStateWords; ++e) st[e] = 0.0;
        st[UNW_STATUS] = rz == 0.0 ? (double)UNW_CONVERGED : (rz > 0.0 && rz < INFINITY ? (double)UNW_RUNNING : (double)UNW_BREAKDOWN);
        st[UNW_RELRES] = rz == 0.0 ? 0.0 : 1.0;
    } else if (stage == 1 || stage == 4) {
        if (st[UNW_RZ] <= tol2 * rz0) st[UNW_STATUS] = (double)UNW_CONVERGED;
        else if (st[UNW_ITER] >= (double)maxiter) st[UNW_STATUS] = (double)UNW_MAXITER;
        else if (stage == 1) {
            const double pq = tot[0];
            st[UNW_PQ] = pq;
            if (!(pq > 0.0) || !(pq < INFINITY)) st[UNW_STATUS] = (double)UNW_BREAKDOWN;   // x stays as it is
            else st[UNW_ALPHA] = st[UNW_RZ] / pq;
        }
    } else if (stage == 2) {
        const double rz = tot[0], it = st[UNW_ITER] + 1.0;
        st[UNW_BETA] = rz / st[UNW_RZ];
        st[UNW_RZ] = rz;
        st[UNW_ITER] = it;
        st[UNW_RELRES] = sqrt(rz / rz0);
        if (rz <= tol2 * rz0) st[UNW_STATUS] = (double)UNW_CONVERGED;
        else if (it >= (double)maxiter) st[UNW_STATUS] = (double)UNW_MAXITER;
    } else {
        st[UNW_C] = (tot[0] == 0.0 && tot[1] == 0.0) ? 0.0 : atan2(tot[1], tot[0]);
    }
}

// grid (ceil((nz - 1) (n - 1) / 256), ptheta), 256 threads; count zeroed by the launcher
__global__ __launch_bounds__(256) void k_unwrap_residues(signed char* __restrict__ charge, unsigned long long* __restrict__ count,
                                                         const float* __restrict__ phase, const float* __restrict__ weight,
                                                         const int nz, const int n) {
    const int t = blockIdx.y;
    const long long loops = (long long)(nz - 1) * (n - 1), i = (long long)blockIdx.x * 256 + threadIdx.x;
    const size_t plane = (size_t)nz * (size_t)n;
    int ch = 0;
    if (i < loops) {
        const int y = (int)(i / (n - 1)), x = (int)(i % (n - 1));
        const size_t a = (size_t)t * plane + (size_t)y * (size_t)n + (size_t)x;
        const bool lit = unwrap_weight(weight, a) > 0.0f && unwrap_weight(weight, a + 1) > 0.0f &&
                         unwrap_weight(weight, a + (size_t)n) > 0.0f && unwrap_weight(weight, a + (size_t)n + 1) > 0.0f;
        if (lit) {
            const float f00 = phase[a], f01 = phase[a + 1], f10 = phase[a + (size_t)n], f11 = phase[a + (size_t)n + 1];
            const float s = __fadd_rn(__fadd_rn(__fadd_rn(unwrap_W(__fsub_rn(f01, f00)), unwrap_W(__fsub_rn(f11, f01))),
                                                unwrap_W(__fsub_rn(f10, f11))), unwrap_W(__fsub_rn(f00, f10)));
            const float k = rintf(__fdiv_rn(s, kUnwTwoPiF));
            ch = k > 0.5f ? 1 : (k < -0.5f ? -1 : 0);
        }
        if (charge) charge[(size_t)t * (size_t)loops + (size_t)i] = (signed char)ch;
    }
    const unsigned long long m = __ballot(ch != 0);
    if ((threadIdx.x & 63) == 0 && m) atomicAdd(count + t, (unsigned long long)__popcll(m));   // integers: order-free
}

#endif  // __HIPCC__

}  // namespace pty
