// k_resample.hpp -- B-spline resampling of images (ptycho_spline_prefilter, ptycho_warp, ptycho_moments,
// libtike.hipfft.resample): the prefilter that turns samples into B-spline coefficients, the affine warp that evaluates
// them, and the moments behind a centre of mass.  Orders 0 ... 5, mirror extension (whole-sample symmetric, period
// 2 n - 2), the geometry of scipy.ndimage.affine_transform.  No handle, no atomics, fixed summation orders: the same inputs
// give the same bits.  include/ptycho_hip.h and DESIGN.md section 17 state the mathematics; tests/resample_ref.py restates
// it in NumPy.
//
// Prefilter.  A line of n samples is cut into segments of kRsSeg = 64.  A segment [s0, s1) is filtered over the extended
// range [a0, b1) = [max(0, s0 - halo), min(n, s1 + halo)) held in LDS and only [s0, s1) is written.  Where the range
// touches an end of the line the recursion starts exactly (causal: the sum over the mirrored line; anticausal: Unser's
// closed form); elsewhere it starts from zero state, which is off by |z|^k after k samples.  The warm-up H of a pole
// satisfies |z|^H <= 1e-9:
//     order   poles                     H          halo
//     2       -0.17157                  12         12
//     3       -0.26795                  16         16
//     4       -0.36134, -0.013725       21 + 5     28   (26 rounded up to a multiple of 4)
//     5       -0.43058, -0.043096       25 + 7     32
// Orders with two poles cascade over the SAME extended range: the second recursion reads first-pole values that are still
// wrong by |z1|^(j - a0) at sample j, and damps what it reads at j by |z2|^(s0 - j) on its way to s0; every term of that
// sum is below |z1|^(H1 + H2) since |z2| < |z1|, so the warm-ups add and nothing else is needed.  The halo is a multiple
// of four samples so that a0 keeps the 16-byte alignment of the segment start.
// A complex image [ny][nx] is a float image [ny][2 nx] whose lines along x interleave two channels; the kernels know floats
// and a channel count only.
//   k_spline_cols   one workgroup per (128 floats of a row, segment of y, image): rows a0 .. b1 into LDS with coalesced
//                   (16-byte when VEC) loads, threads across x, each walks its column in LDS, rows s0 .. s1 out.
//   k_spline_rows   one workgroup per (segment of x, 96 lines, image): the lines into an LDS tile of pitch C (R + 1) floats
//                   (R + 1 odd: the 64 lanes of a wave, each walking its own line, fall into 64 different banks), out alike.
//
// Warp.  k_warp<ORDER, CPLX>: one workgroup per 32 x 32 output tile, a thread owns four pixels of one column.  The source
// coordinate of output pixel (oy, ox) is s = M (oy, ox) + offset in float64, each product and sum rounded on its own.  The
// tile maps its four corners, takes the bounding box of every tap index it can touch (rs_axis_range, reflections included)
// and stages that box of coefficients in LDS when it holds at most kRsBoxElems elements; otherwise (strong minification)
// the taps are read from global memory.  Both paths run the same arithmetic on the same values.  A tile whose coordinates
// all lie outside the extent (constant mode) writes cval and loads nothing.
//
// Moments.  k_moments leaves per workgroup the five float64 sums of its pixels (block_sum of frame_part.hpp),
// k_moments_fold adds the workgroups of an image in index order.
//
// Everything outside the __HIPCC__ guards is plain C++: host_resample.cpp walks it on the CPU.
#pragma once

#include <cmath>
#include <type_traits>

#include "frame_part.hpp"

namespace pty {

constexpr int kRsSeg = 64;                      // L: samples of a line that one segment writes (PTYCHO_SPLINE_SEGMENT)
constexpr int kRsMaxHalo = 32;
constexpr int kRsChunk = 8;                      // samples of a line that the recursion loads at a time
constexpr int kRsColW = 128;                    // floats of a row per column-pass workgroup
constexpr int kRsRowLines = 96;                 // lines (rows x channels) per row-pass workgroup
constexpr int kRsTile = 32;                     // side of the warp's output tile
constexpr int kRsBoxElems = 4096;               // elements of the warp's LDS box (52^2 covers any rotation at unit scale)
constexpr int kRsMomBlocks = 512;               // most workgroups per image of k_moments
constexpr int kRsMomWords = 8;                  // float64 words of `work` per workgroup (five used)
constexpr unsigned long long kRsMaxImages = 65535;          // gridDim.z
constexpr unsigned long long kRsMaxSide = 65536;
constexpr unsigned long long kRsMaxPixels = 1ull << 31;     // ny * nx below this: pixel indices stay in int
constexpr double kRsClamp = 1.0 / 1048576.0;    // 2^-20 pixel: coordinates this close to the extent are clamped onto it
constexpr double kRsFar = 1073741824.0;         // 2^30: a mirror-mode coordinate beyond this counts as outside
enum { RS_MIRROR = 1, RS_GLOBAL = 2 };          // flags of ptycho_warp
enum { RS_PATH_CVAL = 0, RS_PATH_LDS = 1, RS_PATH_GLOBAL = 2 };
enum { RS_VALUE = 0, RS_POSITIVE = 1, RS_POWER = 2 };

PTY_HD int rs_halo(const int order) { return order == 2 ? 12 : order == 3 ? 16 : order == 4 ? 28 : order == 5 ? 32 : 0; }
PTY_HD int rs_npoles(const int order) { return order < 2 ? 0 : order < 4 ? 1 : 2; }
// the poles in float64 closed form; returns their number
inline int rs_poles(const int order, double z[2]) {
    z[0] = z[1] = 0.0;
    if (order == 2) z[0] = std::sqrt(8.0) - 3.0;
    if (order == 3) z[0] = std::sqrt(3.0) - 2.0;
    if (order == 4) {
        z[0] = std::sqrt(664.0 - std::sqrt(438976.0)) + std::sqrt(304.0) - 19.0;
        z[1] = std::sqrt(664.0 + std::sqrt(438976.0)) - std::sqrt(304.0) - 19.0;
    }
    if (order == 5) {
        z[0] = std::sqrt(67.5 - std::sqrt(4436.25)) + std::sqrt(26.25) - 6.5;
        z[1] = std::sqrt(67.5 + std::sqrt(4436.25)) - std::sqrt(26.25) - 6.5;
    }
    return rs_npoles(order);
}
inline double rs_gain(const int order) {
    double z[2], g = 1.0;
    const int np = rs_poles(order, z);
    for (int p = 0; p < np; ++p) g *= (1.0 - z[p]) * (1.0 - 1.0 / z[p]);
    return g;
}

struct RsSeg {
    int a0, s0, s1, b1;   // filtered range [a0, b1), written range [s0, s1)
};
PTY_HD int rs_segments(const int n) { return (n + kRsSeg - 1) / kRsSeg; }
PTY_HD RsSeg rs_segment(const int s, const int n, const int halo) {
    RsSeg g;
    g.s0 = s * kRsSeg;
    g.s1 = g.s0 + kRsSeg < n ? g.s0 + kRsSeg : n;
    g.a0 = g.s0 - halo > 0 ? g.s0 - halo : 0;
    g.b1 = g.s1 + halo < n ? g.s1 + halo : n;
    return g;
}

// the recursions of np poles over v[0], v[st], ... (len >= 2 samples, already times the gain), which are the samples
// a0 .. a0 + len of a line of n.  at_start: a0 = 0; at_end: a0 + len = n; both: the exact whole-line filter.
template <class F>
PTY_HD void rs_filter_line(F* v, const int st, const int len, const bool at_start, const bool at_end, const int n, const F* z,
                           const int np) {
    for (int p = 0; p < np; ++p) {
        const F zp = z[p];
        if (at_start) {
            F c0 = v[0], zi = zp;
            if (at_end) {   // len = n: the sum over one period of the mirrored line, closed over all periods
                F zn1 = F(1);
                for (int i = 0; i < n - 1; ++i) zn1 *= zp;
                F z2 = zn1 * zn1 / zp;
                c0 += zn1 * v[(n - 1) * st];
                for (int i = 1; i < n - 1; ++i) {
                    c0 += (zi + z2) * v[i * st];
                    zi *= zp;
                    z2 /= zp;
                }
                c0 /= F(1) - zn1 * zn1;
            } else {        // the far end is more than kRsSeg samples away: its image is below |z|^64
                for (int i = 1; i < len; ++i) {
                    c0 += zi * v[i * st];
                    zi *= zp;
                }
            }
            v[0] = c0;
        }
        // eight samples at a time: their loads are issued together and do not wait for the recursion, whose running
        // value stays in a register
        F run = v[0];
        for (int i = 1; i < len; i += kRsChunk) {
            F x[kRsChunk];
#pragma unroll
            for (int k = 0; k < kRsChunk; ++k)
                if (i + k < len) x[k] = v[(i + k) * st];
#pragma unroll
            for (int k = 0; k < kRsChunk; ++k)
                if (i + k < len) {
                    run = x[k] + zp * run;
                    v[(i + k) * st] = run;
                }
        }
        run = at_end ? (zp * v[(len - 2) * st] + run) * (zp / (zp * zp - F(1))) : -zp * run;
        v[(len - 1) * st] = run;
        for (int i = len - 2; i >= 0; i -= kRsChunk) {
            F x[kRsChunk];
#pragma unroll
            for (int k = 0; k < kRsChunk; ++k)
                if (i - k >= 0) x[k] = v[(i - k) * st];
#pragma unroll
            for (int k = 0; k < kRsChunk; ++k)
                if (i - k >= 0) {
                    run = zp * (run - x[k]);
                    v[(i - k) * st] = run;
                }
        }
    }
}

// mirror reflection of an index into [0, n), period 2 n - 2, n >= 2
PTY_HD int rs_reflect(int i, const int n) {
    if ((unsigned)i < (unsigned)n) return i;
    const int p = 2 * n - 2;
    i %= p;
    if (i < 0) i += p;
    return i < n ? i : p - i;
}

// one source coordinate: (m0 oy + m1 ox) + off, every operation rounded on its own
PTY_HD double rs_coord(const double m0, const double m1, const double off, const double oy, const double ox) {
#pragma clang fp contract(off)
    const double a = m0 * oy, b = m1 * ox;
    const double c = a + b;
    return c + off;
}

// first tap and fractional position of coordinate s: odd orders floor(s), even orders floor(s + 1/2)
PTY_HD int rs_first_tap(const double s, const int order, float& t) {
    const double f = std::floor((order & 1) ? s : s + 0.5);
    t = (float)(s - f);
    return (int)f - order / 2;
}

// [lo, hi] within [0, n): every reflected index of every tap of every coordinate in [smin, smax] (one pixel of slack on
// either side against the rounding of the corners)
PTY_HD void rs_axis_range(const double smin, const double smax, const int n, const int order, int& lo, int& hi) {
    const double l = std::floor(smin) - order / 2 - 1, h = std::floor(smax) + (order + 1) / 2 + 1;
    lo = 0;
    hi = n - 1;
    if (!(l >= -(double)(n - 1)) || !(h <= 2.0 * (n - 1)) || !(l <= h)) return;   // reflected more than once, or not finite
    int li = (int)l, hi_ = (int)h;
    if (li < 0 && -li > hi_) hi_ = -li;
    if ((int)h > n - 1 && 2 * (n - 1) - (int)h < li) li = 2 * (n - 1) - (int)h;
    lo = li > 0 ? li : 0;
    hi = hi_ < n - 1 ? hi_ : n - 1;
}

struct RsBox {
    int y0, x0, h, w;   // the box of coefficients, rows y0 .. y0 + h, columns x0 .. x0 + w
    int path;           // RS_PATH_*
};
// what the tile of output pixels [oy0, oy1] x [ox0, ox1] (inclusive) of an image with transform xf = (m00, m01, m10, m11,
// offy, offx) needs of an ny x nx image
PTY_HD RsBox rs_tile_box(const double* xf, const int oy0, const int oy1, const int ox0, const int ox1, const int ny,
                         const int nx, const int order, const int flags) {
    double ymin = 0, ymax = 0, xmin = 0, xmax = 0;
    for (int k = 0; k < 4; ++k) {
        const double oy = (k & 2) ? oy1 : oy0, ox = (k & 1) ? ox1 : ox0;
        const double sy = rs_coord(xf[0], xf[1], xf[4], oy, ox), sx = rs_coord(xf[2], xf[3], xf[5], oy, ox);
        if (k == 0 || sy < ymin) ymin = sy;
        if (k == 0 || sy > ymax) ymax = sy;
        if (k == 0 || sx < xmin) xmin = sx;
        if (k == 0 || sx > xmax) xmax = sx;
    }
    RsBox b;
    b.y0 = b.x0 = b.h = b.w = 0;
    b.path = RS_PATH_CVAL;
    if (!(flags & RS_MIRROR) && (ymax < -1e-5 || xmax < -1e-5 || ymin > ny - 1 + 1e-5 || xmin > nx - 1 + 1e-5)) return b;
    int ylo, yhi, xlo, xhi;
    rs_axis_range(ymin, ymax, ny, order, ylo, yhi);
    rs_axis_range(xmin, xmax, nx, order, xlo, xhi);
    b.y0 = ylo;
    b.x0 = xlo;
    b.h = yhi - ylo + 1;
    b.w = xhi - xlo + 1;
    const long long need = (long long)b.h * (b.w | 1);
    b.path = (flags & RS_GLOBAL) || need > kRsBoxElems ? RS_PATH_GLOBAL : RS_PATH_LDS;
    return b;
}

// whether coordinate (sy, sx) is evaluated, after the clamp of constant mode; false: the pixel is cval
PTY_HD bool rs_inside(double& sy, double& sx, const int ny, const int nx, const int flags) {
    if (flags & RS_MIRROR) return std::fabs(sy) < kRsFar && std::fabs(sx) < kRsFar;
    if (sy < 0.0 && sy >= -kRsClamp) sy = 0.0;
    if (sx < 0.0 && sx >= -kRsClamp) sx = 0.0;
    if (sy > ny - 1 && sy <= ny - 1 + kRsClamp) sy = ny - 1;
    if (sx > nx - 1 && sx <= nx - 1 + kRsClamp) sx = nx - 1;
    return sy >= 0.0 && sy <= ny - 1 && sx >= 0.0 && sx <= nx - 1;
}

// workgroups per image of k_moments
PTY_HD int rs_moment_blocks(const long long npix) {
    const long long nb = (npix + 4095) / 4096;
    return nb < 1 ? 1 : nb > kRsMomBlocks ? kRsMomBlocks : (int)nb;
}

// the ORDER + 1 centred cardinal B-spline values at distance t + ORDER / 2 - a from tap a, by the recursion
// beta_k(x) = ((k + 1) / 2 + x) beta_{k-1}(x + 1/2) / k + ((k + 1) / 2 - x) beta_{k-1}(x - 1/2) / k, unrolled
template <int ORDER>
PTY_HD void rs_weights(const float t, float (&w)[ORDER + 1]) {
    w[0] = 1.0f;
    const float dn = t + (float)(ORDER / 2);
#pragma unroll
    for (int k = 1; k <= ORDER; ++k) {
        const float dk = dn - 0.5f * (float)(ORDER - k), half = 0.5f * (float)(k + 1), inv = 1.0f / (float)k;
#pragma unroll
        for (int a = k; a >= 0; --a) {
            const float left = a >= 1 ? w[a - 1] : 0.0f, right = a <= k - 1 ? w[a] : 0.0f;
            w[a] = ((half + dk - (float)a) * left + (half - dk + (float)a) * right) * inv;
        }
    }
}

#if defined(__HIPCC__)

typedef float rs_c32 __attribute__((ext_vector_type(2)));

template <int ORDER>
struct RsCfg {
    static constexpr int kHalo = ORDER == 2 ? 12 : ORDER == 3 ? 16 : ORDER == 4 ? 28 : 32;
    static constexpr int kNp = ORDER < 4 ? 1 : 2;
    static constexpr int kR = kRsSeg + 2 * kHalo;        // longest filtered range
    static constexpr int kRowPitch = kR + 1;             // samples; odd
};

template <int ORDER, bool VEC>
__global__ __launch_bounds__(256) void k_spline_cols(float* __restrict__ out, const float* __restrict__ in, const int ny,
                                                     const int W, const float z0, const float z1, const float gain) {
    using Cfg = RsCfg<ORDER>;
    __shared__ __attribute__((aligned(16))) float tile[Cfg::kR * kRsColW];
    const int tid = threadIdx.x;
    const RsSeg sg = rs_segment((int)blockIdx.y, ny, Cfg::kHalo);
    const int x0 = (int)blockIdx.x * kRsColW, len = sg.b1 - sg.a0;
    const long long base = (long long)blockIdx.z * ny * W;
    if constexpr (VEC) {
        for (int u = tid; u < len * (kRsColW / 4); u += 256) {
            const int r = u / (kRsColW / 4), c = (u % (kRsColW / 4)) * 4;
            if (x0 + c < W)
                *(vec4f*)&tile[r * kRsColW + c] = *(const vec4f*)(in + base + (long long)(sg.a0 + r) * W + x0 + c) * gain;
        }
    } else {
        for (int u = tid; u < len * kRsColW; u += 256) {
            const int r = u / kRsColW, c = u % kRsColW;
            if (x0 + c < W) tile[r * kRsColW + c] = in[base + (long long)(sg.a0 + r) * W + x0 + c] * gain;
        }
    }
    __syncthreads();
    if (tid < kRsColW && x0 + tid < W) {
        const float z[2] = {z0, z1};
        rs_filter_line<float>(tile + tid, kRsColW, len, sg.a0 == 0, sg.b1 == ny, ny, z, Cfg::kNp);
    }
    __syncthreads();
    const int r0 = sg.s0 - sg.a0, rows = sg.s1 - sg.s0;
    if constexpr (VEC) {
        for (int u = tid; u < rows * (kRsColW / 4); u += 256) {
            const int r = u / (kRsColW / 4), c = (u % (kRsColW / 4)) * 4;
            if (x0 + c < W) *(vec4f*)(out + base + (long long)(sg.s0 + r) * W + x0 + c) = *(const vec4f*)&tile[(r0 + r) * kRsColW + c];
        }
    } else {
        for (int u = tid; u < rows * kRsColW; u += 256) {
            const int r = u / kRsColW, c = u % kRsColW;
            if (x0 + c < W) out[base + (long long)(sg.s0 + r) * W + x0 + c] = tile[(r0 + r) * kRsColW + c];
        }
    }
}

// C channels interleaved along x (1: real, 2: complex); W = nx C floats per row
template <int ORDER, int C, bool VEC>
__global__ __launch_bounds__(256) void k_spline_rows(float* __restrict__ out, const float* __restrict__ in, const int ny,
                                                     const int nx, const float z0, const float z1, const float gain) {
    using Cfg = RsCfg<ORDER>;
    constexpr int kRows = kRsRowLines / C, kPitch = C * Cfg::kRowPitch;
    __shared__ float tile[kRows * kPitch];
    const int tid = threadIdx.x;
    const RsSeg sg = rs_segment((int)blockIdx.x, nx, Cfg::kHalo);
    const int y0 = (int)blockIdx.y * kRows, rows = ny - y0 < kRows ? ny - y0 : kRows;
    const int W = nx * C, flen = (sg.b1 - sg.a0) * C;
    const long long base = (long long)blockIdx.z * ny * W + (long long)y0 * W;
    if constexpr (VEC) {
        const int upr = flen / 4;
        for (int u = tid; u < rows * upr; u += 256) {
            const int r = u / upr, c = (u % upr) * 4;
            const vec4f v = *(const vec4f*)(in + base + (long long)r * W + sg.a0 * C + c) * gain;
            float* t = tile + r * kPitch + c;
            t[0] = v.x; t[1] = v.y; t[2] = v.z; t[3] = v.w;
        }
    } else {
        for (int u = tid; u < rows * flen; u += 256) {
            const int r = u / flen, c = u % flen;
            tile[r * kPitch + c] = in[base + (long long)r * W + sg.a0 * C + c] * gain;
        }
    }
    __syncthreads();
    if (tid < rows * C) {
        const float z[2] = {z0, z1};
        rs_filter_line<float>(tile + (tid / C) * kPitch + tid % C, C, sg.b1 - sg.a0, sg.a0 == 0, sg.b1 == nx, nx, z, Cfg::kNp);
    }
    __syncthreads();
    const int c0 = (sg.s0 - sg.a0) * C, olen = (sg.s1 - sg.s0) * C;
    if constexpr (VEC) {
        const int upr = olen / 4;
        for (int u = tid; u < rows * upr; u += 256) {
            const int r = u / upr, c = (u % upr) * 4;
            const float* t = tile + r * kPitch + c0 + c;
            *(vec4f*)(out + base + (long long)r * W + sg.s0 * C + c) = vec4f{t[0], t[1], t[2], t[3]};
        }
    } else {
        for (int u = tid; u < rows * olen; u += 256) {
            const int r = u / olen, c = u % olen;
            out[base + (long long)r * W + sg.s0 * C + c] = tile[r * kPitch + c0 + c];
        }
    }
}

__device__ __forceinline__ float rs_fma(const float w, const float c, const float acc) { return fmaf(w, c, acc); }
__device__ __forceinline__ rs_c32 rs_fma(const float w, const rs_c32 c, const rs_c32 acc) {
    return rs_c32{fmaf(w, c.x, acc.x), fmaf(w, c.y, acc.y)};
}

// sum_a wy[a] (sum_b wx[b] c[iy[a] pitch + ix[b]]), rows first, taps in index order
template <int ORDER, class T>
__device__ __forceinline__ T rs_taps(const T* __restrict__ c, const long long pitch, const int (&iy)[ORDER + 1],
                                     const int (&ix)[ORDER + 1], const float (&wy)[ORDER + 1], const float (&wx)[ORDER + 1]) {
    T acc = T(0);
#pragma unroll
    for (int a = 0; a <= ORDER; ++a) {
        const T* row = c + (long long)iy[a] * pitch;
        T s = T(0);
#pragma unroll
        for (int b = 0; b <= ORDER; ++b) s = rs_fma(wx[b], row[ix[b]], s);
        acc = rs_fma(wy[a], s, acc);
    }
    return acc;
}

template <int ORDER, bool CPLX>
__global__ __launch_bounds__(256) void k_warp(void* __restrict__ out_, const void* __restrict__ coef_,
                                              const double* __restrict__ xf_, const int ny, const int nx, const int oh,
                                              const int ow, const int flags, const float cre, const float cim,
                                              int* __restrict__ path) {
    using T = typename std::conditional<CPLX, rs_c32, float>::type;
    __shared__ T box[kRsBoxElems];
    const int tid = threadIdx.x, img = (int)blockIdx.z;
    T* out = (T*)out_ + (long long)img * oh * ow;
    const T* coef = (const T*)coef_ + (long long)img * ny * nx;
    double xf[6];
#pragma unroll
    for (int k = 0; k < 6; ++k) xf[k] = xf_[(long long)img * 6 + k];
    const int oy0 = (int)blockIdx.y * kRsTile, ox0 = (int)blockIdx.x * kRsTile;
    const int oy1 = oy0 + kRsTile - 1 < oh - 1 ? oy0 + kRsTile - 1 : oh - 1;
    const int ox1 = ox0 + kRsTile - 1 < ow - 1 ? ox0 + kRsTile - 1 : ow - 1;
    const RsBox b = rs_tile_box(xf, oy0, oy1, ox0, ox1, ny, nx, ORDER, flags);
    if (path && tid == 0) path[((long long)img * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = b.path;
    T cval;
    if constexpr (CPLX) cval = rs_c32{cre, cim};
    else cval = cre;
    const int ox = ox0 + (tid & 31);
    const int pitch = b.w | 1;
    if (b.path == RS_PATH_LDS) {
        for (int e = tid; e < b.h * b.w; e += 256) {
            const int r = e / b.w, c = e % b.w;
            box[r * pitch + c] = coef[(long long)(b.y0 + r) * nx + b.x0 + c];
        }
        __syncthreads();
    }
#pragma unroll 1
    for (int j = 0; j < 4; ++j) {
        const int oy = oy0 + (tid >> 5) + 8 * j;
        if (oy > oy1 || ox > ox1) continue;
        T v = cval;
        if (b.path != RS_PATH_CVAL) {
            double sy = rs_coord(xf[0], xf[1], xf[4], (double)oy, (double)ox);
            double sx = rs_coord(xf[2], xf[3], xf[5], (double)oy, (double)ox);
            if (rs_inside(sy, sx, ny, nx, flags)) {
                float ty, tx, wy[ORDER + 1], wx[ORDER + 1];
                const int by = rs_first_tap(sy, ORDER, ty), bx = rs_first_tap(sx, ORDER, tx);
                rs_weights<ORDER>(ty, wy);
                rs_weights<ORDER>(tx, wx);
                int iy[ORDER + 1], ix[ORDER + 1];
#pragma unroll
                for (int a = 0; a <= ORDER; ++a) {
                    iy[a] = rs_reflect(by + a, ny);
                    ix[a] = rs_reflect(bx + a, nx);
                }
                if (b.path == RS_PATH_LDS) {
#pragma unroll
                    for (int a = 0; a <= ORDER; ++a) {
                        iy[a] -= b.y0;
                        ix[a] -= b.x0;
                    }
                    v = rs_taps<ORDER, T>(box, pitch, iy, ix, wy, wx);
                } else {
                    v = rs_taps<ORDER, T>(coef, nx, iy, ix, wy, wx);
                }
            }
        }
        out[(long long)oy * ow + ox] = v;
    }
}

// per workgroup (blockIdx.x of gridDim.x per image, image blockIdx.y): sum w, w y, w x, w y^2, w x^2 over its pixels
__global__ __launch_bounds__(256) void k_moments(double* __restrict__ work, const float* __restrict__ x,
                                                 const float* __restrict__ weight, const int ny, const int nx, const int cplx,
                                                 const int which) {
    __shared__ double part[4 * 5];
    const unsigned npix = (unsigned)ny * (unsigned)nx;
    const long long img = blockIdx.y;
    const float* xi = x + img * (long long)npix * (cplx ? 2 : 1);
    const float* wi = weight ? weight + img * (long long)npix : nullptr;
    double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (unsigned i = blockIdx.x * 256u + threadIdx.x; i < npix; i += gridDim.x * 256u) {
        float w;
        if (cplx) {
            const float re = xi[2ull * i], im = xi[2ull * i + 1];
            w = __fadd_rn(__fmul_rn(re, re), __fmul_rn(im, im));
        } else {
            w = xi[i];
            if (which == RS_POSITIVE) w = w > 0.0f ? w : 0.0f;
            if (which == RS_POWER) w = __fmul_rn(w, w);
        }
        if (wi) w = __fmul_rn(w, wi[i]);
        const double d = (double)w, yy = (double)(i / (unsigned)nx), xx = (double)(i % (unsigned)nx);
        v[0] += d;
        v[1] += d * yy;
        v[2] += d * xx;
        v[3] += d * yy * yy;
        v[4] += d * xx * xx;
    }
    block_sum<5>(v, work + (img * gridDim.x + blockIdx.x) * kRsMomWords, part);
}

// one workgroup per image: the workgroups' sums in index order
__global__ __launch_bounds__(64) void k_moments_fold(double* __restrict__ sums, const double* __restrict__ work, const int nb) {
    const long long img = blockIdx.x;
    if (threadIdx.x >= 5) return;
    double s = 0.0;
    for (int b = 0; b < nb; ++b) s += work[(img * nb + b) * kRsMomWords + threadIdx.x];
    sums[img * 5 + threadIdx.x] = s;
}

#endif  // __HIPCC__

}  // namespace pty
