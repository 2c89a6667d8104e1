// k_propagate.hpp -- free-space propagation of square complex fields and the figures of a focus series
// (ptycho_propagate, libtike.hipfft.propagate).  Part of libptychohip: included inside the anonymous namespace of
// ptycho_kernels.hip after k_tile.hpp; csrc/host_propagate.cpp includes it the same way (after fft_core.hpp and
// frame_part.hpp) and checks everything outside the __HIPCC__ guard on the host.
//
// plane[f][d] = IDFT(spec[f] H_d), spec the unnormalised forward DFT of field f, H_d the transfer function of distance
// d (include/ptycho_hip.h states it; prop_turns is its phase), and per (f, d) eight float64 words over v = |plane|^2:
// {sum v, sum v^2, sum v y, sum v x, sum v y^2, sum v x^2, max v, flat index of the first maximum}.
//
//   k_prop_tile<N>   sides with a plan and a tile that fits a compute unit's LDS (16 ... 128), option "tile" on: ONE launch.
//                    Persistent workgroups walk the pairs j = f nplane + d (consecutive workgroups share a spectrum, which
//                    they read from L2 with plain 16-byte loads); spec H_d goes into the LDS tile, the row and the column
//                    IDFT run there (tile_dft / tile_put, as k_rows_tile<N, +1, true>), and one epilogue reads the tile
//                    once: the plane leaves in 16-byte nontemporal stores if it was asked for, each thread adds its pixels
//                    to eight figures in float64, and the threads of the TILE reduce them (prop_group: a shuffle tree
//                    inside groups of GW lanes, then the NG groups of the tile in order through LDS).  No plane reaches
//                    memory unless it was asked for.
//   k_prop_apply     every other side: spec H_d for all pairs (H_d is evaluated once per pixel and plane and multiplies
//                    every field); the project's in-place inverse transform follows (do_fft2 / do_fft2_generic);
//   k_prop_metrics   then one 256-thread workgroup per pair: pixels in flat order, block_sum, the same max rule.
//
// v is formed in float32 as round(round(re re) + round(im im)) -- no fused multiply-add, so that a host restatement forms
// the same bits -- and converted to double; every term of the six sums is then exact in float64 (24-bit v times an index
// below 2^11, or its square) and only the order of the additions is the kernel's own: fixed, no atomics, the same inputs
// on the same path give the same bits.  A NaN v is skipped by the max (the comparison is false) and propagates into the
// sums; with no comparable v at all the max is -inf and the index -1.  Larger value first, lower index on ties.
#pragma once

// ---- plain C++: checked on the host by host_propagate.cpp ----------------------------------------------------------------

// integer frequency of index i of an s-point DFT (numpy.fft.fftfreq(s) * s)
PTY_HD constexpr int prop_freq(const int i, const int s) { return i <= (s - 1) / 2 ? i : i - s; }

// Phase of the transfer function at frequency (ky, kx) in turns, reduced to [-0.5, 0.5]; false: evanescent, H = 0.
// q = q0 (ky^2 + kx^2), zl = z / lambda.  method 0 (Fresnel): -zl q / 2; method 1 (angular spectrum, carrier removed):
// -zl q / (1 + sqrt(1 - q)) for q <= 1, the cancellation-free form of zl (sqrt(1 - q) - 1).  All float64: zl q reaches
// 1e7 turns and more, and float32 keeps 1e-7 of that.  (No contraction: 1 - q0 k2 in one rounding would move t by
// zl eps / sqrt(1 - q), and a host restatement would not follow.)
PTY_HD bool prop_turns(const int method, const double zl, const double q0, const int ky, const int kx, double& t) {
#pragma clang fp contract(off)
    const double k2 = (double)((long long)ky * ky + (long long)kx * kx);
    const double q = q0 * k2;
    t = 0.0;
    if (method == 0) {
        t = -0.5 * zl * q;
    } else {
        if (!(q <= 1.0)) return false;
        t = -zl * q / (1.0 + std::sqrt(1.0 - q));
    }
    t -= std::rint(t);
    return true;
}

// Which threads reduce together in k_prop_tile<N>.  A tile has TT = N T threads (TileCfg<N>::TT), TPW tiles share a
// workgroup of NT threads.  The threads of a tile form NG groups of GW consecutive threads; a group lies inside one wave
// at a multiple of GW (GW a power of two <= 64), so a xor-shuffle tree with offsets below GW never leaves it: 16 lanes at
// N = 16 (four tiles to a wave), the whole wave from N = 32 on, where the NG = TT / 64 waves of a tile then add up in LDS.
template <int N>
struct PropCfg {
    static constexpr int TT = N * Plan<N>::T;
    static constexpr int TPW = TT >= 256 ? 1 : 256 / TT;
    static constexpr int NT = TT * TPW;
    static constexpr int GW = TT < 64 ? TT : 64;
    static constexpr int NG = TT / GW;
    static_assert((GW & (GW - 1)) == 0 && TT % GW == 0 && NT % 64 == 0, "groups tile the waves: no wave is partly idle");
};
// thread tid of the workgroup -> tile slot w, group g of that tile, position r in the group (r = 0 writes)
PTY_HD void prop_group(const int tid, const int tt, const int gw, int& w, int& g, int& r) {
    w = tid / tt;
    const int t = tid % tt;
    g = t / gw;
    r = t % gw;
}

constexpr int kPropWords = 8;                       // float64 words per (field, plane)
constexpr unsigned long long kPropMaxPairs = 1ull << 30;

#if defined(__HIPCC__)

struct PropArgs {
    c32* planes;           // [nfield][nplane][S][S] or null
    double* metrics;       // [nfield][nplane][8] or null
    const c32* spec;       // [nfield][S][S]
    const double* zl;      // [nplane], device
    c32* work;             // two-pass path without planes: [nfield][nplane][S][S]
    long long nfield, nplane;
    double q0;
    int method;
};

// H at (ky, kx): exp(2 pi i t) / S^2 formed in float64 and rounded once
__device__ __forceinline__ c32 prop_h(const int method, const double zl, const double q0, const int ky, const int kx,
                                      const double inv) {
    double t;
    if (!prop_turns(method, zl, q0, ky, kx, t)) return c32{0.0f, 0.0f};
    double sn, cs;
    sincospi(2.0 * t, &sn, &cs);
    return c32{(float)(cs * inv), (float)(sn * inv)};
}

struct PropAcc {
    double s[6];
    float m;
    int i;
};
__device__ __forceinline__ PropAcc prop_acc_init() {
    return PropAcc{{0.0, 0.0, 0.0, 0.0, 0.0, 0.0}, -INFINITY, 0x7fffffff};
}
__device__ __forceinline__ void prop_max(float& m, int& i, const float om, const int oi) {
    if (om > m || (om == m && oi < i)) { m = om; i = oi; }
}
// pixel (y, x) of a plane; a thread meets its pixels in ascending flat order, so `>` keeps its first maximum
__device__ __forceinline__ void prop_add(PropAcc& a, const c32 p, const int y, const int x, const int flat) {
    const float vf = __fadd_rn(__fmul_rn(p.x, p.x), __fmul_rn(p.y, p.y));
    const double v = (double)vf;
    a.s[0] += v;
    a.s[1] += v * v;
    a.s[2] += v * (double)y;
    a.s[3] += v * (double)x;
    a.s[4] += v * (double)(y * y);
    a.s[5] += v * (double)(x * x);
    if (vf > a.m) { a.m = vf; a.i = flat; }
}
// butterfly over the GW lanes of a group: every lane ends with the group's figures
template <int GW>
__device__ __forceinline__ void prop_group_reduce(PropAcc& a) {
#pragma unroll
    for (int e = 0; e < 6; ++e) {
#pragma unroll
        for (int o = GW / 2; o >= 1; o >>= 1) a.s[e] += __shfl_xor(a.s[e], o);
    }
#pragma unroll
    for (int o = GW / 2; o >= 1; o >>= 1) {
        const float om = __shfl_xor(a.m, o);
        const int oi = __shfl_xor(a.i, o);
        prop_max(a.m, a.i, om, oi);
    }
}
__device__ __forceinline__ void prop_write(double* __restrict__ out, const PropAcc& a) {
#pragma unroll
    for (int e = 0; e < 6; ++e) out[e] = a.s[e];
    out[6] = (double)a.m;
    out[7] = a.i == 0x7fffffff ? -1.0 : (double)a.i;
}

template <int N>
__global__ __launch_bounds__(TileCfg<N>::NT) void k_prop_tile(const PropArgs a, const c32* __restrict__ table) {
    using CF = TileCfg<N>;
    using P = Plan<N>;
    using PC = PropCfg<N>;
    static_assert(PC::TT == CF::TT && PC::TPW == CF::TPW && PC::NT == CF::NT && CF::CPT == 1, "PropCfg restates TileCfg");
    constexpr int E = P::E, TT = CF::TT, TPW = CF::TPW, LS = CF::LS, CPT = CF::CPT, NL = CF::NL, GW = PC::GW, NG = PC::NG;
    __shared__ c32 lds[TPW * N * LS];
    __shared__ c32 wtab[N];
    __shared__ double part[NG > 1 ? NG * kPropWords : 1];
    const int tid = threadIdx.x, t = tid % TT;
    int w, g, r;
    prop_group(tid, TT, GW, w, g, r);
    const int c = t % NL, j0 = t / NL;
    c32* tile = lds + w * N * LS;
    for (int i = tid; i < N; i += CF::NT) wtab[i] = table[i];
    __syncthreads();
    const int npairs = (int)(a.nfield * a.nplane), nplane = (int)a.nplane;   // the host checks npairs < 2^30
    const double inv = 1.0 / ((double)N * (double)N);
    for (int base = blockIdx.x * TPW; base < npairs; base += gridDim.x * TPW) {
        const bool live = base + w < npairs;
        const int j = live ? base + w : npairs - 1;   // an idle tile slot of the last trip repeats a pair and writes nothing
        const int f = j / nplane, d = j % nplane;
        const double zl = a.zl[d];
        // ---- spec H_d -> tile: whole rows, 16 bytes per lane, plain loads (the spectrum is read nplane times) ----
        const f32x4* in = reinterpret_cast<const f32x4*>(a.spec + (size_t)f * N * N);
#pragma unroll 1
        for (int u = t; u < N * N / 2; u += TT) {
            const int row = u / (N / 2), cu = (u % (N / 2)) * 2;
            const f32x4 val = in[u];
            const int ky = prop_freq(row, N);
            const c32 h0 = prop_h(a.method, zl, a.q0, ky, prop_freq(cu, N), inv);
            const c32 h1 = prop_h(a.method, zl, a.q0, ky, prop_freq(cu + 1, N), inv);
            tile[row * LS + cu] = cmul(c32{val.x, val.y}, h0);
            tile[row * LS + cu + 1] = cmul(c32{val.z, val.w}, h1);
        }
        __syncthreads();
        // ---- IDFT over x of the thread's rows, then over y of its columns ----
        {
            c32 v[CPT][E];
            // (an opaque copy of j0, as in k_fwd_tile: it keeps the tile and twiddle addresses of each transform inside the
            // pair loop; hoisted out of it they stay live across the float64 sincospi above and k_prop_tile<128> spills)
            int jv = j0;
            asm volatile("" : "+v"(jv));
            tile_dft<N, +1, true, true>(v, tile, wtab, c, jv);
            if (P::NSTEP > 1) __syncthreads();
            tile_put<N, +1, true>(v, tile, c, jv);
            __syncthreads();
            asm volatile("" : "+v"(jv));
            tile_dft<N, +1, false, true>(v, tile, wtab, c, jv);
            if (P::NSTEP > 1) __syncthreads();
            tile_put<N, +1, false>(v, tile, c, jv);
            __syncthreads();
        }
        // ---- one read of the tile: the plane to memory if wanted, the pixels into the thread's figures ----
        PropAcc acc = prop_acc_init();
        f32x4* out = a.planes && live ? reinterpret_cast<f32x4*>(a.planes + (size_t)j * N * N) : nullptr;
#pragma unroll 1
        for (int u = t; u < N * N / 2; u += TT) {
            const int row = u / (N / 2), cu = (u % (N / 2)) * 2;
            const c32 lo = tile[row * LS + cu], hi = tile[row * LS + cu + 1];
            if (out) __builtin_nontemporal_store(f32x4{lo.x, lo.y, hi.x, hi.y}, out + u);
            if (a.metrics) {
                prop_add(acc, lo, row, cu, row * N + cu);
                prop_add(acc, hi, row, cu + 1, row * N + cu + 1);
            }
        }
        if (a.metrics) {   // (uniform over the workgroup: the barrier below is met by every thread or by none)
            prop_group_reduce<GW>(acc);
            double* dst = a.metrics + (size_t)j * kPropWords;
            if constexpr (NG > 1) {
                // one tile per workgroup: its NG waves leave their figures in LDS, thread 0 adds them in wave order
                if (r == 0) {
#pragma unroll
                    for (int e = 0; e < 6; ++e) part[g * kPropWords + e] = acc.s[e];
                    part[g * kPropWords + 6] = (double)acc.m;
                    part[g * kPropWords + 7] = (double)acc.i;
                }
                __syncthreads();
                if (t == 0 && live) {
#pragma unroll 1   // (unrolled, the 15 x 8 partials of N = 128 are all requested at once and spill)
                    for (int gg = 1; gg < NG; ++gg) {
#pragma unroll
                        for (int e = 0; e < 6; ++e) acc.s[e] += part[gg * kPropWords + e];
                        prop_max(acc.m, acc.i, (float)part[gg * kPropWords + 6], (int)part[gg * kPropWords + 7]);
                    }
                    prop_write(dst, acc);
                }
            } else if (r == 0 && live) {
                prop_write(dst, acc);
            }
        }
        __syncthreads();   // the tile and the partials are rewritten by the next pair
    }
}

// grid (ceil(S^2 / 256), min(nplane, 65535)), 256 threads: pixel i of plane d for every field
__global__ __launch_bounds__(256) void k_prop_apply(c32* __restrict__ dst, const c32* __restrict__ spec,
                                                    const double* __restrict__ zlv, const long long nfield,
                                                    const long long nplane, const int s, const double q0, const int method) {
    const long long npix = (long long)s * s;
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= npix) return;
    const int ky = prop_freq((int)(i / s), s), kx = prop_freq((int)(i % s), s);
    const double inv = 1.0 / ((double)s * (double)s);
    for (long long d = blockIdx.y; d < nplane; d += gridDim.y) {
        const c32 h = prop_h(method, zlv[d], q0, ky, kx, inv);
        for (long long f = 0; f < nfield; ++f) dst[(size_t)((f * nplane + d) * npix + i)] = cmul(spec[(size_t)(f * npix + i)], h);
    }
}

// grid min(npairs, cap), 256 threads: the pairs j = blockIdx.x, + gridDim.x, ...; pixels in flat order
__global__ __launch_bounds__(256) void k_prop_metrics(double* __restrict__ metrics, const c32* __restrict__ planes,
                                                      const long long npairs, const int s) {
    __shared__ double part[4 * 6];
    __shared__ float pm[4];
    __shared__ int pi[4];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int npix = s * s;   // s <= 2048
    for (long long j = blockIdx.x; j < npairs; j += gridDim.x) {
        const c32* p = planes + (size_t)j * npix;
        PropAcc acc = prop_acc_init();
        for (int i = tid; i < npix; i += 256) prop_add(acc, p[i], i / s, i % s, i);
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            const float om = __shfl_xor(acc.m, o);
            const int oi = __shfl_xor(acc.i, o);
            prop_max(acc.m, acc.i, om, oi);
        }
        if (lane == 0) { pm[wave] = acc.m; pi[wave] = acc.i; }
        double* dst = metrics + (size_t)j * kPropWords;
        block_sum<6>(acc.s, dst, part);   // (its barriers also publish pm / pi)
        if (tid == 0) {
            PropAcc top = prop_acc_init();
            for (int k = 0; k < 4; ++k) prop_max(top.m, top.i, pm[k], pi[k]);
            dst[6] = (double)top.m;
            dst[7] = top.i == 0x7fffffff ? -1.0 : (double)top.i;
        }
        __syncthreads();   // pm / pi / part are rewritten by the next pair
    }
}

#endif  // __HIPCC__
