// k_modes.hpp -- orthogonal incoherent probe modes (ptycho_orthogonalize_modes, CGPtychoSolver.run(ortho_prb=True)).
//
// For every angle t the M modes of the probe form the columns of P = [nprb^2, M].  With G = P^H P = V diag(lambda) V^H
// (Hermitian, formed in float64), the modes are replaced by P V: mode 0 is the strongest and the new modes are mutually
// orthogonal, with powers lambda (descending; sum lambda = sum_k |P_k|^2).  Two launches:
//
//   k_mode_gram_eig<M>  one workgroup per angle: the upper triangle of G over the pixels in a fixed order (per-thread
//                       float64 sums, a shuffle tree per wave, the four waves added in order: no atomics, so the result
//                       is bitwise reproducible), then a cyclic Jacobi solve of G in LDS (jacobi_herm below), the sort
//                       and the phase convention (eig_finish); writes V (complex128 [M][M]) and lambda (float64 [M]);
//   k_mode_rotate<M>    y_j = sum_k V_kj x_k in place, for the probe and up to two companions ([ptheta][M][npix]
//                       complex64 each); every thread loads the M values of its pixel before it writes.
//
// jacobi_herm / eig_finish are plain C++ over a "team" (HostTeam: one thread walks every index; the device team: the
// threads of the workgroup split the indices and meet at a barrier), so tests/test_ortho_cpu.py compiles them with the host
// compiler and compares them with numpy.linalg.eigh.
#pragma once

#include <cmath>

#if defined(__HIPCC__)
#define PTY_HD __host__ __device__
#else
#define PTY_HD inline
#endif

namespace pty {

constexpr int kOrthoMaxModes = 16;
constexpr int kJacobiMaxSweeps = 40;
constexpr double kJacobiTol = 1e-14;   // stop once the off-diagonal Frobenius norm is below kJacobiTol * ||G||_F

// one thread does everything, in index order
struct HostTeam {
    PTY_HD int first() const { return 0; }
    PTY_HD int step() const { return 1; }
    PTY_HD void sync() const {}
};

// (x_p, x_q) <- (c x_p - s f x_q, s x_p + c f x_q) with f = fr + i fi, |f| = 1
PTY_HD void rotate_pair(double* xr, double* xi, const int p, const int q, const double c, const double s, const double fr,
                        const double fi) {
    const double pr = xr[p], pi = xi[p];
    const double ur = xr[q] * fr - xi[q] * fi, ui = xi[q] * fr + xr[q] * fi;
    xr[p] = c * pr - s * ur;
    xi[p] = c * pi - s * ui;
    xr[q] = s * pr + c * ur;
    xi[q] = s * pi + c * ui;
}

// Cyclic Jacobi on the Hermitian M x M matrix G (row-major re / im arrays, ld = M), in place: on return G is diagonal
// (the eigenvalues, unsorted) and the columns of V (re / im, ld = M) are the eigenvectors, G_in = V diag(G) V^H.
// Rotation (p, q), with g = G_pq = r e (r = |g|, |e| = 1): J = [[c, s], [-s conj(e), c conj(e)]] on rows / columns p, q,
// c, s of the real symmetric Schur step on [[G_pp, r], [r, G_qq]]; G <- J^H G J (columns, then rows; the 2 x 2 block is
// set to its exact result), V <- V J.  Every member of the team evaluates the rotation from the same LDS words, so every
// branch below is uniform.  Returns the number of sweeps.
template <class Team>
PTY_HD int jacobi_herm(const Team& tm, double* gr, double* gi, double* vr, double* vi, const int M) {
    for (int k = tm.first(); k < M * M; k += tm.step()) {
        vr[k] = (k / M == k % M) ? 1.0 : 0.0;
        vi[k] = 0.0;
    }
    for (int k = tm.first(); k < M; k += tm.step()) gi[k * M + k] = 0.0;   // Hermitian: a real diagonal
    tm.sync();
    double nrm = 0.0;
    for (int k = 0; k < M * M; ++k) nrm += gr[k] * gr[k] + gi[k] * gi[k];
    const double tol2 = kJacobiTol * kJacobiTol * nrm;
    int sweep = 0;
    for (; sweep < kJacobiMaxSweeps; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < M; ++p)
            for (int q = p + 1; q < M; ++q) off += 2.0 * (gr[p * M + q] * gr[p * M + q] + gi[p * M + q] * gi[p * M + q]);
        if (off <= tol2) break;
        for (int p = 0; p < M; ++p) {
            for (int q = p + 1; q < M; ++q) {
                const double a = gr[p * M + p], b = gr[q * M + q], xr = gr[p * M + q], xi = gi[p * M + q];
                const double r = std::sqrt(xr * xr + xi * xi);
                if (r == 0.0) continue;
                const double er = xr / r, ei = xi / r;
                const double tau = (b - a) / (2.0 * r);
                const double t = (tau >= 0.0 ? 1.0 : -1.0) / (std::fabs(tau) + std::sqrt(1.0 + tau * tau));
                const double c = 1.0 / std::sqrt(1.0 + t * t), s = t * c;
                tm.sync();   // every member has read a, b, g
                // columns: col_p <- c col_p - s conj(e) col_q,  col_q <- s col_p + c conj(e) col_q  (G and V)
                for (int k = tm.first(); k < M; k += tm.step()) {
                    rotate_pair(gr + k * M, gi + k * M, p, q, c, s, er, -ei);
                    rotate_pair(vr + k * M, vi + k * M, p, q, c, s, er, -ei);
                }
                tm.sync();
                // rows: row_p <- c row_p - s e row_q,  row_q <- s row_p + c e row_q; the 2 x 2 block exactly
                for (int k = tm.first(); k < M; k += tm.step()) {
                    if (k == p) {
                        gr[p * M + p] = a - t * r;
                        gi[p * M + p] = 0.0;
                        gr[q * M + p] = 0.0;
                        gi[q * M + p] = 0.0;
                    } else if (k == q) {
                        gr[q * M + q] = b + t * r;
                        gi[q * M + q] = 0.0;
                        gr[p * M + q] = 0.0;
                        gi[p * M + q] = 0.0;
                    } else {
                        const double pr = gr[p * M + k], pi = gi[p * M + k];
                        const double qr = gr[q * M + k], qi = gi[q * M + k];
                        const double ur = qr * er - qi * ei, ui = qi * er + qr * ei;   // e row_q
                        gr[p * M + k] = c * pr - s * ur;
                        gi[p * M + k] = c * pi - s * ui;
                        gr[q * M + k] = s * pr + c * ur;
                        gi[q * M + k] = s * pi + c * ui;
                    }
                }
                tm.sync();
            }
        }
    }
    return sweep;
}

// After jacobi_herm: eigenvalue j goes to position rank(j) = #{i : lambda_i > lambda_j} + #{i < j : lambda_i == lambda_j}
// (descending, stable by index on exact ties), and its eigenvector is scaled so that its component of largest magnitude
// (the lowest index on exact ties) is real and positive.  out: complex [M][M] (row k, column = rank), lam: [M].
template <class Team>
PTY_HD void eig_finish(const Team& tm, const double* gr, const double* vr, const double* vi, const int M,
                       double* out_re, double* out_im, const int out_stride, double* lam) {
    for (int j = tm.first(); j < M; j += tm.step()) {
        const double lj = gr[j * M + j];
        int rank = 0;
        for (int i = 0; i < M; ++i) {
            const double li = gr[i * M + i];
            rank += (li > lj || (li == lj && i < j)) ? 1 : 0;
        }
        int kmax = 0;
        double m2 = -1.0;
        for (int k = 0; k < M; ++k) {
            const double a2 = vr[k * M + j] * vr[k * M + j] + vi[k * M + j] * vi[k * M + j];
            if (a2 > m2) {
                m2 = a2;
                kmax = k;
            }
        }
        const double am = std::sqrt(m2);
        const double fr = vr[kmax * M + j] / am, fi = -vi[kmax * M + j] / am;   // conj(v_kmax) / |v_kmax|
        for (int k = 0; k < M; ++k) {
            const double xr = vr[k * M + j], xi = vi[k * M + j];
            out_re[(k * M + rank) * out_stride] = xr * fr - xi * fi;
            out_im[(k * M + rank) * out_stride] = xr * fi + xi * fr;
        }
        out_im[(kmax * M + rank) * out_stride] = 0.0;
        lam[rank] = lj;
    }
    tm.sync();
}

// pair e of the upper triangle, row by row: (0,0), (0,1) .. (0,M-1), (1,1), ...
PTY_HD constexpr void mode_pair(int e, const int M, int& j, int& k) {
    j = 0;
    while (e >= M - j) {
        e -= M - j;
        ++j;
    }
    k = j + e;
}

#if defined(__HIPCC__)

struct WorkgroupTeam {
    __device__ int first() const { return (int)threadIdx.x; }
    __device__ int step() const { return (int)blockDim.x; }
    __device__ void sync() const { __syncthreads(); }
};

// Gram entries c0 .. c0 + CH of the upper triangle (pairs of mode_pair) over all pixels, into gr / gi (both triangles).
// Per thread a float64 complex sum over the pixels tid, tid + 256, ... (U pixels x M modes loaded before they are added),
// then a shuffle tree per wave and the four waves added in order.
template <int M, int C0>
__device__ __forceinline__ void gram_pass(const c32* __restrict__ base, const long long npix, double* part, double* gr, double* gi) {
    constexpr int NP = M * (M + 1) / 2;
    constexpr int CH = NP < 16 ? NP : 16;
    constexpr int NE = NP - C0 < CH ? NP - C0 : CH;   // entries of this pass
    constexpr int U = M >= 16 ? 1 : 16 / M;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    double ar[NE], ai[NE];
#pragma unroll
    for (int e = 0; e < NE; ++e) ar[e] = ai[e] = 0.0;
    for (long long x0 = tid; x0 < npix; x0 += 256 * U) {
        c32 v[U][M];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const long long x = x0 + 256 * u;
#pragma unroll
            for (int k = 0; k < M; ++k) v[u][k] = x < npix ? base[(size_t)k * npix + x] : c32{0.0f, 0.0f};
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
#pragma unroll
            for (int j = 0; j < M; ++j) {
#pragma unroll
                for (int k = j; k < M; ++k) {
                    const int e = j * M - j * (j - 1) / 2 + (k - j) - C0;   // mode_pair's index of (j, k), this pass
                    if (e < 0 || e >= NE) continue;
                    const double pr = v[u][j].x, pi = v[u][j].y, qr = v[u][k].x, qi = v[u][k].y;
                    ar[e] += pr * qr + pi * qi;   // conj(P_j) P_k
                    ai[e] += pr * qi - pi * qr;
                }
            }
        }
    }
#pragma unroll
    for (int e = 0; e < NE; ++e) {
#pragma unroll
        for (int o = 32; o >= 1; o >>= 1) {
            ar[e] += __shfl_xor(ar[e], o);
            ai[e] += __shfl_xor(ai[e], o);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int e = 0; e < NE; ++e) {
            part[wave * 2 * CH + 2 * e] = ar[e];
            part[wave * 2 * CH + 2 * e + 1] = ai[e];
        }
    }
    __syncthreads();
    if (tid < NE) {
        int j = 0, k = 0;
        mode_pair(C0 + tid, M, j, k);
        const double* w = part + 2 * tid;
        const double sr = ((w[0] + w[2 * CH]) + w[4 * CH]) + w[6 * CH];
        const double si = ((w[1] + w[2 * CH + 1]) + w[4 * CH + 1]) + w[6 * CH + 1];
        gr[j * M + k] = sr;
        gi[j * M + k] = si;
        gr[k * M + j] = sr;
        gi[k * M + j] = -si;
    }
    __syncthreads();
    if constexpr (C0 + CH < NP) gram_pass<M, C0 + CH>(base, npix, part, gr, gi);
}

// One workgroup (256 threads) per angle: G by gram_pass (CH <= 16 float64 complex accumulators per thread and pass), the
// Jacobi solve, the sort and the phase convention; V (complex128 [M][M]) and the powers to the caller's buffers.
template <int M>
__global__ __launch_bounds__(256) void k_mode_gram_eig(const c32* __restrict__ prb, const long long npix,
                                                       double* __restrict__ v_out, double* __restrict__ powers) {
    constexpr int NP = M * (M + 1) / 2;
    constexpr int CH = NP < 16 ? NP : 16;
    __shared__ double gr[M * M], gi[M * M], vr[M * M], vi[M * M];
    __shared__ double part[4 * 2 * CH];
    gram_pass<M, 0>(prb + (size_t)blockIdx.x * M * (size_t)npix, npix, part, gr, gi);
    const WorkgroupTeam tm;
    jacobi_herm(tm, gr, gi, vr, vi, M);
    double* vo = v_out + (size_t)blockIdx.x * M * M * 2;   // complex128 [M][M]
    eig_finish(tm, gr, vr, vi, M, vo, vo + 1, 2, powers + (size_t)blockIdx.x * M);
}

struct ModeRotateArgs {
    c32* x[3];            // probe and up to two companions, [ptheta][M][npix] each
    const double* v;      // complex128 [ptheta][M][M] (k_mode_gram_eig)
    long long npix;
    long long blocks;     // workgroups per (array, angle): ceil(npix / 256)
    int ptheta;
};

// workgroup b: array b / (ptheta blocks), angle (b / blocks) % ptheta, pixels 256 (b % blocks) + [0, 256)
template <int M>
__global__ __launch_bounds__(256) void k_mode_rotate(const ModeRotateArgs a) {
    __shared__ double vs[M * M * 2];
    const long long b = blockIdx.x;
    const long long blk = b % a.blocks;
    const long long t = (b / a.blocks) % a.ptheta;
    const int arr = (int)(b / (a.blocks * a.ptheta));
    const int tid = threadIdx.x;
    for (int i = tid; i < M * M * 2; i += 256) vs[i] = a.v[(size_t)t * M * M * 2 + i];
    __syncthreads();
    const long long x = blk * 256 + tid;
    if (x >= a.npix) return;
    c32* p = a.x[arr] + (size_t)t * M * (size_t)a.npix + x;
    c32 in[M];
#pragma unroll
    for (int k = 0; k < M; ++k) in[k] = p[(size_t)k * a.npix];
#pragma unroll
    for (int j = 0; j < M; ++j) {
        double yr = 0.0, yi = 0.0;
#pragma unroll
        for (int k = 0; k < M; ++k) {
            const double wr = vs[2 * (k * M + j)], wi = vs[2 * (k * M + j) + 1];
            yr += wr * in[k].x - wi * in[k].y;
            yi += wr * in[k].y + wi * in[k].x;
        }
        p[(size_t)j * a.npix] = c32{(float)yr, (float)yi};
    }
}

#endif  // __HIPCC__

}  // namespace pty
