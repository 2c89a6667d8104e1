/* ptycho_hip.h -- C ABI of libptychohip.so (gfx950 / MI355X).
 *
 * Drop-in boundary for the native class `ptychofft` of nikitinvv/libtike-cufft
 * (reference paths relative to /root/reference):
 *
 *   ptychofft::ptychofft(ptheta,nz,n,nscan,ndet,nprb)  src/include/ptychofft.cuh:35-36, src/cuda/ptychofft.cu:5-41
 *   ptychofft::fwd(g,f,scan,prb)                       src/include/ptychofft.cuh:40,    src/cuda/ptychofft.cu:60-73
 *   ptychofft::adj(f,g,scan,prb,flg)                   src/include/ptychofft.cuh:42,    src/cuda/ptychofft.cu:76-88
 *   ptychofft::free() / ~ptychofft()                   src/include/ptychofft.cuh:38,43, src/cuda/ptychofft.cu:44-57
 *   read-only fields ptheta,nz,n,nscan,ndet,nprb       src/cuda/swig/ptychofft.i:11-16
 *
 * Differences from the reference interface, on purpose:
 *   - plain C functions on an opaque handle instead of a SWIG/pybind11 class;
 *   - every entry point returns an int status (0 = ok) and validates its
 *     arguments; ptycho_last_error() describes the last failure of the calling
 *     thread (the reference returns void and checks nothing);
 *   - the caller's HIP stream is passed explicitly (the reference uses the
 *     legacy default stream); no per-call operand state is kept in the handle.
 *     Calls on ONE handle must be stream-serialised (same stream, or ordered by
 *     events): the handle owns scratch that the kernels of a call share -- the
 *     adjoint's intermediate, the position order, the CG work slots, the
 *     fixed-point image of the deterministic adjoints, and the ticket + partial-sum
 *     table through which every CG reduction adds up its workgroups in a fixed
 *     order.  Two stage calls of one handle running concurrently on different
 *     streams would mix their partial sums; use one handle per stream;
 *   - taps outside the object read as zero / are dropped instead of being
 *     undefined behaviour (the reference only rejects negative positions,
 *     src/cuda/kernels.cu:39).
 *
 * All device pointers are borrowed for the duration of the call.  Layouts
 * (C-contiguous, complex64 = interleaved float re,im):
 *   f    object   complex64 [ptheta][nz][n]
 *   g    farplane complex64 [ptheta][nscan][ndet][ndet]   (DC at [0][0])
 *   prb  probe    complex64 [ptheta][nprb][nprb]
 *   scan          float32   [ptheta][nscan][2]  ([..][0] = row/y, [..][1] = column/x)
 * ndet: 2 .. 1024, or a power of two up to 2048.  Sizes with a Stockham plan of their own run the fused kernels and the
 * CG stages below: the powers of two 16 .. 2048 and 48, 80, 96, 112, 192 (mixed radix 3 / 5 / 7 x 4|8 x 4|8; 112 is the crop of the
 * reference's tests/test_fsc.py:115-120); every other size runs a Bluestein transform on the next power-of-two plan (operators
 * and ptycho_fft2 only).  nprb <= ndet.
 */
#ifndef PTYCHO_HIP_H
#define PTYCHO_HIP_H

#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ptycho_handle_s* ptycho_handle;

enum {
    PTYCHO_OK = 0,
    PTYCHO_ERR_ARG = 1,      /* invalid argument / unsupported size */
    PTYCHO_ERR_HIP = 2,      /* a HIP runtime call failed */
    PTYCHO_ERR_FREED = 3     /* handle used after ptycho_free */
};

/* ptychofft ctor: builds the twiddle table and the chunk scratch.  ptheta * nscan < 2^30 positions; the processing order of
 * the windowed kernels is computed by a single-launch ranking kernel with n^2 / 2 key compares (39 us at 4096 positions,
 * ~0.1 ms at the 32768 positions of a configs[3] shard, tens of ms at 3e5): shard larger jobs over handles / GPUs by
 * position, as BASELINE.json configs[3] does, or keep scan unchanged between calls (option "trust_order"). */
int ptycho_create(ptycho_handle* out, size_t ptheta, size_t nz, size_t n,
                  size_t nscan, size_t ndet, size_t nprb);
/* ptychofft::free -- idempotent; the handle stays valid for ptycho_get/destroy. */
int ptycho_free(ptycho_handle h);
/* ~ptychofft: free + release the handle itself. */
int ptycho_destroy(ptycho_handle h);
/* read-only size fields: which = 0 ptheta, 1 nz, 2 n, 3 nscan, 4 ndet, 5 nprb;
 * 100: positions per launch pair of the adjoint (option "chunk"), 101: option "window";
 * 102: 1 if a measured-pixel mask is set (ptycho_set_mask), else 0;
 * 103: option "model" (0 gaussian, 1 poisson_ml);
 * 200 + slot (slot < 16): 1 if CG work slot `slot` (one farplane, ptheta * nscan * ndet^2 * 8 bytes) is allocated. */
long long ptycho_get(ptycho_handle h, int which);

/* g = F Q f : probe (x) bilinear patch, 1/ndet, centred zero pad, 2-D DFT. */
int ptycho_fwd(ptycho_handle h, void* g, const void* f, const void* scan,
               const void* prb, void* stream);
/* flg = 0: f   += Q* F* g   (f must be zeroed by the caller, as in the reference)
 * flg = 1: prb += O* F* g   (prb must be zeroed by the caller)
 * Same argument order as the reference; g is never modified. */
int ptycho_adj(ptycho_handle h, void* f, const void* g, const void* scan,
               void* prb, int flg, void* stream);

/* Batched unnormalised 2-D DFT of nbatch ndet x ndet complex64 tiles
 * (dir = -1 forward, +1 inverse; dst may equal src).  This is the cuFFT plan of
 * src/cuda/ptychofft.cu:14-20 exposed for the position registration
 * (cp.fft.ifft2 in src/libtike/cufft/ptycho.py:204). */
int ptycho_fft2(ptycho_handle h, void* dst, const void* src, size_t nbatch,
                int dir, void* stream);

/* Scan-position gradient (PtychoHIP.adj_scan, the backward of PtychoHIP.fwd_autograd; no counterpart in the reference):
 * out (float32 [ptheta][nscan][2]) <- the derivative of Re <g, F Q f> with respect to scan, g held fixed, inside the
 * interpolation cell that the position's truncation selects.  With (iy, ix) = trunc(scan) and (fy, fx) = scan - trunc(scan)
 * on the float32 value, the taps f00 = f[iy+i][ix+j], f01 = f[iy+i][ix+j+1], f10 = f[iy+i+1][ix+j], f11 = f[iy+i+1][ix+j+1]
 * (taps outside the object read 0), w = the centre nprb x nprb crop of the unnormalised inverse DFT of the position's tile
 * of g and c = 1 / ndet:
 *   out[..][0] = c Re sum_ij conj(w_ij) prb_ij ((f10 - f00)(1 - fx) + (f11 - f01) fx)
 *   out[..][1] = c Re sum_ij conj(w_ij) prb_ij ((f01 - f00)(1 - fy) + (f11 - f10) fy)
 * A position the operators skip (iy < 0 or ix < 0) gives exactly 0.0 twice; trunc(-0.3) = -0 is not skipped and has a
 * negative fraction, as in ptycho_fwd.  Every element of out is written: the caller need not zero it.
 * work: complex64 [work_tiles][ndet][ndet], work_tiles >= 1, not aliasing g; g is never modified.  The positions are taken in
 * chunks of work_tiles: ptycho_fft2 (dir = +1) of the chunk into work, then one launch of one workgroup per position
 * (csrc/k_scangrad.hpp), so every detector size of ptycho_fft2 works, the Bluestein sizes included.  Differences, weights and
 * the product with the probe are float32, the sum is float64 in a fixed order with no atomics: the same inputs give the
 * same bits, whatever work_tiles is.  Everything runs on `stream`, no host synchronisation; the position sort of the handle
 * is neither used nor changed.
 * PTYCHO_ERR_ARG, before any HIP call, for a null handle, a null out / g / f / scan / prb / work, work_tiles == 0, or
 * work == g (PTYCHO_ERR_FREED for a handle after ptycho_free). */
int ptycho_adj_scan(ptycho_handle h, float* out, const void* g, const void* f, const void* scan, const void* prb, void* work,
                    size_t work_tiles, void* stream);

/* Orthogonal incoherent probe modes (CGPtychoSolver.run(..., ortho_prb=True); no counterpart in the reference, whose
 * attempts are commented out at src/libtike/cufft/ptycho.py:414-419, 467-470).  Needs no handle.
 * prb (and dprb, gradprb0 when not null): complex64 [ptheta][nmodes][npix], npix = nprb^2, rotated in place.  Per angle t,
 * with P = [npix, nmodes] the modes of t: G = P^H P (float64, summed in a fixed order, bitwise reproducible),
 * G = V diag(lambda) V^H by cyclic Jacobi in float64 with lambda descending (stable by index on exact ties) and every
 * column of V scaled so that its component of largest magnitude (the lowest index on ties) is real and positive; then
 * X <- X V for each of the three arrays.  The new modes are orthogonal, mode 0 the strongest, and sum |P_k|^2 per pixel is
 * unchanged up to rounding.  Outputs: v_out complex128 [ptheta][nmodes][nmodes] (row k, column j = V_kj), powers float64
 * [ptheta][nmodes] = lambda.  nmodes = 1: V = 1, only the power is computed.  Two launches on `stream`, no host
 * synchronisation.  PTYCHO_ERR_ARG, before any HIP call, for nmodes outside [1, 16], a null prb / v_out / powers,
 * npix == 0 or ptheta == 0. */
int ptycho_orthogonalize_modes(void* prb, void* dprb, void* gradprb0, size_t ptheta, int nmodes, size_t npix,
                               void* v_out, double* powers, void* stream);

/* Fourier ring correlation (no handle; libtike.hipfft.frc).  Both calls are one launch on `stream`, no host
 * synchronisation; s (the crop side) must be in [16, 1024] or 2048, ptheta in [1, 32767].
 *   ptycho_frc_prepare  out (complex64 [2][ptheta][s][s]) <- the crops [.., y0:y0+s, x0:x0+s] of a, then of b (complex64
 *                       [ptheta][nz][n] each), times window[y] * window[x] (float32 [s]; NULL: no window)
 *   ptycho_frc_rings    sums (float64 [ptheta][s/2+1][5]) <- per angle and ring k = round(|f|) <= s/2 of the spectra in
 *                       spec (complex64 [2][ptheta][s][s], A then B): {Re C, Im C, PA, PB, n} with C = sum A conj(B'),
 *                       PA = sum |A|^2, PB = sum |B|^2, n the pixel count, B' = B exp(-2 pi i (fy dy + fx dx) / s) with
 *                       (dy, dx) = shift[angle] (float64 [ptheta][2] on the device; NULL: no shift).  Fixed summation
 *                       order, no atomics: the same inputs give the same bits.
 * PTYCHO_ERR_ARG, before any HIP call, for a null out / a / b / sums / spec, an unsupported s or ptheta, or a crop
 * outside the image. */
int ptycho_frc_prepare(void* out, const void* a, const void* b, size_t ptheta, size_t nz, size_t n, size_t y0, size_t x0,
                       size_t s, const float* window, void* stream);
int ptycho_frc_rings(double* sums, const void* spec, size_t ptheta, size_t s, const double* shift, void* stream);

/* Illumination map and gauge fixing (no handle; libtike.hipfft.gauge).  A ptychographic solution is defined up to one
 * complex factor traded between object and probe and a linear phase ramp on the object paired with the opposite ramp on
 * the probe; the poorly lit border means nothing.  Every launch runs on `stream`, nothing synchronises, no float atomics
 * and fixed summation orders: the same inputs give the same bits.  ptheta in [1, 65535].
 *   ptycho_illumination  out (float32 [ptheta][nz][n], written in full) <- the diagonal weight with which the object
 *                        adjoint spreads |probe|^2: with A[t][iy][ix] = sum_m |probe[t][m][iy][ix]|^2 (probe complex64
 *                        [ptheta][nmodes][nprb][nprb]) and position j of scan (float32 [ptheta][nscan][2], row first)
 *                        split by modff into (sy, sx) + (fy, fx), out[t][sy+iy+a][sx+ix+b] += w_ab A[t][iy][ix] for a, b
 *                        in {0, 1}, w_00 = (1-fx)(1-fy), w_01 = fx (1-fy), w_10 = (1-fx) fy, w_11 = fx fy.  A position
 *                        with a negative integer part, a non-finite value or a value >= 1e9 is skipped; taps outside the
 *                        object are dropped, the others kept.  One launch; per pixel the positions are added in index
 *                        order, taps in the order above, in float32.
 *   ptycho_gauge_fit     gauge (float64 [ptheta][6]) <- (gy, gx, phi0, s, yc, xc) per angle of psi (complex64
 *                        [ptheta][nz][n]) against ref (same shape; NULL: u = psi) under weight (float32, >= 0, same
 *                        shape; NULL: all ones), all sums in float64, u = psi conj(ref):
 *                          gx = arg sum_{y, x<n-1} w[y][x] w[y][x+1] u[y][x+1] conj(u[y][x]), gy the same along y
 *                          (arg 0 = 0; valid for |g| < pi rad / pixel);  W = sum w, yc = sum w y / W, xc = sum w x / W;
 *                          phi0 = arg sum w u exp(-i (gy (y - yc) + gx (x - xc)));
 *                          s = sqrt(sum w |psi|^2 / sum w |ref|^2) (without ref: / W), 1 if either sum is 0.
 *                        W = 0 gives the identity (0, 0, 0, 1, 0, 0).  Pixels of weight 0 enter no sum, whatever they
 *                        hold.  work: float64 scratch of ptheta * PTYCHO_GAUGE_WORK_PER_ANGLE words.  Four launches (two
 *                        reduction passes, each followed by a one-workgroup-per-angle finish); the second pass reads
 *                        the first one's result from gauge on the device.
 *   ptycho_gauge_apply   in place on x (complex64 [ptheta][ny][nx]) with gauge (float64 [ptheta][6]):
 *                        which = 0, object: x *= exp(-i (phi0 + gy (y - yc) + gx (x - xc))) / s;
 *                        which = 1, probe companion: x *= s exp(+i (gy y + gx x)), local probe coordinates.
 *                        Both applied (which = 1 to every probe mode) multiply each position's exit wave by a constant
 *                        phase: the intensities stay (exactly at whole-pixel positions).  One launch.
 * PTYCHO_ERR_ARG, before any HIP call, for a null out / scan / probe / gauge / psi / work / x, a zero size, nmodes < 1,
 * which outside {0, 1}, ptheta > 65535 or a side too large for one launch (> 2^30; nz > 16 * 65535 for the illumination). */
#define PTYCHO_GAUGE_WORK_PER_ANGLE 16384
int ptycho_illumination(float* out, const void* scan, const void* probe, size_t ptheta, size_t nscan, int nmodes,
                        size_t nprb, size_t nz, size_t n, void* stream);
int ptycho_gauge_fit(double* gauge, const void* psi, const void* ref, const float* weight, size_t ptheta, size_t nz,
                     size_t n, double* work, void* stream);
int ptycho_gauge_apply(void* x, const double* gauge, size_t ptheta, size_t ny, size_t nx, int which, void* stream);

/* Fit residuals of a reconstruction per frame and per detector pixel (no handle; libtike.hipfft.fit): how well the
 * modelled intensity explains the data.  Every launch runs on `stream`, nothing synchronises, no float atomics and fixed
 * summation orders: the same inputs give the same bits.  ptheta in [1, 65535], nscan and npix below 2^31, ptheta *
 * nscan * npix at most 2^59.
 *   ptycho_fit_accumulate  inten (float32 [count]) = |g|^2 (add = 0) or += |g|^2 (add != 0), g complex64 [count],
 *                          |g|^2 = re * re + im * im in float32, each operation rounded (no fused multiply-add).  One launch.
 *   ptycho_fit_work_words  float64 words of scratch that ptycho_fit_frames needs (it may be 0: pass any non-null
 *                          pointer then); at most max(1 MiB, bytes of data / 4) / 8.  0 also for sizes out of range.
 *   ptycho_fit_frames      one pass over g (complex64 [ptheta][nscan][npix], the farplane of the last or only mode; may be
 *                          NULL), inten (float32, same shape, the summed intensity of the other modes; may be NULL, not
 *                          both) and data (float32, same shape), then a second launch that adds the partial sums left
 *                          in `work` in index order.  Per pixel, in float32: I = (inten ? inten : 0) + (g ? |g|^2 : 0),
 *                          I' = I * (float)((a/b) * (a/b)) with {a, b} = ab (float64 [2] on the device, as in
 *                          ptycho_cg_project; NULL: I' = I), d = data; square roots and logarithms are the hardware's
 *                          (1 ulp), ln x = ln 2 * log2 x.  mask: npix bytes shared by all frames, nonzero = measured, in
 *                          the layout of ptycho_set_mask's argument; NULL: every pixel is measured.  An unmeasured pixel
 *                          enters no sum, whatever data, g or inten hold there (NaN and Inf included: a select, not a
 *                          product); a non-finite value at a measured pixel propagates.
 *                          frames (float64 [ptheta][nscan][8], written in full): sums over the measured pixels of the
 *                          frame, terms in float32, accumulated in float64, of
 *                            0: I'   1: d   2: sqrt(I' d)   3: (sqrt I' - sqrt d)^2   4: I' - d ln(I' + 1e-32)
 *                            5: d - d ln(d + 1e-32)   6: |sqrt I' - sqrt d|   7: sqrt d
 *                          (2 and 0 summed over all frames are a and b of the probe rescale; 3 is the gaussian cost,
 *                          4 the poisson_ml cost as logged, 2 * (4 - 5) the Poisson deviance, 6 / 7 the amplitude
 *                          R-factor).  pixels (float64 [ptheta][4][npix], written in full; NULL: not wanted): sums over
 *                          the nscan frames of the angle in index order of
 *                            0: I'   1: d   2: sqrt I' - sqrt d (signed)   3: (sqrt I' - sqrt d)^2,
 *                          every map exactly 0 at an unmeasured pixel.  A frame's sums depend on that frame's values
 *                          alone; frames do not depend on whether pixels is asked for.
 * PTYCHO_ERR_ARG, before any HIP call, for a null inten / g (accumulate), a null frames / data / work, inten and g both
 * null, a zero size or sizes out of the range above. */
int ptycho_fit_accumulate(float* inten, const void* g, size_t count, int add, void* stream);
size_t ptycho_fit_work_words(size_t ptheta, size_t nscan, size_t npix);
int ptycho_fit_frames(double* frames, double* pixels, const float* inten, const void* g, const float* data,
                      const unsigned char* mask, const double* ab, size_t ptheta, size_t nscan, size_t npix,
                      double* work, void* stream);

/* Raw detector frames to the solver's data (no handle; libtike.hipfft.prepare): crop, bin, dark, gain, bad pixels, clip,
 * scale, ifftshift and statistics in one pass that reads every raw byte once, then a second launch that combines the
 * partial results left in `work` in index order.  Runs on `stream`, nothing synchronises, no atomics and fixed summation
 * orders: the same inputs give the same bits.
 *   raw    frames [ptheta][nraw][H][W], stored centred; dtype 0 uint16, 1 uint32, 2 int32, 3 float32.
 *   index  int64 [ptheta][nscan] on the device or NULL: output frame j reads raw frame index[t][j] (NULL: frame j, and
 *          nraw must equal nscan).  An index outside [0, nraw) gives an all-zero frame and four zero statistics; nothing
 *          is read out of bounds for it.
 *   dark, gain  float32 [H][W] or NULL (0 and 1).  bad: uint8 [H][W] or NULL, nonzero = bad.
 *   y0, x0 raw row and column of the first pixel of the crop window; they may be negative or leave part of the window
 *          outside the frame.  bin: 1, 2 or 4.  ndet: any size in [1, 32768].
 * Centred pixel (oy, ox) covers the raw pixels (y0 + oy bin + by, x0 + ox bin + bx), by, bx < bin.  It is MEASURED if all
 * of them lie inside the frame and none is bad (the same for every frame).  In float32, every operation rounded (no
 * fused multiply-add): t = ((float)raw - dark) * gain per raw pixel; v = sum of t in the order by outer, bx inner from
 * the first term; clip != 0: v = v < 0 ? 0 : v (a NaN stays); v = v * scale; an unmeasured pixel gets v = 0 by a select,
 * whatever raw, dark and gain hold there (NaN and Inf included).  A non-finite value at a measured pixel reaches that
 * pixel and that frame's sums only.
 *   data   float32 [ptheta][nscan][ndet][ndet] in the operators' layout: data[r][c] = v[(r + ndet/2) % ndet][(c + ndet/2)
 *          % ndet] (ifftshift: centred pixel ndet/2 lands at [0][0]; for even ndet this is also fftshift).
 *   mask   uint8 [ndet][ndet], same layout, 1 = measured: the argument of ptycho_set_mask.
 *   frames float64 [ptheta][nscan][4], over the measured pixels of the frame: 0 sum of v, 1 sum of v * v (the product
 *          rounded in float32, both sums accumulated in float64), 2 max of v (fmaxf from -inf: a NaN is skipped; -inf
 *          without a measured pixel), 3 the number of raw pixels of measured bins with (float)raw >= saturation (a NaN
 *          saturation disables the count).
 *   pixels float64 [ptheta][4][ndet][ndet] or NULL, layout of data: the same four over the frames of the angle whose
 *          index is in range; map 3 counts the frames in which any raw pixel of the bin was saturated; every map is 0
 *          at an unmeasured pixel.
 *   work   float64 scratch of ptycho_prepare_work_words(ptheta, nscan, ndet * ndet) words (it may be 0: pass any
 *          non-null pointer then; 0 also for sizes out of range).
 * PTYCHO_ERR_ARG, before any HIP call, for a null data / mask / frames / raw / work, a zero size, bin outside {1, 2, 4},
 * an unknown dtype, ptheta > 65535, index NULL with nraw != nscan, ndet > 32768, nraw or nscan or H * W at or above 2^31,
 * |y0| or |x0| above 2^30, or more than 2^59 elements of raw or data. */
size_t ptycho_prepare_work_words(size_t ptheta, size_t nscan, size_t npix);
int ptycho_prepare_frames(float* data, unsigned char* mask, double* frames, double* pixels, const void* raw, int dtype,
                          const long long* index, const float* dark, const float* gain, const unsigned char* bad,
                          size_t ptheta, size_t nraw, size_t nscan, size_t H, size_t W, long long y0, long long x0,
                          int bin, size_t ndet, float saturation, float scale, int clip, double* work, void* stream);

/* Weighted least-squares phase unwrapping (no handle; libtike.hipfft.unwrap): Jacobi-preconditioned conjugate gradients
 * on the pixel grid (Ghiglia & Romero 1994).  Every launch runs on `stream`, nothing synchronises, no float atomics and
 * fixed summation orders: the same inputs give the same bits.  ptheta in [1, 65535], nz >= 2, n >= 2, nz * n < 2^31.
 * Per angle: phase phi and weight w are float32 [nz][n] (weight NULL: all ones).  w' = w where w > 0 and finite, else 0 (a
 * select).  W(a) = a - 2 pi rint(a / 2 pi) in float32.  The edge between neighbours p -> q (q to the right of or below
 * p) has weight w_e = min(w'_p, w'_q) and difference d_e = W(phi_q - phi_p); an edge of weight 0 contributes exactly 0 to
 * everything, whatever phi holds at its ends.  The solver minimises sum_e w_e (x_q - x_p - d_e)^2, i.e. L x = b with
 * (L x)_p = sum_{e at p} w_e (x_p - x_other), b_p = sum_{e into p} w_e d_e - sum_{e out of p} w_e d_e, D_p = sum_{e at p}
 * w_e and the preconditioner 1 / D (0 where D = 0), from x = 0.  Arrays are float32; every dot product, alpha, beta and the
 * stopping tests are float64.
 *   state   float64 [ptheta][PTYCHO_UNWRAP_STATE_WORDS]: rz0, rz, p.q, alpha, beta, iterations, status (0 running,
 *           1 converged: rz <= tol^2 rz0, rz0 = 0 included; 2 breakdown: p.q <= 0 or not finite, x stays as it is;
 *           3 maxiter), relres = sqrt(rz / rz0), c; the rest is zero.
 *   buf     float32 scratch of ptycho_unwrap_buffer_floats words: per angle the planes x, r, p, p', q, 1 / D.
 *   work    float64 scratch of ptycho_unwrap_work_words words (both 0 for sizes out of range).
 *   ptycho_unwrap_begin     b -> r, 1 / D, x = 0, p = r / D, rz0; state is initialised.  Two launches.
 *   ptycho_unwrap_iterate   enqueues niter iterations (q = L p, alpha = rz / p.q, x += alpha p, r -= alpha q, z = r / D,
 *                           rz' = r.z, p = z + (rz' / rz) p), four launches each, and one more that applies the stopping
 *                           tests; the launches of an angle that has stopped return at once, and no angle runs past
 *                           maxiter however many iterations are enqueued.  weight: as given to begin.
 *   ptycho_unwrap_finish    c = arg sum w' [D > 0] exp(i (phi - x)) (arg 0 = 0) -> state; congruent != 0:
 *                           out = phi + 2 pi rint((x + c - phi) / 2 pi), formed in float64 and rounded once;
 *                           congruent = 0: out = x + c; out = phi where D = 0.  Three launches.
 *   ptycho_unwrap_residues  charge (int8 [ptheta][nz-1][n-1], or NULL) <- for the loop with corner (y, x),
 *                           rint((W(phi[y][x+1] - phi[y][x]) + W(phi[y+1][x+1] - phi[y][x+1]) + W(phi[y+1][x] -
 *                           phi[y+1][x+1]) + W(phi[y][x] - phi[y+1][x])) / 2 pi) if all four pixels have w' > 0, else 0;
 *                           count (int64 [ptheta]) <- the number of loops of charge +-1.  A memset and one launch.
 * PTYCHO_ERR_ARG, before any HIP call, for a null buf / state / phase / work / out / count, nz < 2 or n < 2,
 * nz * n >= 2^31, ptheta outside [1, 65535], niter < 0, maxiter < 0, or a tol that is negative or not finite. */
#define PTYCHO_UNWRAP_STATE_WORDS 16
size_t ptycho_unwrap_work_words(size_t ptheta, size_t nz, size_t n);
size_t ptycho_unwrap_buffer_floats(size_t ptheta, size_t nz, size_t n);
int ptycho_unwrap_begin(float* buf, double* state, const float* phase, const float* weight, size_t ptheta, size_t nz,
                        size_t n, double* work, void* stream);
int ptycho_unwrap_iterate(float* buf, double* state, const float* weight, size_t ptheta, size_t nz, size_t n, int niter,
                          int maxiter, double tol, double* work, void* stream);
int ptycho_unwrap_finish(float* out, double* state, const float* buf, const float* phase, const float* weight,
                         int congruent, size_t ptheta, size_t nz, size_t n, double* work, void* stream);
int ptycho_unwrap_residues(signed char* charge, long long* count, const float* phase, const float* weight, size_t ptheta,
                           size_t nz, size_t n, void* stream);

/* A first look at a scan before any reconstruction (no handle; libtike.hipfft.dpc): the moments of every diffraction
 * pattern, per-position values spread over the object grid, and the integration of a gradient field.  Every launch runs on
 * `stream`, nothing synchronises, no float atomics and fixed summation orders: the same inputs give the same bits.
 *   ptycho_frame_moments_work_words  float64 words of scratch that ptycho_frame_moments needs (it may be 0: pass any
 *                          non-null pointer then; 0 also for sizes out of range).
 *   ptycho_frame_moments   one pass over data (float32 [ptheta][nscan][ndet][ndet], DC at [0][0], any ndet >= 1).  mask:
 *                          ndet^2 bytes in the layout of data, nonzero = measured, or NULL; an unmeasured pixel is given
 *                          I = 0 by a select, so what data holds there never matters; a non-finite value at a measured
 *                          pixel stays in its frame.  With k(r) = r for r < ndet - ndet / 2, else r - ndet (the signed
 *                          frequency index), moments (float64 [ptheta][nscan][8]) <- the sums over the pixels (y, x) of a
 *                          frame of
 *                            0  I          3  k(y)^2 I       6  I where k(y)^2 + k(x)^2 > darkfield^2
 *                            1  k(y) I     4  k(x)^2 I          (0 for a negative darkfield)
 *                            2  k(x) I     5  k(y) k(x) I    7  0
 *                          each term formed as (double) I times the integer factor and added in float64.  16-byte loads
 *                          when ndet^2 is a multiple of 4 and data is 16-byte aligned, scalar ones otherwise: the same
 *                          bits.  Two launches (one when the detector has at most 512 pixels).
 *   ptycho_scan_map        values: float32 [ptheta][nscan][nval], nval in [1, 4]; keep: uint8 [ptheta][nscan], a zero byte
 *                          excludes the position, or NULL; scan, probe, nmodes, nprb, nz, n as for ptycho_illumination.
 *                          weight (float32 [ptheta][nz][n]) <- ptycho_illumination of the kept positions in their order,
 *                          formed by the same kernel: the same bits.  With A, the split (sy, sx) + (fy, fx) and the taps
 *                          w_ab of ptycho_illumination, num_c[sy+iy+a][sx+ix+b] += (w_ab A[iy][ix]) v_j[c] over the
 *                          positions in order and the taps in the order (0,0) (0,1) (1,0) (1,1), A = sum_m (re^2 + im^2),
 *                          every operation rounded to float32 (no fused multiply-add), and out (float32
 *                          [ptheta][nval][nz][n]) <- num_c / weight where weight > 0, else 0 (raw != 0: num_c itself, which
 *                          is 0 where weight is).  Both are written in full.
 *                          A position that the illumination skips or that keep excludes adds to nothing, whatever its
 *                          values hold.  work: float32 scratch of 2 ptheta nscan words, needed (non-null) only with keep.
 *                          Two launches, three with keep.
 *   ptycho_integrate_begin   ptycho_unwrap_begin with one change: the difference of the edge p -> q is not the wrapped
 *                          phase difference but d_e = (gx_p + gx_q) / 2 if q is to the right of p, (gy_p + gy_q) / 2 if q
 *                          is below p, in float32 with both operations rounded (gy, gx: float32 [ptheta][nz][n], the
 *                          gradient in units per pixel along rows' index and columns' index).  Edge weights, b, D, 1 / D,
 *                          buf, state and work are the unwrapper's, and what gy and gx hold at a pixel of weight 0 never
 *                          matters.  Iterate with ptycho_unwrap_iterate.  Two launches.
 *   ptycho_integrate_finish  c = sum w' [D > 0] x / sum w' [D > 0] in float64 (0 for an empty sum) -> state;
 *                          out = x - c, formed in float64 and rounded once, where D > 0, else 0.  Three launches.
 * PTYCHO_ERR_ARG, before any HIP call, for a null moments / data / work / weight / out / values / scan / probe / buf /
 * state / gy / gx, a null work of ptycho_scan_map with keep, a zero size, nval outside [1, 4], nmodes < 1, a darkfield that
 * is NaN or +Inf, and the size limits of ptycho_fit_frames (npix = ndet^2 <= 2^31 - 1), ptycho_illumination and
 * ptycho_unwrap_begin. */
size_t ptycho_frame_moments_work_words(size_t ptheta, size_t nscan, size_t ndet);
int ptycho_frame_moments(double* moments, const float* data, const unsigned char* mask, double darkfield, size_t ptheta,
                         size_t nscan, size_t ndet, double* work, void* stream);
int ptycho_scan_map(float* weight, float* out, const float* values, const unsigned char* keep, const void* scan,
                    const void* probe, size_t ptheta, size_t nscan, int nval, int nmodes, size_t nprb, size_t nz, size_t n,
                    int raw, float* work, void* stream);
int ptycho_integrate_begin(float* buf, double* state, const float* gy, const float* gx, const float* weight, size_t ptheta,
                           size_t nz, size_t n, double* work, void* stream);
int ptycho_integrate_finish(float* out, double* state, const float* buf, const float* weight, size_t ptheta, size_t nz,
                            size_t n, double* work, void* stream);

/* Free-space propagation of square complex fields and the figures of a focus series (libtike.hipfft.propagate).  h is
 * a handle whose ndet is the side S of the fields, as for ptycho_fft2; it supplies the twiddle table and nothing of it is
 * changed.  Any side ptycho_fft2 takes from 16 up: 16 <= S <= 1024, or 2048.  Everything runs on `stream`, nothing
 * synchronises, no float atomics and fixed summation orders: the same inputs on the same path give the same bits.
 * A field u is complex64 [S][S] in image layout; nothing is shifted: spec is its UNNORMALISED forward DFT
 * (ptycho_fft2, dir = -1) with DC at [0][0], and H is indexed the same way.  With k = fftfreq(S) S the integer
 * frequencies, k2 = ky^2 + kx^2, q = q0 k2 (q0 = (lambda / (S p))^2, p the pixel size of the field's plane) and
 * zl = z / lambda, all float64, the transfer function in turns is
 *   method 0, Fresnel (paraxial):                     t = -zl q / 2,                |H| = 1;
 *   method 1, angular spectrum, carrier removed:      t = -zl q / (1 + sqrt(1 - q)) for q <= 1 (the cancellation-free
 *                                                     form of zl (sqrt(1 - q) - 1)), |H| = 1; H = 0 for q > 1
 *                                                     (evanescent), whatever the sign of z.
 * t -= rint(t) in float64 (zl q reaches 1e7 turns and more), H = exp(2 pi i t) by sincospi(2 t) in float64, times 1 / S^2,
 * rounded once to float32; every product and sum that forms t is rounded on its own (no fused multiply-add).
 *   plane[f][d] = IDFT(spec[f] H_d)       (complex64; z = 0 gives u back; the convolution is circular: padding is the
 *                                          caller's)
 *   metrics[f][d][8] (float64), with v = |plane|^2 formed in float32 as round(round(re re) + round(im im)), converted to
 *   double, and y, x the pixel indices 0 ... S - 1:
 *       { sum v, sum v^2, sum v y, sum v x, sum v y^2, sum v x^2, max v, flat index y S + x of the first maximum }.
 *   A NaN v is skipped by the max, as in ptycho_prepare_frames, and propagates into the sums; if no v compares, the max
 *   is -inf and the index -1.  Of equal maxima the one with the lowest index counts.
 * Arguments: spec complex64 [nfield][S][S]; zl float64 [nplane] ON THE DEVICE; planes complex64 [nfield][nplane][S][S]
 * or NULL; metrics float64 [nfield][nplane][8] or NULL (not both NULL); work float64 scratch of
 * ptycho_propagate_work_words(h, nfield, nplane, planes != NULL) words -- the count may be 0: pass any non-null pointer
 * then; it is 0 for sizes out of range.
 * Two paths, chosen as ptycho_fft2 chooses.  Sides with a plan whose tile fits a compute unit's LDS (16, 32, 48, 64, 80,
 * 96, 112, 128) with option "tile" on: ONE launch, the spectrum times H_d, both inverse passes and the figures of a pair
 * (f, d) stay on the compute unit, and a plane is written only if planes is given; no scratch.  Every other side, and those
 * sides with "tile" off: spec H_d into planes (or into work when planes is NULL), the in-place inverse transform of
 * ptycho_fft2, and one workgroup per pair for the figures.  The two paths add in different orders: their sums agree to
 * rounding, their maxima and indices exactly when their planes do.
 * PTYCHO_ERR_ARG, before any HIP call, for a null or freed handle, a null spec / zl / work, planes and metrics both
 * null, S < 16 (or S = 1025 ... 2047), nfield or nplane zero, nfield * nplane >= 2^30, a method other than 0 and 1, a q0
 * that is negative or not finite, spec or planes not 16-byte aligned. */
size_t ptycho_propagate_work_words(ptycho_handle h, size_t nfield, size_t nplane, int planes_wanted);
int ptycho_propagate(ptycho_handle h, void* planes, double* metrics, const void* spec, size_t nfield, const double* zl,
                     size_t nplane, double q0, int method, void* work, void* stream);

/* B-spline resampling of images (no handle; libtike.hipfft.resample): the prefilter, the affine warp and the moments
 * behind a centre of mass.  Everything runs on `stream`, nothing synchronises, no atomics and fixed summation orders: the
 * same inputs give the same bits.  An image is [ny][nx] of float32 (cplx = 0) or complex64 (cplx != 0, real and imaginary
 * part treated alike); nimg in [1, 65535], 2 <= ny, nx <= 65536, ny * nx < 2^31.  Interpolation is by B-splines of order
 * 0 ... 5 as scipy.ndimage does it, with MIRROR extension: whole-sample symmetric, period 2 n - 2, refl(i) the index in
 * [0, n) that i reflects to.
 *   ptycho_spline_prefilter   out <- the B-spline coefficients of in along both axes (orders 0 and 1: a copy).  Per axis
 *       and pole z (order 2: sqrt 8 - 3; 3: sqrt 3 - 2; 4: -0.36134, -0.013725; 5: -0.43058, -0.043096, closed forms in
 *       float64, rounded to float32), after multiplication by the gain prod (1 - z)(1 - 1 / z):
 *       c+[0] = sum over the mirrored line of z^|k| x[k], c+[k] = x[k] + z c+[k-1],
 *       c[n-1] = (z c+[n-2] + c+[n-1]) z / (z^2 - 1), c[k] = z (c[k+1] - c+[k]); two poles cascade.  This is
 *       scipy.ndimage.spline_filter(mode="mirror").  A line is cut into segments of PTYCHO_SPLINE_SEGMENT samples; a
 *       segment is filtered over itself and a halo of 12 / 16 / 28 / 32 samples (orders 2 ... 5) on either side, exactly
 *       where that range touches an end of the line and from zero state elsewhere, which is off by at most 1e-9 of the
 *       line's largest value.  Arithmetic is float32.  Columns first (in -> work), then rows (work -> out): out may be
 *       in.  work: ptycho_spline_work_words float64 words (0 for sizes out of range), neither out nor in.  16-byte
 *       accesses when nx * (cplx ? 2 : 1) is a multiple of 4 and out, in and work are 16-byte aligned.  Two launches.
 *   ptycho_warp   out[i] (oh x ow) <- coef[i] (ny x nx, coefficients of ptycho_spline_prefilter) under the affine map
 *       xf[i] = (m00, m01, m10, m11, offy, offx), float64 ON THE DEVICE: output pixel (oy, ox) has the source coordinate
 *       sy = (m00 oy + m01 ox) + offy, sx = (m10 oy + m11 ox) + offx in float64, every operation rounded on its own
 *       (the geometry of scipy.ndimage.affine_transform).  Per axis the first tap is b = floor(s) - order / 2 for odd and
 *       floor(s + 1/2) - order / 2 for even orders, t = s - floor(.) in float32, and the value is
 *       sum_a wy[a] (sum_b wx[b] coef[refl(by + a)][refl(bx + b)]) in float32, w the centred cardinal B-spline at
 *       t + order / 2 - a.  flags: PTYCHO_WARP_MIRROR evaluates every pixel (a coordinate beyond 2^30 in magnitude or
 *       not finite still gives cval); without it a coordinate within 2^-20 of the extent [0, ny-1] x [0, nx-1] is clamped
 *       onto it and a pixel outside gets (cval_re, cval_im).  A 32 x 32 output tile stages the box of coefficients that its
 *       taps touch in LDS when the box holds at most 4096 elements and reads global memory otherwise (strong
 *       minification); PTYCHO_WARP_GLOBAL forces the latter; both give the same bits.  path: NULL, or int32
 *       [nimg][ceil(oh / 32)][ceil(ow / 32)] that receives per tile 0 (wholly outside: cval, nothing loaded), 1 (LDS) or
 *       2 (global).  out must not be coef.  One launch.
 *   ptycho_moments   sums (float64 [nimg][5]) <- sum w, sum w y, sum w x, sum w y^2, sum w x^2 over the pixels (y, x) of
 *       each image, in float64.  w is float32: which = 0 the value, 1 its positive part, 2 its square, for a complex
 *       image (which = 2 only) round(round(re re) + round(im im)); times weight (float32 [nimg][ny][nx]) if not NULL,
 *       rounded once.  work: ptycho_moments_work_words float64 words (0 for sizes out of range).  Two launches.
 * PTYCHO_ERR_ARG, before any HIP call, for a null out / in / work / coef / xf / sums / x, nimg outside [1, 65535], a side
 * below 2 or above 65536, ny * nx >= 2^31, an output side of 0 or above 65536, oh * ow >= 2^31, an order outside
 * [0, 5], unknown flags, work equal to out or in, out equal to coef, which outside [0, 2], a complex image with which != 2. */
#define PTYCHO_SPLINE_SEGMENT 64
#define PTYCHO_WARP_MIRROR 1
#define PTYCHO_WARP_GLOBAL 2
size_t ptycho_spline_work_words(size_t nimg, size_t ny, size_t nx, int cplx);
int ptycho_spline_prefilter(void* out, const void* in, size_t nimg, size_t ny, size_t nx, int cplx, int order, void* work,
                            void* stream);
int ptycho_warp(void* out, const void* coef, const double* xf, size_t nimg, size_t ny, size_t nx, size_t oh, size_t ow,
                int cplx, int order, int flags, float cval_re, float cval_im, int* path, void* stream);
size_t ptycho_moments_work_words(size_t nimg, size_t ny, size_t nx);
int ptycho_moments(double* sums, const void* x, const float* weight, size_t nimg, size_t ny, size_t nx, int cplx, int which,
                   double* work, void* stream);

/* ---- fused CG-stage entry points ("plus fused CG-stage entry points") ----
 * The elementwise stages of CGPtychoSolver.run (src/libtike/cufft/ptycho.py:325-393) are
 * fused into the row pass of the DFT so that farplanes are never materialised.  The
 * handle owns work buffers ("slots" 0..15, one farplane each, allocated on first use; the
 * single-mode loop uses 0 and 1, the multi-mode loop one pair (2k, 2k+1) per probe mode)
 * that hold column-pass intermediates between calls.  sums/cost/costs and ab are DEVICE
 * pointers to float64 (ab = {a, b} of ptycho.py:342-343; NULL means scale 1); the
 * kernels ADD into sums/cost/costs, the caller zeroes them.  Every such sum is formed in a fixed order (per-workgroup
 * partials, folded by the last workgroup to finish): the same inputs give the same bits, whatever the scheduling.
 *   ptycho_cg_fwd_cols   slot <- column pass of fwd(f, scan, prb)            (ptycho.py:332)
 *   ptycho_cg_stats      sums += { sum sqrt(|g|^2 d), sum |g|^2 }            (ptycho.py:333,342-343)
 *   ptycho_cg_project    dst  <- IDFT_x( fpsi - sqrt(d) fpsi / (sqrt(I)+1e-32) ), cost += ||sqrt I - sqrt d||^2
 *                                                                             (ptycho.py:344-353,310)
 *   ptycho_cg_adj_cols   column pass of adj from a slot into f (flg 0) / prb (flg 1) (ptycho.py:352,429)
 *   ptycho_cg_linesearch costs[j] += f(p1 + y_j^2 p2 + y_j p3), y_j = gamma0 2^-j, j < ncand <= 16;
 *                        costs[ncand] += f(p1); p1,p2,p3 from slot1 (scaled by a/b) and slot2
 *                                                                             (ptycho.py:383-393,253-281) */
int ptycho_cg_fwd_cols(ptycho_handle h, int slot, const void* f, const void* scan,
                       const void* prb, void* stream);
/* Measured-pixel mask of the CG stages.  mask: DEVICE array of ndet * ndet bytes in the layout of data (un-fftshifted,
 * DC at [0, 0]), nonzero = measured; NULL clears the mask.  The handle packs it into a buffer of its own (freed by
 * ptycho_free; the caller's array may go once this returns) and checks it on the host (one synchronisation of `stream`).
 * While a mask is set, every ptycho_cg_* stage that reads data -- stats, project, project_multi, linesearch,
 * intensity_modes (sums), linesearch_modes and the native object / probe / line-search stages built on them -- sums
 * over measured pixels only: data, the intensity and the line-search terms count as 0 at an unmeasured pixel, whatever
 * data holds there (NaN and Inf included), and the projected residual is 0 there.  An all-ones mask gives the bits of
 * no mask.  ptycho_fwd / adj / fft2, ptycho_cg_cross / argmax / zoom do not use it.
 * PTYCHO_ERR_ARG: a mask with no measured pixel (a / b would be 0 / 0), or a detector size without a Stockham plan
 * (those sizes have no fused CG stages). */
int ptycho_set_mask(ptycho_handle h, const void* mask, void* stream);
int ptycho_cg_stats(ptycho_handle h, int slot, const void* data, double* sums, void* stream);
int ptycho_cg_project(ptycho_handle h, int src_slot, int dst_slot, const void* data,
                      const double* ab, double* cost, void* stream);
int ptycho_cg_adj_cols(ptycho_handle h, int slot, void* f, const void* scan, void* prb,
                       int flg, void* stream);
int ptycho_cg_linesearch(ptycho_handle h, int slot1, int slot2, const void* data,
                         const double* ab, double gamma0, int ncand, double* costs,
                         void* stream);

/* Multi-mode variants (ptycho.py:330-333,349-356,386-391,425-434 loop over probe modes):
 * the summed intensity is a float32 array [ptheta][nscan][ndet][ndet] owned by the caller;
 * each mode k has its own pair of work slots (2k, 2k+1).
 *   ptycho_cg_intensity_modes  inten = sum_k |g_k|^2 over the slots 2k, k < nmodes (inten may be NULL), and,
 *                              if sums is given, sums += { sum sqrt(inten d), sum inten }: one pass
 *   ptycho_cg_project_multi    as ptycho_cg_project with I = inten * (a/b)^2; slot_unscaled = 0: the slot was
 *                              made with the rescaled probe, 1: with the probe before its rescale
 *   ptycho_cg_linesearch_modes as ptycho_cg_linesearch with p1,p2,p3 summed in registers over the mode
 *                              pairs (slot 2k, slot 2k+1), mode0 <= k < mode0 + nmodes <= 8 (no arrays); p1 = inten if given
 */
int ptycho_cg_intensity_modes(ptycho_handle h, int nmodes, void* inten, const void* data, double* sums,
                              void* stream);
int ptycho_cg_project_multi(ptycho_handle h, int src_slot, int dst_slot, const void* data,
                            const void* inten, const double* ab, int slot_unscaled, double* cost,
                            void* stream);
int ptycho_cg_linesearch_modes(ptycho_handle h, int mode0, int nmodes, const void* data, const void* inten,
                               const double* ab, double gamma0, int ncand, double* costs,
                               void* stream);

/* Compact multi-mode layout (option "compact_modes" = M): mode k keeps its forward column pass in slot k and ALL
 * modes share one further slot M (projected residual of one mode at a time; direction column passes), M + 1
 * farplanes instead of 2 M.  The object line search (ptycho.py:383-393) needs fwd(dpsi, probe_k) of every mode at
 * once, so it runs over M equal ranges ("chunks") of positions: for chunk c the M direction column passes of
 * those positions go side by side into the shared slot and one line-search pass adds the chunk's costs -- the
 * same work as before in M smaller launches.  The option also makes the position order chunk-major.
 *   ptycho_cg_fwd_cols_modes   column passes of fwd(f, scan, prbs[k]) for nmodes modes (mode0 ...), the object
 *                              patch gathered once per position for up to four modes per launch (ptycho.py:330-333
 *                              gathers per mode); into_b = 0: into the modes' own slots, all positions;
 *                              into_b = 1 (compact layout, all modes): the positions of `chunk` into the shared slot
 *   ptycho_cg_linesearch_chunk costs += line-search costs of chunk `chunk` (pairs: slot k, shared slot part k) */
int ptycho_cg_fwd_cols_modes(ptycho_handle h, int nmodes, int mode0, const void* f, const void* scan,
                             const void* const* prbs, int into_b, int chunk, void* stream);
int ptycho_cg_linesearch_chunk(ptycho_handle h, int chunk, const void* data, const double* ab, double gamma0,
                               int ncand, double* costs, void* stream);

/* Position correction (ptycho.py:398-403 + 198-207), fused: with the column passes of
 * fwd(psi, 1) in slot1 and fwd(dpsi, 1) in slot2,
 *   ptycho_cg_cross   image_product = u1 conj(u2), u2 = u1 + gamma G dpsi (complex64
 *                     [ptheta][nscan][ndet][ndet], kept for the zoomed DFT); slot2 <- IDFT_x(product)
 *   ptycho_cg_argmax  IDFT_y of the slot, |.|, first maximum per position as
 *                     best[p] = (float bits of the value << 32) | (0xffffffff - flat index) */
/* image_product = NULL (here and in ptycho_cg_zoom): the product is kept in work slot 2 instead of a caller buffer */
int ptycho_cg_cross(ptycho_handle h, int slot1, int slot2, double gamma, void* image_product,
                    void* stream);
int ptycho_cg_argmax(ptycho_handle h, int slot, void* best, void* stream);

/* Sub-pixel stage of the registration (ptycho.py:209-235): from the whole-pixel peaks
 * (best = output of ptycho_cg_argmax; only the low word, 0xffffffff - flat index, is read)
 * wrap the peak to [-ndet/2, ndet/2), then evaluate the zoomed matrix DFT of the image
 * product on an ups x ups window around it (ups = ceil(1.5 upsample_factor)),
 *   cross[i,j2,j1] = sum_p sum_k e^{+i th_p (j2 - offy_i)} e^{+i th_k (j1 - offx_i)} ip[i,p,k],
 *   th = 2 pi fftfreq(ndet, upsample_factor),  off = fix(ups/2) - shift upsample_factor,
 * take the first maximum of |cross[i]| and return
 *   shifts[i] = shift + (argmax - fix(ups/2)) / upsample_factor     (float64 [ptheta*nscan][2]).
 * The centred window kernel K[j,k] = exp(+i th_k (j - (ups-1)/2)) is passed as real low-rank
 * factors  K = sum_{r<nc} lz[j,r] vt[k,r] + i sum_{r>=nc} lz[j,r] vt[k,r],
 * vt: float64 [ndet][16], lz: float64 [ups][16] (cos terms first, then sin terms).
 * Needs ndet % 16 == 0, ndet <= 1024, ups <= max(256, ndet). */
int ptycho_cg_zoom(ptycho_handle h, const void* image_product, const void* best, const void* vt,
                   const void* lz, int nc, int ups, double upsample_factor, void* shifts,
                   void* stream);

/* ---- device-resident CG iteration (native sequencing of ptycho.py:325-465) -----------------------
 * The reference decides every line-search trial on the host and runs the object- / probe-sized
 * stages (probe rescale, gradient normalisation, Dai-Yuan direction, updates) as dozens of small
 * array kernels per iteration.  Here they are HIP kernels driven by a float64 STATE vector that
 * lives on the device (owned by the caller, PTYCHO_CG_STATE_WORDS doubles, zero-initialised once),
 * and an iteration is issued as a few stage calls with no device synchronisation.  Between the
 * stages a multi-GPU caller all-reduces (sum) the words / arrays named below; a single-GPU caller
 * just calls them back to back.  One probe mode, gaussian model, ptheta = 1 for the position step.
 *
 *   ptycho_cg_obj_begin   slot 0 <- column pass of fwd(psi, probe); state[A,B] <- statistics (stored, like every sum of
 *                         the native stages: the state needs no zero fill) (ptycho.py:330-343).
 *                                                                    all-reduce: state[PTYCHO_ST_A .. +2)
 *   ptycho_cg_obj_grad    probe *= a/b (:344) and state[MAX_PRB] <- max|probe| in one pass; slot 1 <- projected residual,
 *                         state[COST] <- cost (:347-353); grad <- adj (raw, not yet divided by max|probe|^2; stored, no
 *                         zero fill needed with the deterministic adjoints).   all-reduce: grad
 *                         Option "defer_finish" (single GPU): grad stays in the adjoint's fixed-point image and
 *                         ptycho_cg_obj_dir folds it in -- do not read grad between the two calls; a deterministic
 *                         adjoint (ptycho_adj, ptycho_cg_adj_cols, ptycho_cg_prb_grad) issued in between fails with
 *                         PTYCHO_ERR_ARG instead of adding into the pending image.
 *   ptycho_cg_obj_dir     grad /= max|probe|^2 (:356); Dai-Yuan dpsi, grad0 <- grad (:366-373); slot 1 <- column
 *                         pass of fwd(dpsi, probe); first line-search pass (:383-393).
 *                                                                    all-reduce: state[PTYCHO_ST_COSTS .. +119)
 *                         Option "ls_fused_decide" (single GPU): every pass replays line_search_sqr on its own totals
 *                         in its last workgroup; ptycho_cg_ls_next(pass = 1, 2, 3) then only issues the next pass.
 *   ptycho_cg_ls_next     decide on the pass just reduced (line_search_sqr, :253-281); pass = 1, 2, 3: issue the next
 *                         pass (16, 32, 64 step lengths; each returns at once when the search is already
 *                         resolved) -> all-reduce state[COSTS..] again; pass = 4: decide only.  For a multi-GPU
 *                         caller, who pays a collective per pass: pass = 6 (issue 32) then 7 (issue the 80 that are
 *                         left) then 4 -- three collectives per search --, or pass = 5 (all 112 at once) then 4.  The accepted
 *                         step length times 0.5 lands in state[GAMMA_PSI] (which = 0) / state[GAMMA_PRB] (which = 1).
 *   ptycho_cg_reg_prepare (optional, multi-GPU) slot 2 <- column pass of fwd(psi, ones): the first operand of the position
 *                         correction depends on psi and scan only, so a caller that has to wait for the gradient
 *                         all-reduce anyway issues it in that gap; ptycho_cg_obj_finish then takes correct_positions = 2
 *   ptycho_cg_obj_finish  i > 0: position correction (:398-403; needs the zoom factors of ptycho_cg_zoom), scan[0] += shifts
 *                         (by the kernel that finds them; the next column pass re-sorts the positions);
 *                         psi += gamma dpsi (:405).  correct_positions: 0 off, 1 on, 2 on with slot 2 prepared, 3 on with slots 2 and 3 prepared
 *   ptycho_cg_prb_grad    slot 0 <- column pass of fwd(psi, probe); slot 1 <- projected residual (:421-430);
 *                         gprb <- adj_probe (raw).                   all-reduce: gprb
 *   ptycho_cg_prb_dir     gprb <- gprb / max|psi|^2 / nscan_total * nmodes (:431); Dai-Yuan dprb (:437-448);
 *                         slot 1 <- column pass of fwd(psi, dprb); first line-search pass (:451-461).
 *   ptycho_cg_prb_finish  probe += gamma dprb (:465)
 * state[PTYCHO_ST_LS_FAILED] counts failed line searches ("Line search failed for conjugate gradient."). */
enum {
    PTYCHO_ST_A = 0, PTYCHO_ST_B = 1,           /* sum sqrt(I d), sum I                       */
    PTYCHO_ST_COST = 2, PTYCHO_ST_COST2 = 3,    /* start-of-iteration cost; probe-step scratch */
    PTYCHO_ST_DY_OBJ = 4, PTYCHO_ST_DY_PRB = 7, /* 3 words each: ||g||^2, Re, Im sum conj(d)(g - g0) */
    PTYCHO_ST_MAX_PRB = 10, PTYCHO_ST_MAX_PSI = 11,   /* float bits of max|.| in the low half of the word */
    PTYCHO_ST_ZEROED = 12,                      /* (rounds 1-2: words [0, 12) were cleared by ptycho_cg_obj_begin; now every sum is stored) */
    PTYCHO_ST_GAMMA_PSI = 12, PTYCHO_ST_GAMMA_PRB = 13,
    PTYCHO_ST_LS_GAMMA0 = 14, PTYCHO_ST_LS_NCAND = 15, PTYCHO_ST_LS_NGROUPS = 16, PTYCHO_ST_LS_TRIED = 17,
    PTYCHO_ST_LS_RESOLVED = 18, PTYCHO_ST_LS_FAILED = 19,
    PTYCHO_ST_HINT = 20,                        /* [2] accepted index of the last object / probe search (seed with 14) */
    PTYCHO_ST_COSTS = 24,                       /* 7 groups x (16 step lengths + f(p1)) */
    PTYCHO_CG_STATE_WORDS = 160
};
int ptycho_cg_obj_begin(ptycho_handle h, double* state, const void* psi, const void* scan, const void* prb,
                        const void* data, void* stream);
/* obj_begin2 / obj_dir2: as obj_begin / obj_dir; with ones_prb != NULL the operands of the position correction ride along --
 * slot 2 <- column pass of fwd(psi, 1), slot 3 <- column pass of fwd(dpsi, 1) -- in the same launches, which gather the
 * object patch once for both probes; ptycho_cg_obj_finish then takes correct_positions = 3 (both prepared). */
int ptycho_cg_obj_begin2(ptycho_handle h, double* state, const void* psi, const void* scan, const void* prb,
                         const void* ones_prb, const void* data, void* stream);
int ptycho_cg_obj_dir2(ptycho_handle h, double* state, int first, const void* scan, const void* prb, const void* ones_prb,
                       const void* data, void* grad, void* grad0, void* dpsi, void* stream);
int ptycho_cg_obj_grad(ptycho_handle h, double* state, const void* scan, void* prb, const void* data, void* grad,
                       void* stream);
int ptycho_cg_obj_dir(ptycho_handle h, double* state, int first, const void* scan, const void* prb, const void* data,
                      void* grad, void* grad0, void* dpsi, void* stream);
int ptycho_cg_ls_next(ptycho_handle h, double* state, int which, int pass, const void* data, int use_ab, void* stream);
int ptycho_cg_reg_prepare(ptycho_handle h, double* state, const void* psi, const void* scan, const void* ones_prb, void* stream);
int ptycho_cg_obj_finish(ptycho_handle h, double* state, int correct_positions, void* psi, const void* dpsi, void* scan,
                         const void* ones_prb, const void* vt, const void* lz, int nc, int ups, double upsample_factor,
                         void* stream);
int ptycho_cg_prb_grad(ptycho_handle h, double* state, const void* psi, const void* scan, const void* prb,
                       const void* data, void* gprb, void* stream);
int ptycho_cg_prb_dir(ptycho_handle h, double* state, int first, double nscan_total, double nmodes, const void* psi,
                      const void* scan, const void* data, void* gprb, void* gprb0, void* dprb, void* stream);
int ptycho_cg_prb_finish(ptycho_handle h, double* state, void* prb, const void* dprb, void* stream);

/* Line searches of the multi-mode loop (compact slot layout) on the same device-resident state -- the host enqueues the
 * worst case and never reads a cost back (src/libtike/cufft/ptycho.py:274-276 synchronises once per trial):
 *   ptycho_cg_ls_begin      reset the search state of kind `which` (0 object, 1 probe); first pass sized from the last accepted index
 *   ptycho_cg_ls_obj_chunk  one chunk of an object-search pass: column passes of fwd(dpsi, prbs[k]) for the chunk's positions
 *                           (all modes, shared slot) + the line-search pass over them; chunk 0 stores the costs, the others add
 *                           (:383-393 with the sums over the modes of :386-391).  all-reduce after the last chunk: state[COSTS .. +119)
 *   ptycho_cg_ls_prb_pass   one pass of the probe search of mode `mode` (pair slot A(mode) / shared slot; p1 = inten) (:451-461)
 *   ptycho_cg_ls_decide     line_search_sqr on the costs of the pass (:253-281); next_groups = groups of 16 step lengths the
 *                           next pass prices (0: none follows).  Passes issued after the search is resolved return at once,
 *                           their column passes included.
 *   ptycho_cg_cross_dev     ptycho_cg_cross with gamma read from device memory (the accepted step never visits the host) */
int ptycho_cg_ls_begin(ptycho_handle h, double* state, int which, void* stream);
int ptycho_cg_ls_obj_chunk(ptycho_handle h, double* state, int chunk, const void* dpsi, const void* scan,
                           const void* const* prbs, const void* data, const double* ab, void* stream);
int ptycho_cg_ls_prb_pass(ptycho_handle h, double* state, int mode, const void* data, const void* inten, void* stream);
int ptycho_cg_ls_decide(ptycho_handle h, double* state, int which, int next_groups, void* stream);
int ptycho_cg_cross_dev(ptycho_handle h, int slot1, int slot2, const double* gamma_dev, void* image_product, void* stream);

/* Tuning knobs: "chunk" (positions per launch pair, 0 = default);
 * "window" (1 = LDS overlap-add object adjoint [default], 0 = direct atomics);
 * "trust_order" (1 = the caller vouches that the scan buffer passed to the next calls is the
 * same pointer with unchanged contents as in the previous call, so the position sort is
 * reused; set 0 after modifying scan; default 0);
 * "split" (ndet = 256: 1 = one radix-16 step of the DFT over y runs in the row pass [default]);
 * "tile" (ndet <= 128: 1 = forward operator and probe adjoint as ONE launch each, the tile stays in the CU's LDS and the
 * column<->row intermediate never reaches HBM [default]; 0 = the two-pass kernels of the larger sizes);
 * "deterministic" (1 = the adjoints add their per-workgroup sums into a 64-bit fixed-point image with integer
 * atomics and fold it into the output once: bitwise reproducible for a given chunk / run partition, one extra read of
 * g for the scale (none after ptycho_cg_project, which leaves max |slot| on the device); needs the windowed kernels
 * (powers of two up to 512, or any other size with nprb <= ~1000); default 0: float atomics, as kernels.cu:73-80,92-93);
 * "compact_modes" (M = number of probe modes: compact slot layout + chunk-major position order, see above; 0 = slot pairs);
 * "model" (likelihood of every stage that prices or projects against data: 0 = gaussian [default], 1 = poisson_ml; any
 * other value PTYCHO_ERR_ARG).  With 1, ptycho_cg_project / project_multi and the projections of the native object and
 * probe stages form the residual fpsi - d fpsi / (I' + 1e-32) and the cost sum I' - d ln(I' + 1e-32), and every
 * line-search pass (ptycho_cg_linesearch, _modes, _chunk, ls_obj_chunk, ls_prb_pass and the native searches) prices
 * sum |x| - d ln(|x| + 1e-32) for x = p1 + y^2 p2 + y p3.  The statistics of the probe rescale (a, b), the cross stage
 * and the operators do not depend on it.  The probe gradient of poisson_ml is not multiplied by the number of modes:
 * pass nmodes = 1 to ptycho_cg_prb_dir;
 * "defer_finish", "ls_fused_decide" (native CG stages on one GPU, see above; default 0);
 * "release_scratch" (any value: frees the adjoint's intermediate, which the fused CG stages never use; ptycho_adj re-allocates it);
 * "release_work" (value = slot: frees that CG work slot; the next stage that writes the slot allocates it again.  The native
 * loop with the position correction's shared gathers holds slots 0-3, without them 0-1 (+2 with a process group));
 * "trust_order" is the CALLER's: the native CG stages track the scan buffer themselves and do not touch it.
 * Experiments build only (make experiments, -DPTYCHO_EXPERIMENTS; the shipped library rejects / ignores them):
 * "fused" (ndet = 256: forward operator as ONE launch that keeps the column<->row intermediate on the CU,
 * k_fwd_fused256: 0 = off, 1 / 2 = one / two class tiles per pass; measured slower) and the
 * environment variables PTYCHO_HIP_CHUNK, PTYCHO_HIP_WINDOW, PTYCHO_HIP_SPLIT, PTYCHO_HIP_FUSED (initial values
 * of the options above), PTYCHO_HIP_NT (nontemporal load/store mask), PTYCHO_HIP_ROWGRID, PTYCHO_HIP_COLSEGS,
 * PTYCHO_HIP_MINSEG (launch geometry), PTYCHO_HIP_NMMAX, PTYCHO_HIP_ZOOM_SCALAR (zoomed DFT without the matrix cores). */
int ptycho_set_option(ptycho_handle h, const char* name, long long value);

/* In-library profiler for bench.py: when enabled, every kernel launch is
 * bracketed by HIP events on the caller's stream.  ptycho_profile_read waits for
 * the recorded launches, returns summed milliseconds and launch counts per kernel
 * (index 0 k_cols<FWD>, 1 k_rows<fwd>, 2 k_rows<inv>, 3 k_cols<ADJ_OBJ>,
 * 4 k_cols<ADJ_PRB>, 5 k_cols<PLAIN>, 6 position sort, 7 / 8 / 9 fused CG row passes (statistics / projection /
 * line search), 10 unused, 11 single-launch forward (experiments build), 12 unused, 13 cross row pass,
 * 14 arg-max column pass, 15 zoomed DFT + arg-max, 16 / 17 one-launch forward / probe adjoint of ndet <= 128; n >= 16:
 * arrays of 16 entries, as earlier versions of this header asked for, simply do not receive ids 16 / 17)
 * and clears the record.
 * No counterpart in the reference (it has no timing code). */
int ptycho_profile(ptycho_handle h, int enable);
int ptycho_profile_read(ptycho_handle h, double* ms, long long* launches, int n);

const char* ptycho_last_error(void);
const char* ptycho_version(void);

#ifdef __cplusplus
}
#endif
#endif
