// ptycho_kernels.hip -- the C ABI of include/ptycho_hip.h over the gfx950 kernels: one translation unit, one compile.
//
// What it replaces in the reference:
//   muloperator flg=2/0/1           src/cuda/kernels.cu:8-108
//   ptychofft ctor/fwd/adj/free     src/cuda/ptychofft.cu:5-88
//   cuFFT batched 2-D C2C           src/cuda/ptychofft.cu:14-20,72,85
//
// Structure: the 2-D DFT is split into a column pass and a row pass; the probe/object work is fused into
// the column pass, which owns a strip of C detector columns for a run of sorted scan positions and keeps the probe
// strip (or the probe-gradient accumulators) in registers across positions.
//
//   fwd : k_cols_gatherwin<FWD>  object rows cached in LDS -> bilerp * probe -> DFT over y -> strip of g
//         k_rows                 in-place DFT over x on g (zero columns are never read)
//   adj : k_rows                 inverse DFT over x, g -> chunk scratch (g untouched)
//         k_cols_adjreg / adjwin inverse DFT over y -> conj(probe) -> overlap-add window (registers at 256 / 512, else LDS) -> f   (object)
//         k_cols_gatherwin<ADJ_PRB>                  -> conj(patch) -> probe accumulators -> prb    (probe)
//   ndet <= 128: the tile fits a CU's LDS and both passes run in one launch (k_tile.hpp); ndet = 256: one radix-16 step
//   of the DFT over y moves into the row pass ("split"); k_cols<MODE> is the un-windowed path (option window = 0,
//   ndet > 512); sizes without a Stockham plan run Bluestein lines (k_generic.hpp).
//
// The adjoint's intermediate lives in a scratch of at most 4 GiB (one launch pair per chunk of positions; at
// 4096 x 256^2 that is a single pair).
//
// Reading order: ptycho_common.hpp first (arguments, and what the run-structured column kernels share: run bounds and
// decode, tile address, accumulate; run_split.hpp is the host's half of the run structure), then the kernel headers (k_*.hpp;
// k_rows.hpp opens with row_steps, the forward row transform that its fused CG stages, k_rows_split and the Bluestein lines of
// k_generic.hpp share, and holds TrialTerm, the line-search term of both likelihoods;
// frame_part.hpp before the analysis ones, which share its (frame, pixel) partition, fold and block sum), then
// the host side by topic -- col_path.hpp (which column and row pass an operator or a CG stage runs: the rule, plain C++),
// host_handle.hpp (handle, errors, shared argument checks, profiler, allocations, dispatch macros, the host's half of the
// partition), host_ops.hpp (launchers, launch_fwd_cols / launch_adj_cols that switch on the rule, the three operators),
// host_cg.hpp (CG stages and the bodies of the native stage entries, *_native) -- and
// below them nothing but the exported functions: argument checks in the order the tests rely on, then one call.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/ptycho_hip.h"
#include "fft_core.hpp"
#include "run_split.hpp"
#include "col_path.hpp"
#include "adjreg_map.hpp"
#include "k_modes.hpp"
#include "k_frc.hpp"
#include "k_gauge.hpp"
#include "k_fit.hpp"
#include "k_prepare.hpp"
#include "k_unwrap.hpp"
#include "k_resample.hpp"
#include "k_dpc.hpp"
#include "k_scangrad.hpp"

using namespace pty;

namespace {
#include "ptycho_common.hpp"
#include "k_cols_plain.hpp"
#include "k_rows.hpp"
#include "k_cols_window.hpp"
#ifdef PTYCHO_EXPERIMENTS
#include "k_fwd_fused.hpp"   // single-launch forward: measured slower, experiments build only
#endif
#include "k_cg_small.hpp"
#include "k_generic.hpp"
#include "k_zoom.hpp"
#include "k_tile.hpp"
#include "k_propagate.hpp"
}  // namespace

#include "host_handle.hpp"
#include "host_ops.hpp"
#include "host_cg.hpp"
#include "host_gauge.hpp"
#include "host_fit.hpp"
#include "host_prepare.hpp"
#include "host_unwrap.hpp"
#include "host_propagate.hpp"
#include "host_resample.hpp"
#include "host_dpc.hpp"
#include "host_scangrad.hpp"

extern "C" {

const char* ptycho_last_error(void) { return g_err.c_str(); }
#ifdef PTY_STAMPS
// diagnostic build only: read and clear the in-kernel phase stamps (tools/stamps.py)
int ptycho_debug_stamps(ptycho_handle h, unsigned long long* out24) {
    if (!h || !out24) return PTYCHO_ERR_ARG;
    if (!h->stamps) {
        if (hipMalloc((void**)&h->stamps, 24 * sizeof(unsigned long long)) != hipSuccess) return PTYCHO_ERR_HIP;
        (void)hipMemset(h->stamps, 0, 24 * sizeof(unsigned long long));
    }
    if (hipDeviceSynchronize() != hipSuccess) return PTYCHO_ERR_HIP;
    (void)hipMemcpy(out24, h->stamps, 24 * sizeof(unsigned long long), hipMemcpyDeviceToHost);
    (void)hipMemset(h->stamps, 0, 24 * sizeof(unsigned long long));
    return PTYCHO_OK;
}
#endif
const char* ptycho_version(void) { return "ptychohip 0.4 (gfx950)"; }

int ptycho_create(ptycho_handle* out, size_t ptheta, size_t nz, size_t n, size_t nscan, size_t ndet, size_t nprb) {
    if (!out) return fail(PTYCHO_ERR_ARG, "out is null");
    *out = nullptr;
    if (ptheta == 0 || nz == 0 || n == 0 || nscan == 0 || ndet == 0 || nprb == 0)
        return fail(PTYCHO_ERR_ARG, "all sizes must be positive");
    const bool pow2 = native_size(ndet);   // (name kept: "has a plan of its own"; every other size runs the Bluestein lines)
    if (ndet < 2 || ndet > 2048 || (!pow2 && ndet > 1024))
        return fail(PTYCHO_ERR_ARG, "ndet must be in [2, 1024], or a power of two up to 2048");
    if (nprb > ndet) return fail(PTYCHO_ERR_ARG, "nprb must be <= ndet");
    if (ptheta * nscan > (size_t)0x7fffffff / 2 || ptheta > (1u << 19) || nz > 65536 * 4 || n > 65536 * 4)
        return fail(PTYCHO_ERR_ARG, "problem too large for 32-bit position indices");
    ptycho_handle h = new ptycho_handle_s();
    h->ge = Geom{(int)ptheta, (int)nz, (int)n, (int)nscan, (int)ndet, (int)nprb, (int)((ndet - nprb) / 2)};
    hipError_t e = hipGetDevice(&h->device);
    if (e != hipSuccess) {
        delete h;
        return fail(PTYCHO_ERR_HIP, std::string("hipGetDevice: ") + hipGetErrorString(e));
    }
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, h->device) == hipSuccess && prop.multiProcessorCount > 0)
        h->n_cu = prop.multiProcessorCount;
    size_t tlen = ndet;
    if (!pow2) {   // Bluestein plan: smallest power of two >= 2 ndet - 1 (and >= 16)
        tlen = 16;
        while (tlen < 2 * ndet - 1) tlen *= 2;
        h->bs_m = (int)tlen;
    }
    std::vector<c32> tab(tlen);
    for (size_t k = 0; k < tlen; ++k) {
        const double ang = -2.0 * M_PI * (double)k / (double)tlen;
        tab[k] = c32{(float)std::cos(ang), (float)std::sin(ang)};
    }
    e = hipMalloc((void**)&h->table, tlen * sizeof(c32));
    if (e == hipSuccess) e = hipMemcpy(h->table, tab.data(), tlen * sizeof(c32), hipMemcpyHostToDevice);
    if (e == hipSuccess && !pow2) {
        // chirp b[m] = exp(-i pi m^2 / n) (phase reduced modulo 2 n exactly) and H = FFT_M(conj b, circular) / M in float64
        const size_t n = ndet, M = tlen;
        std::vector<double> br(n), bi(n), hr(M, 0.0), hi(M, 0.0), Hr(M), Hi(M);
        std::vector<c32> bf(n), Hf(M);
        for (size_t m = 0; m < n; ++m) {
            const double ang = -M_PI * (double)((m * m) % (2 * n)) / (double)n;
            br[m] = std::cos(ang); bi[m] = std::sin(ang);
            bf[m] = c32{(float)br[m], (float)bi[m]};
            hr[m] = br[m]; hi[m] = -bi[m];
            if (m) { hr[M - m] = br[m]; hi[M - m] = -bi[m]; }
        }
        for (size_t k = 0; k < M; ++k) {   // plain O(M^2) DFT, once per handle (M <= 2048)
            double sr = 0.0, si = 0.0;
            for (size_t m = 0; m < M; ++m) {
                if (hr[m] == 0.0 && hi[m] == 0.0) continue;
                const double ang = -2.0 * M_PI * (double)((k * m) % M) / (double)M;
                const double c = std::cos(ang), s2 = std::sin(ang);
                sr += hr[m] * c - hi[m] * s2;
                si += hr[m] * s2 + hi[m] * c;
            }
            Hf[k] = c32{(float)(sr / (double)M), (float)(si / (double)M)};
        }
        e = hipMalloc((void**)&h->bs_chirp, n * sizeof(c32));
        if (e == hipSuccess) e = hipMemcpy(h->bs_chirp, bf.data(), n * sizeof(c32), hipMemcpyHostToDevice);
        if (e == hipSuccess) e = hipMalloc((void**)&h->bs_hfilt, M * sizeof(c32));
        if (e == hipSuccess) e = hipMemcpy(h->bs_hfilt, Hf.data(), M * sizeof(c32), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess) {
        release(h);
        delete h;
        return fail(PTYCHO_ERR_HIP, std::string("twiddle table: ") + hipGetErrorString(e));
    }
    h->use_window = exp_env("PTYCHO_HIP_WINDOW", 1) != 0;
    h->use_split = exp_env("PTYCHO_HIP_SPLIT", 1) != 0;
    h->use_fused = exp_env("PTYCHO_HIP_FUSED", 0);

    h->chunk = default_chunk(h->ge);
    h->fold_rows = h->n_cu * 8 > 2048 ? h->n_cu * 8 : 2048;
    e = hipMalloc((void**)&h->fold.part, (size_t)h->fold_rows * kFoldStride * sizeof(unsigned long long));
    if (e == hipSuccess) e = hipMalloc((void**)&h->fold.ticket, 64);
    if (e == hipSuccess) e = hipMemset(h->fold.ticket, 0, 64);
    if (e != hipSuccess) {
        release(h);
        delete h;
        return fail(PTYCHO_ERR_HIP, std::string("fold scratch: ") + hipGetErrorString(e));
    }
    int rc = alloc_sort(h);   // the adjoint's scratch (up to 4 GiB) is allocated by the first ptycho_adj call
    if (rc) {
        release(h);
        delete h;
        return rc;
    }
    *out = h;
    return PTYCHO_OK;
}

int ptycho_free(ptycho_handle h) {
    if (!h) return fail(PTYCHO_ERR_ARG, "null handle");
    if (!h->freed) {
        h->freed = true;
        release(h);
    }
    return PTYCHO_OK;
}

int ptycho_destroy(ptycho_handle h) {
    if (!h) return PTYCHO_OK;
    ptycho_free(h);
    delete h;
    return PTYCHO_OK;
}

long long ptycho_get(ptycho_handle h, int which) {
    if (!h) return -1;
    switch (which) {
        case 0: return h->ge.ptheta;
        case 1: return h->ge.nz;
        case 2: return h->ge.n;
        case 3: return h->ge.nscan;
        case 4: return h->ge.ndet;
        case 5: return h->ge.nprb;
        case 100: return h->chunk;
        case 101: return h->use_window;
        case 102: return h->mask ? 1 : 0;   // measured-pixel mask set (ptycho_set_mask)?
        case 103: return h->model;          // option "model": 0 gaussian, 1 poisson_ml
        default:
            if (which >= 200 && which < 200 + ptycho_handle_s::kSlots) return h->work[which - 200] ? 1 : 0;   // CG work slot allocated?
            return -1;
    }
}

int ptycho_set_option(ptycho_handle h, const char* name, long long value) {
    if (int rc = check_args(h)) return rc;
    if (!name) return fail(PTYCHO_ERR_ARG, "null option name");
    if (std::strcmp(name, "chunk") == 0) {
        h->chunk = value > 0 ? value : default_chunk(h->ge);
        return free_scratch(h);
    }
    static const struct { const char* name; int ptycho_handle_s::*flag; } kFlags[] = {   // on / off, nothing else to do
        {"window", &ptycho_handle_s::use_window}, {"split", &ptycho_handle_s::use_split}, {"tile", &ptycho_handle_s::use_tile},
        {"deterministic", &ptycho_handle_s::deterministic}, {"ls_fused_decide", &ptycho_handle_s::ls_fused_decide}};
    for (const auto& f : kFlags) {
        if (std::strcmp(name, f.name) == 0) { h->*f.flag = value != 0; return PTYCHO_OK; }
    }
    if (std::strcmp(name, "trust_order") == 0) {
        h->trust_order = value != 0;
        h->native_order = 0;
        if (!h->trust_order) h->order_scan = nullptr;
        return PTYCHO_OK;
    }
    if (std::strcmp(name, "model") == 0) {   // likelihood of the data stages: 0 gaussian, 1 Poisson maximum likelihood
        if (value != MODEL_GAUSSIAN && value != MODEL_POISSON_ML) return fail(PTYCHO_ERR_ARG, "model must be 0 (gaussian) or 1 (poisson_ml)");
        h->model = (int)value;
        return PTYCHO_OK;
    }
    if (std::strcmp(name, "compact_modes") == 0) {   // value = number of probe modes (0: slot pairs); also makes the order chunk-major
        if (value < 0 || value > kMaxModes || (value > 0 && (long long)h->ge.ptheta * value > (1 << 19)))
            return fail(PTYCHO_ERR_ARG, "compact_modes must be in [0, 8]");
        h->compact_modes = (int)value;
        h->sort_chunks = value > 1 ? (int)value : 1;
        h->order_scan = nullptr;
        return PTYCHO_OK;
    }
    if (std::strcmp(name, "fused") == 0) {
#ifdef PTYCHO_EXPERIMENTS
        h->use_fused = (int)value;
        return PTYCHO_OK;
#else
        if (value == 0) return PTYCHO_OK;
        return fail(PTYCHO_ERR_ARG, "option fused: the single-launch forward is an experiment (measured slower, DESIGN.md); build with -DPTYCHO_EXPERIMENTS");
#endif
    }
    if (std::strcmp(name, "release_scratch") == 0)   // give back the adjoint's intermediate (<= 4 GiB; the next ptycho_adj allocates it again)
        return free_scratch(h);
    if (std::strcmp(name, "release_work") == 0) {   // give back one CG work slot (a farplane); the next stage that writes it allocates it again
        if (value < 0 || value >= ptycho_handle_s::kSlots) return fail(PTYCHO_ERR_ARG, "work slot out of range");
        HIP_TRY(hipDeviceSynchronize());
        if (h->work[value]) { HIP_TRY(hipFree(h->work[value])); h->work[value] = nullptr; }
        h->slot_max_ok[value] = false;
        return PTYCHO_OK;
    }
    if (std::strcmp(name, "defer_finish") == 0) {
        h->defer_finish = value != 0;
        h->det_pending = false;
        return PTYCHO_OK;
    }
    return fail(PTYCHO_ERR_ARG, std::string("unknown option ") + name);
}

int ptycho_set_mask(ptycho_handle h, const void* mask, void* stream) {
    if (int rc = check_args(h)) return rc;
    if (!mask) {   // clear (the buffer stays for the next mask)
        h->mask = nullptr;
        return PTYCHO_OK;
    }
    return set_mask_dispatch(h, static_cast<const unsigned char*>(mask), (hipStream_t)stream);
}

int ptycho_profile(ptycho_handle h, int enable) {
    if (int rc = check_args(h)) return rc;
    h->profile = enable != 0;
    return PTYCHO_OK;
}

int ptycho_profile_read(ptycho_handle h, double* ms, long long* launches, int n) {
    if (int rc = check_args(h)) return rc;
    if (!ms || !launches || n < 16) return fail(PTYCHO_ERR_ARG, "need arrays of at least 16 entries (18 for every kernel id)");
    for (int i = 0; i < n; ++i) { ms[i] = 0.0; launches[i] = 0; }
    for (auto& sp : h->spans) {
        HIP_TRY(hipEventSynchronize(sp.b));
        float t = 0.f;
        HIP_TRY(hipEventElapsedTime(&t, sp.a, sp.b));
        if (sp.kid < n) {   // callers with the 16-entry arrays of earlier headers do not see ids 16 / 17
            ms[sp.kid] += t;
            launches[sp.kid] += 1;
        }
        (void)hipEventDestroy(sp.a);
        (void)hipEventDestroy(sp.b);
    }
    h->spans.clear();
    return PTYCHO_OK;
}

// ---- operators ----------------------------------------------------------------------------------------------------
int ptycho_fwd(ptycho_handle h, void* g, const void* f, const void* scan, const void* prb, void* stream) {
    if (int rc = check_args(h, g, f, scan, prb)) return rc;
    hipStream_t st = (hipStream_t)stream;
    h->native_order = 0;
    if (h->bs_m) { PTY_DISPATCH_POW2(h->bs_m, (do_fwd_generic<NN>(h, (c32*)g, (const c32*)f, (const float*)scan, (const c32*)prb, st))); }
    PTY_DISPATCH(h->ge.ndet, (do_fwd<NN>(h, (c32*)g, (const c32*)f, (const float*)scan, (const c32*)prb, st)));
}

int ptycho_adj(ptycho_handle h, void* f, const void* g, const void* scan, void* prb, int flg, void* stream) {
    if (int rc = check_args(h, g, f, scan, prb)) return rc;
    if (int rc = check_flg(flg)) return rc;
    h->native_order = 0;
    hipStream_t st = (hipStream_t)stream;
    if (h->bs_m) { PTY_DISPATCH_POW2(h->bs_m, (do_adj_generic<NN>(h, (c32*)f, (const c32*)g, (const float*)scan, (c32*)prb, flg, st))); }
    PTY_DISPATCH(h->ge.ndet, (do_adj<NN>(h, (c32*)f, (const c32*)g, (const float*)scan, (c32*)prb, flg, st)));
}

int ptycho_fft2(ptycho_handle h, void* dst, const void* src, size_t nbatch, int dir, void* stream) {
    if (int rc = check_args(h, dst, src)) return rc;
    if (dir != -1 && dir != 1) return fail(PTYCHO_ERR_ARG, "dir must be -1 (forward) or +1 (inverse)");
    if (nbatch == 0) return PTYCHO_OK;
    hipStream_t st = (hipStream_t)stream;
    if (h->bs_m) { PTY_DISPATCH_POW2(h->bs_m, (do_fft2_generic<NN>(h, (c32*)dst, (const c32*)src, (long long)nbatch, dir, st))); }
    PTY_DISPATCH(h->ge.ndet, (do_fft2<NN>(h, (c32*)dst, (const c32*)src, (long long)nbatch, dir, st)));
}

// ---- scan-position gradient (k_scangrad.hpp, PtychoHIP.adj_scan / fwd_autograd) -----------------------------------------
int ptycho_adj_scan(ptycho_handle h, float* out, const void* g, const void* f, const void* scan, const void* prb, void* work,
                    size_t work_tiles, void* stream) {
    if (int rc = check_args(h, out, g, f, scan, prb, work)) return rc;
    if (work_tiles == 0) return fail(PTYCHO_ERR_ARG, "work_tiles must be positive");
    if (work == g) return fail(PTYCHO_ERR_ARG, "work must not be g");
    return do_adj_scan(h, out, (const c32*)g, (const c32*)f, (const float*)scan, (const c32*)prb, (c32*)work, work_tiles,
                       (hipStream_t)stream);
}

// ---- CG stages, one probe -----------------------------------------------------------------------------------------
int ptycho_cg_fwd_cols(ptycho_handle h, int slot, const void* f, const void* scan, const void* prb, void* stream) {
    if (int rc = check_args(h, f, scan, prb)) return rc;
    return fwd_cols_stage(h, slot, f, scan, prb, (hipStream_t)stream);
}

int ptycho_cg_adj_cols(ptycho_handle h, int slot, void* f, const void* scan, void* prb, int flg, void* stream) {
    if (int rc = check_args(h, f, scan, prb)) return rc;
    if (int rc = check_flg(flg)) return rc;
    if (int rc = need_slots(h, slot)) return rc;
    return adj_cols_stage(h, slot, f, scan, prb, flg, nullptr, 1, (hipStream_t)stream);
}

int ptycho_cg_stats(ptycho_handle h, int slot, const void* data, double* sums, void* stream) {
    if (int rc = check_args(h, data, sums)) return rc;
    if (int rc = need_slots(h, slot)) return rc;
    return stats_stage(h, slot, data, sums, 0, (hipStream_t)stream);
}

int ptycho_cg_project(ptycho_handle h, int src_slot, int dst_slot, const void* data, const double* ab,
                      double* cost, void* stream) {
    if (int rc = check_args(h, data, cost)) return rc;
    if (int rc = need_slots(h, src_slot)) return rc;
    return project_stage(h, src_slot, dst_slot, data, nullptr, ab, 0, cost, 0, (hipStream_t)stream);
}

int ptycho_cg_linesearch(ptycho_handle h, int slot1, int slot2, const void* data, const double* ab, double gamma0,
                         int ncand, double* costs, void* stream) {
    if (int rc = check_args(h, data, costs)) return rc;
    if (int rc = check_ncand(ncand)) return rc;
    return linesearch_stage(h, slot1, slot2, data, LsSearch{ab, gamma0, ncand, costs, nullptr, 0}, (hipStream_t)stream);
}

// ---- CG stages, several probe modes -------------------------------------------------------------------------------
int ptycho_cg_project_multi(ptycho_handle h, int src_slot, int dst_slot, const void* data, const void* inten,
                            const double* ab, int slot_unscaled, double* cost, void* stream) {
    if (int rc = check_args(h, data, cost, inten)) return rc;
    if (int rc = need_slots(h, src_slot)) return rc;
    return project_stage(h, src_slot, dst_slot, data, inten, ab, slot_unscaled ? 1 : 0, cost, 0, (hipStream_t)stream);
}

int ptycho_cg_intensity_modes(ptycho_handle h, int nmodes, void* inten, const void* data, double* sums, void* stream) {
    if (int rc = check_args(h)) return rc;
    if (nmodes < 1 || nmodes > kMaxModes) return fail(PTYCHO_ERR_ARG, "nmodes must be in [1, 8]");
    if (!inten && !sums) return fail(PTYCHO_ERR_ARG, "nothing to compute: inten and sums are both null");
    if (sums && !data) return fail(PTYCHO_ERR_ARG, "null operand");
    return intensity_stage(h, nmodes, inten, data, sums, (hipStream_t)stream);
}

int ptycho_cg_linesearch_modes(ptycho_handle h, int mode0, int nmodes, const void* data, const void* inten,
                               const double* ab, double gamma0, int ncand, double* costs, void* stream) {
    if (int rc = check_args(h, data, costs)) return rc;
    if (mode0 < 0 || nmodes < 1 || mode0 + nmodes > kMaxModes) return fail(PTYCHO_ERR_ARG, "modes must lie in [0, 8)");
    if (int rc = check_ncand(ncand)) return rc;
    if (h->compact_modes && nmodes != 1) return fail(PTYCHO_ERR_ARG, "compact slot layout: one mode pair per call (use ptycho_cg_linesearch_chunk)");
    return linesearch_modes_stage(h, mode0, nmodes, data, inten, LsSearch{ab, gamma0, ncand, costs, nullptr, 0}, (hipStream_t)stream);
}

int ptycho_cg_fwd_cols_modes(ptycho_handle h, int nmodes, int mode0, const void* f, const void* scan,
                             const void* const* prbs, int into_b, int chunk, void* stream) {
    return fwd_cols_modes_impl(h, nmodes, mode0, f, scan, prbs, into_b, chunk, stream, nullptr);
}

int ptycho_cg_linesearch_chunk(ptycho_handle h, int chunk, const void* data, const double* ab, double gamma0,
                               int ncand, double* costs, void* stream) {
    if (int rc = check_args(h, data, costs)) return rc;
    if (!h->compact_modes || chunk < 0 || chunk >= h->sort_chunks) return fail(PTYCHO_ERR_ARG, "chunked line search needs the compact slot layout");
    if (int rc = check_ncand(ncand)) return rc;
    return linesearch_chunk_stage(h, chunk, data, LsSearch{ab, gamma0, ncand, costs, nullptr, 0}, (hipStream_t)stream);
}

// ---- registration (position correction) ---------------------------------------------------------------------------
int ptycho_cg_cross(ptycho_handle h, int slot1, int slot2, double gamma, void* image_product, void* stream) {
    if (int rc = check_args(h)) return rc;
    return cross_public(h, slot1, slot2, gamma, nullptr, image_product, (hipStream_t)stream);
}

int ptycho_cg_cross_dev(ptycho_handle h, int slot1, int slot2, const double* gamma_dev, void* image_product, void* stream) {
    if (int rc = check_args(h, gamma_dev)) return rc;
    return cross_public(h, slot1, slot2, 0.0, gamma_dev, image_product, (hipStream_t)stream);
}

int ptycho_cg_argmax(ptycho_handle h, int slot, void* best, void* stream) {
    if (int rc = check_args(h, best)) return rc;
    if (int rc = need_slots(h, slot)) return rc;
    return argmax_stage(h, slot, (unsigned long long*)best, (hipStream_t)stream);
}

int ptycho_cg_zoom(ptycho_handle h, const void* image_product, const void* best, const void* vt,
                   const void* lz, int nc, int ups, double upsample_factor, void* shifts, void* stream) {
    return zoom_impl(h, image_product, best, vt, lz, nc, ups, upsample_factor, shifts, nullptr, stream);
}

// ---- native CG stages: the iteration on the device-resident state -----------------------------------------------------
int ptycho_cg_obj_begin2(ptycho_handle h, double* state, const void* psi, const void* scan, const void* prb,
                         const void* ones_prb, const void* data, void* stream) {
    if (int rc = check_stage(h, state, psi, scan, prb, data)) return rc;
    return obj_begin_native(h, state, psi, scan, prb, ones_prb, data, (hipStream_t)stream);
}
int ptycho_cg_obj_begin(ptycho_handle h, double* state, const void* psi, const void* scan, const void* prb,
                        const void* data, void* stream) {
    return ptycho_cg_obj_begin2(h, state, psi, scan, prb, nullptr, data, stream);
}

int ptycho_cg_obj_grad(ptycho_handle h, double* state, const void* scan, void* prb, const void* data, void* grad,
                       void* stream) {
    if (int rc = check_stage(h, state, scan, prb, data, grad)) return rc;
    return obj_grad_native(h, state, scan, prb, data, grad, (hipStream_t)stream);
}

int ptycho_cg_obj_dir(ptycho_handle h, double* state, int first, const void* scan, const void* prb, const void* data,
                      void* grad, void* grad0, void* dpsi, void* stream) {
    return ptycho_cg_obj_dir2(h, state, first, scan, prb, nullptr, data, grad, grad0, dpsi, stream);
}
int ptycho_cg_obj_dir2(ptycho_handle h, double* state, int first, const void* scan, const void* prb, const void* ones_prb,
                       const void* data, void* grad, void* grad0, void* dpsi, void* stream) {
    if (int rc = check_stage(h, state, scan, prb, data, grad, grad0, dpsi)) return rc;
    return obj_dir_native(h, state, first, scan, prb, ones_prb, data, grad, grad0, dpsi, (hipStream_t)stream);
}

int ptycho_cg_ls_next(ptycho_handle h, double* state, int which, int pass, const void* data, int use_ab, void* stream) {
    if (int rc = check_stage(h, state)) return rc;
    if (which < 0 || which > 1 || pass < 1 || pass > 7 || !data) return fail(PTYCHO_ERR_ARG, "bad line-search stage");
    return ls_next_native(h, state, which, pass, data, use_ab, (hipStream_t)stream);
}

int ptycho_cg_obj_finish(ptycho_handle h, double* state, int correct_positions, void* psi, const void* dpsi, void* scan,
                         const void* ones_prb, const void* vt, const void* lz, int nc, int ups, double upsample_factor,
                         void* stream) {
    if (int rc = check_stage(h, state, psi, dpsi, scan)) return rc;
    return obj_finish_native(h, state, correct_positions, psi, dpsi, scan, ones_prb, vt, lz, nc, ups, upsample_factor, (hipStream_t)stream);
}

int ptycho_cg_reg_prepare(ptycho_handle h, double* state, const void* psi, const void* scan, const void* ones_prb, void* stream) {
    if (int rc = check_stage(h, state, psi, scan, ones_prb)) return rc;
    return fwd_cols_stage(h, 2, psi, scan, ones_prb, (hipStream_t)stream, h->ge.nscan);
}

int ptycho_cg_prb_grad(ptycho_handle h, double* state, const void* psi, const void* scan, const void* prb,
                       const void* data, void* gprb, void* stream) {
    if (int rc = check_stage(h, state, psi, scan, prb, data, gprb)) return rc;
    return prb_grad_native(h, state, psi, scan, prb, data, gprb, (hipStream_t)stream);
}

int ptycho_cg_prb_dir(ptycho_handle h, double* state, int first, double nscan_total, double nmodes, const void* psi,
                      const void* scan, const void* data, void* gprb, void* gprb0, void* dprb, void* stream) {
    if (int rc = check_stage(h, state, psi, scan, data, gprb, gprb0, dprb)) return rc;
    return prb_dir_native(h, state, first, nscan_total, nmodes, psi, scan, data, gprb, gprb0, dprb, (hipStream_t)stream);
}

int ptycho_cg_prb_finish(ptycho_handle h, double* state, void* prb, const void* dprb, void* stream) {
    if (int rc = check_stage(h, state, prb, dprb)) return rc;
    return axpy_state(h, prb, dprb, h->ge.prb_elems(), state + PTYCHO_ST_GAMMA_PRB, (hipStream_t)stream);
}

// ---- line searches of the multi-mode loop on the device-resident state (ptycho.py:383-393, 451-461 with nmodes > 1) ----
int ptycho_cg_ls_begin(ptycho_handle h, double* state, int which, void* stream) {
    if (int rc = check_stage(h, state)) return rc;
    if (int rc = check_which(which)) return rc;
    return ls_begin_native(state, which, (hipStream_t)stream);
}

int ptycho_cg_ls_decide(ptycho_handle h, double* state, int which, int next_groups, void* stream) {
    if (int rc = check_stage(h, state)) return rc;
    if (which < 0 || which > 1 || next_groups < 0 || next_groups > kLsGroupsMax) return fail(PTYCHO_ERR_ARG, "bad line-search decision");
    return ls_decide_native(state, which, next_groups, (hipStream_t)stream);
}

int ptycho_cg_ls_obj_chunk(ptycho_handle h, double* state, int chunk, const void* dpsi, const void* scan,
                           const void* const* prbs, const void* data, const double* ab, void* stream) {
    if (int rc = check_stage(h, state, dpsi, scan, prbs, data)) return rc;
    if (!h->compact_modes || chunk < 0 || chunk >= h->sort_chunks) return fail(PTYCHO_ERR_ARG, "chunked line search needs the compact slot layout");
    return ls_obj_chunk_native(h, state, chunk, dpsi, scan, prbs, data, ab, stream);
}

int ptycho_cg_ls_prb_pass(ptycho_handle h, double* state, int mode, const void* data, const void* inten, void* stream) {
    if (int rc = check_stage(h, state, data, inten)) return rc;
    if (mode < 0 || mode >= kMaxModes) return fail(PTYCHO_ERR_ARG, "modes must lie in [0, 8)");
    return linesearch_modes_stage(h, mode, 1, data, inten, ls_on_state(state, nullptr, 1), (hipStream_t)stream);
}

// ---- orthogonal probe modes (k_modes.hpp) and Fourier ring correlation (k_frc.hpp, libtike.hipfft.frc): no handle ----
int ptycho_orthogonalize_modes(void* prb, void* dprb, void* gradprb0, size_t ptheta, int nmodes, size_t npix,
                                          void* v_out, double* powers, void* stream) {
    if (nmodes < 1 || nmodes > kOrthoMaxModes) return fail(PTYCHO_ERR_ARG, "nmodes must be in [1, 16]");
    if (!prb) return fail(PTYCHO_ERR_ARG, "prb is null");
    if (npix == 0) return fail(PTYCHO_ERR_ARG, "npix must be positive");
    if (ptheta == 0) return fail(PTYCHO_ERR_ARG, "ptheta must be positive");
    if (!v_out || !powers) return fail(PTYCHO_ERR_ARG, "v_out and powers must not be null");
    const unsigned long long blocks = (npix + 255) / 256;
    if (ptheta > (1u << 30) || npix > (1ull << 40) || blocks * ptheta * 3 > 0xffffffffull)
        return fail(PTYCHO_ERR_ARG, "ptheta * npix too large for one launch");
    c32* x[3] = {(c32*)prb, nullptr, nullptr};
    int narr = 1;
    if (dprb) x[narr++] = (c32*)dprb;
    if (gradprb0) x[narr++] = (c32*)gradprb0;
    return orthogonalize_modes(nmodes, x, narr, (int)ptheta, (long long)npix, (double*)v_out, powers, (hipStream_t)stream);
}

// ---- Fourier ring correlation (k_frc.hpp, libtike.hipfft.frc) ------------------------------------------------------------
int ptycho_frc_prepare(void* out, const void* a, const void* b, size_t ptheta, size_t nz, size_t n, size_t y0,
                                  size_t x0, size_t s, const float* window, void* stream) {
    if (!out || !a || !b) return fail(PTYCHO_ERR_ARG, "out, a and b must not be null");
    if (!frc_size_ok((long long)s)) return fail(PTYCHO_ERR_ARG, "s must be in [16, 1024] or 2048");
    if (ptheta == 0 || ptheta > kFrcMaxAngles) return fail(PTYCHO_ERR_ARG, "ptheta must be in [1, 32767]");
    if (y0 > nz || s > nz - y0 || x0 > n || s > n - x0) return fail(PTYCHO_ERR_ARG, "the crop lies outside the image");
    if (nz > (1ull << 32) || n > (1ull << 32)) return fail(PTYCHO_ERR_ARG, "image too large");
    const dim3 grid((unsigned)((s + 255) / 256), (unsigned)s, (unsigned)(2 * ptheta));
    hipLaunchKernelGGL(k_frc_prepare, grid, dim3(256), 0, (hipStream_t)stream, (c32*)out, (const c32*)a, (const c32*)b,
                       (int)ptheta, (long long)nz, (long long)n, (long long)y0, (long long)x0, (int)s, window);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

int ptycho_frc_rings(double* sums, const void* spec, size_t ptheta, size_t s, const double* shift,
                                void* stream) {
    if (!sums || !spec) return fail(PTYCHO_ERR_ARG, "sums and spec must not be null");
    if (!frc_size_ok((long long)s)) return fail(PTYCHO_ERR_ARG, "s must be in [16, 1024] or 2048");
    if (ptheta == 0 || ptheta > kFrcMaxAngles) return fail(PTYCHO_ERR_ARG, "ptheta must be in [1, 32767]");
    const dim3 grid((unsigned)frc_rings((int)s), (unsigned)ptheta);
    hipLaunchKernelGGL(k_frc_rings, grid, dim3(kFrcThreads), 0, (hipStream_t)stream, sums, (const c32*)spec, (int)ptheta,
                       (int)s, shift);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

// ---- illumination map and gauge fixing (k_gauge.hpp, libtike.hipfft.gauge): no handle -----------------------------------
// the five sizes of an illumination walk (ptycho_illumination, ptycho_scan_map), the channels (one for the illumination
// itself) and the modes; flat: the launch also runs one thread per position of every angle (k_scan_keep)
static int illum_check_sizes(size_t ptheta, size_t nscan, int nval, int nmodes, size_t nprb, size_t nz, size_t n, bool flat) {
    if (ptheta == 0 || nscan == 0 || nprb == 0 || nz == 0 || n == 0) return fail(PTYCHO_ERR_ARG, "all sizes must be positive");
    if (nval < 1 || nval > kMapMaxVal) return fail(PTYCHO_ERR_ARG, "nval must be in [1, 4]");
    if (nmodes < 1) return fail(PTYCHO_ERR_ARG, "nmodes must be at least 1");
    if (ptheta > kGaugeMaxAngles) return fail(PTYCHO_ERR_ARG, "ptheta must be in [1, 65535]");
    if (nz > kGaugeMaxSide || n > kGaugeMaxSide || nprb > kGaugeMaxSide || nscan > 0x7fffffffull ||
        (nz + kIllTileH - 1) / kIllTileH > 65535 || (flat && (ptheta * nscan + 255) / 256 > 0x7fffffffull))
        return fail(PTYCHO_ERR_ARG, "nz, n, nprb or nscan too large for one launch");
    return PTYCHO_OK;
}

int ptycho_illumination(float* out, const void* scan, const void* probe, size_t ptheta, size_t nscan, int nmodes,
                        size_t nprb, size_t nz, size_t n, void* stream) {
    if (!out || !scan || !probe) return fail(PTYCHO_ERR_ARG, "out, scan and probe must not be null");
    if (int rc = illum_check_sizes(ptheta, nscan, 1, nmodes, nprb, nz, n, false)) return rc;
    return do_illumination(out, (const float*)scan, (const c32*)probe, (int)ptheta, (int)nscan, nmodes, (int)nprb, (int)nz,
                           (int)n, (hipStream_t)stream);
}

int ptycho_gauge_fit(double* gauge, const void* psi, const void* ref, const float* weight, size_t ptheta, size_t nz,
                     size_t n, double* work, void* stream) {
    if (!gauge || !psi || !work) return fail(PTYCHO_ERR_ARG, "gauge, psi and work must not be null");
    if (ptheta == 0 || nz == 0 || n == 0) return fail(PTYCHO_ERR_ARG, "all sizes must be positive");
    if (ptheta > kGaugeMaxAngles) return fail(PTYCHO_ERR_ARG, "ptheta must be in [1, 65535]");
    if (nz > kGaugeMaxSide || n > kGaugeMaxSide) return fail(PTYCHO_ERR_ARG, "nz or n too large for one launch");
    return do_gauge_fit(gauge, (const c32*)psi, (const c32*)ref, weight, (int)ptheta, (int)nz, (int)n, work,
                        (hipStream_t)stream);
}

int ptycho_gauge_apply(void* x, const double* gauge, size_t ptheta, size_t ny, size_t nx, int which, void* stream) {
    if (!x || !gauge) return fail(PTYCHO_ERR_ARG, "x and gauge must not be null");
    if (ptheta == 0 || ny == 0 || nx == 0) return fail(PTYCHO_ERR_ARG, "all sizes must be positive");
    if (int rc = check_which(which)) return rc;
    if (ptheta > kGaugeMaxAngles) return fail(PTYCHO_ERR_ARG, "ptheta must be in [1, 65535]");
    if (ny > kGaugeMaxSide || nx > kGaugeMaxSide || ((nx + 255) / 256) * ny > 0x7fffffffull)
        return fail(PTYCHO_ERR_ARG, "ny or nx too large for one launch");
    return do_gauge_apply((c32*)x, gauge, (int)ptheta, (int)ny, (int)nx, which, (hipStream_t)stream);
}

// ---- fit residuals per frame and per pixel (k_fit.hpp, libtike.hipfft.fit): no handle --------------------------------------
int ptycho_fit_accumulate(float* inten, const void* g, size_t count, int add, void* stream) {
    if (!inten || !g) return fail(PTYCHO_ERR_ARG, "inten and g must not be null");
    if (count == 0) return fail(PTYCHO_ERR_ARG, "count must be positive");
    if (count > kFitMaxElems || (count + 1023) / 1024 > 0x7fffffffull)
        return fail(PTYCHO_ERR_ARG, "count too large for one launch");
    return do_fit_accumulate(inten, (const c32*)g, count, add, (hipStream_t)stream);
}

size_t ptycho_fit_work_words(size_t ptheta, size_t nscan, size_t npix) {
    return frame_work_words<FitPart>(fit_sizes_ok(ptheta, nscan, npix), ptheta, nscan, npix);
}

int ptycho_fit_frames(double* frames, double* pixels, const float* inten, const void* g, const float* data,
                      const unsigned char* mask, const double* ab, size_t ptheta, size_t nscan, size_t npix,
                      double* work, void* stream) {
    if (!frames || !data || !work) return fail(PTYCHO_ERR_ARG, "frames, data and work must not be null");
    if (!inten && !g) return fail(PTYCHO_ERR_ARG, "inten and g must not both be null");
    if (ptheta == 0 || nscan == 0 || npix == 0) return fail(PTYCHO_ERR_ARG, "all sizes must be positive");
    if (ptheta > kFitMaxAngles) return fail(PTYCHO_ERR_ARG, "ptheta must be in [1, 65535]");
    if (!fit_sizes_ok(ptheta, nscan, npix) ||
        (ptheta * nscan * FitPart::kCols + ptheta * FitPart::kMaps * npix) / 256 + 2 > 0x7fffffffull)
        return fail(PTYCHO_ERR_ARG, "nscan, npix or their product with ptheta too large for one launch");
    return do_fit_frames(frames, pixels, inten, (const c32*)g, data, mask, ab, (long long)ptheta, (long long)nscan,
                         (long long)npix, work, (hipStream_t)stream);
}

// ---- raw detector frames to solver data (k_prepare.hpp, libtike.hipfft.prepare): no handle -------------------------------
size_t ptycho_prepare_work_words(size_t ptheta, size_t nscan, size_t npix) {
    return frame_work_words<PrepPart>(prep_sizes_ok(ptheta, nscan, npix), ptheta, nscan, npix);
}

int ptycho_prepare_frames(float* data, unsigned char* mask, double* frames, double* pixels, const void* raw, int dtype,
                          const long long* index, const float* dark, const float* gain, const unsigned char* bad,
                          size_t ptheta, size_t nraw, size_t nscan, size_t H, size_t W, long long y0, long long x0,
                          int bin, size_t ndet, float saturation, float scale, int clip, double* work, void* stream) {
    if (!data || !mask || !frames || !raw || !work)
        return fail(PTYCHO_ERR_ARG, "data, mask, frames, raw and work must not be null");
    if (ptheta == 0 || nraw == 0 || nscan == 0 || H == 0 || W == 0 || ndet == 0)
        return fail(PTYCHO_ERR_ARG, "all sizes must be positive");
    if (bin != 1 && bin != 2 && bin != 4) return fail(PTYCHO_ERR_ARG, "bin must be 1, 2 or 4");
    if (dtype < 0 || dtype >= kPrepDtypes)
        return fail(PTYCHO_ERR_ARG, "dtype must be 0 (uint16), 1 (uint32), 2 (int32) or 3 (float32)");
    if (ptheta > kPrepMaxAngles) return fail(PTYCHO_ERR_ARG, "ptheta must be in [1, 65535]");
    if (!index && nraw != nscan) return fail(PTYCHO_ERR_ARG, "without an index nraw must equal nscan");
    if (ndet > kPrepMaxNdet || !prep_sizes_ok(ptheta, nscan, ndet * ndet) || !prep_raw_ok(ptheta, nraw, H, W) ||
        y0 < -kPrepMaxOrigin || y0 > kPrepMaxOrigin || x0 < -kPrepMaxOrigin || x0 > kPrepMaxOrigin ||
        (ptheta * nscan * PrepPart::kCols + ptheta * PrepPart::kMaps * ndet * ndet) / 256 + 2 > 0x7fffffffull)
        return fail(PTYCHO_ERR_ARG, "sizes, window origin or their products too large for one launch");
    const PrepGeom g{(long long)H, (long long)W, y0, x0, bin, (int)ndet};
    return do_prepare_frames(data, mask, frames, pixels, raw, dtype, index, dark, gain, bad, (long long)ptheta,
                             (long long)nraw, (long long)nscan, g, saturation, scale, clip, work, (hipStream_t)stream);
}

// ---- weighted least-squares phase unwrapping (k_unwrap.hpp, libtike.hipfft.unwrap): no handle ----------------------------
size_t ptycho_unwrap_work_words(size_t ptheta, size_t nz, size_t n) {
    if (!unwrap_sizes_ok(ptheta, nz, n)) return 0;
    return ptheta * (size_t)unwrap_tiles((int)nz, (int)n) * kUnwPart;
}

size_t ptycho_unwrap_buffer_floats(size_t ptheta, size_t nz, size_t n) {
    if (!unwrap_sizes_ok(ptheta, nz, n)) return 0;
    return ptheta * kUnwPlanes * nz * n;
}

static int unwrap_check_sizes(size_t ptheta, size_t nz, size_t n) {
    if (ptheta == 0 || ptheta > kUnwMaxAngles) return fail(PTYCHO_ERR_ARG, "ptheta must be in [1, 65535]");
    if (nz < 2 || n < 2) return fail(PTYCHO_ERR_ARG, "nz and n must be at least 2");
    if (!unwrap_sizes_ok(ptheta, nz, n)) return fail(PTYCHO_ERR_ARG, "nz * n too large: it must stay below 2^31");
    return PTYCHO_OK;
}

int ptycho_unwrap_begin(float* buf, double* state, const float* phase, const float* weight, size_t ptheta, size_t nz,
                        size_t n, double* work, void* stream) {
    if (!buf || !state || !phase || !work) return fail(PTYCHO_ERR_ARG, "buf, state, phase and work must not be null");
    if (int rc = unwrap_check_sizes(ptheta, nz, n)) return rc;
    return do_unwrap_begin(buf, state, phase, weight, (int)ptheta, (int)nz, (int)n, work, (hipStream_t)stream);
}

int ptycho_unwrap_iterate(float* buf, double* state, const float* weight, size_t ptheta, size_t nz, size_t n, int niter,
                          int maxiter, double tol, double* work, void* stream) {
    if (!buf || !state || !work) return fail(PTYCHO_ERR_ARG, "buf, state and work must not be null");
    if (int rc = unwrap_check_sizes(ptheta, nz, n)) return rc;
    if (niter < 0 || maxiter < 0) return fail(PTYCHO_ERR_ARG, "niter and maxiter must not be negative");
    if (!(tol >= 0.0) || !(tol < INFINITY)) return fail(PTYCHO_ERR_ARG, "tol must be finite and not negative");
    return do_unwrap_iterate(buf, state, weight, (int)ptheta, (int)nz, (int)n, niter, maxiter, tol, work,
                             (hipStream_t)stream);
}

int ptycho_unwrap_finish(float* out, double* state, const float* buf, const float* phase, const float* weight,
                         int congruent, size_t ptheta, size_t nz, size_t n, double* work, void* stream) {
    if (!out || !state || !buf || !phase || !work)
        return fail(PTYCHO_ERR_ARG, "out, state, buf, phase and work must not be null");
    if (int rc = unwrap_check_sizes(ptheta, nz, n)) return rc;
    return do_unwrap_finish(out, state, buf, phase, weight, congruent != 0, (int)ptheta, (int)nz, (int)n, work,
                            (hipStream_t)stream);
}

int ptycho_unwrap_residues(signed char* charge, long long* count, const float* phase, const float* weight, size_t ptheta,
                           size_t nz, size_t n, void* stream) {
    if (!count || !phase) return fail(PTYCHO_ERR_ARG, "count and phase must not be null");
    if (int rc = unwrap_check_sizes(ptheta, nz, n)) return rc;
    return do_unwrap_residues(charge, count, phase, weight, (int)ptheta, (int)nz, (int)n, (hipStream_t)stream);
}

// ---- first look: frame moments, scan map, gradient integration (k_dpc.hpp, libtike.hipfft.dpc): no handle --------------------
static bool moments_sizes_ok(size_t ptheta, size_t nscan, size_t ndet) {
    return ndet >= 1 && ndet <= 46340 && fit_sizes_ok(ptheta, nscan, ndet * ndet);   // ndet^2 <= 2^31 - 1
}

size_t ptycho_frame_moments_work_words(size_t ptheta, size_t nscan, size_t ndet) {
    return frame_work_words<MomPart>(moments_sizes_ok(ptheta, nscan, ndet), ptheta, nscan, ndet * ndet);
}

int ptycho_frame_moments(double* moments, const float* data, const unsigned char* mask, double darkfield, size_t ptheta,
                         size_t nscan, size_t ndet, double* work, void* stream) {
    if (!moments || !data || !work) return fail(PTYCHO_ERR_ARG, "moments, data and work must not be null");
    if (ptheta == 0 || nscan == 0 || ndet == 0) return fail(PTYCHO_ERR_ARG, "all sizes must be positive");
    if (ptheta > kFitMaxAngles) return fail(PTYCHO_ERR_ARG, "ptheta must be in [1, 65535]");
    if (darkfield != darkfield || darkfield == INFINITY) return fail(PTYCHO_ERR_ARG, "darkfield must be a finite radius, or negative for none");
    if (!moments_sizes_ok(ptheta, nscan, ndet) || (ptheta * nscan * MomPart::kCols) / 256 + 2 > 0x7fffffffull)
        return fail(PTYCHO_ERR_ARG, "nscan, ndet or their product with ptheta too large for one launch");
    return do_frame_moments(moments, data, mask, darkfield, (long long)ptheta, (long long)nscan, (long long)ndet, work,
                            (hipStream_t)stream);
}

int ptycho_scan_map(float* weight, float* out, const float* values, const unsigned char* keep, const void* scan,
                    const void* probe, size_t ptheta, size_t nscan, int nval, int nmodes, size_t nprb, size_t nz, size_t n,
                    int raw, float* work, void* stream) {
    if (!weight || !out || !values || !scan || !probe)
        return fail(PTYCHO_ERR_ARG, "weight, out, values, scan and probe must not be null");
    if (keep && !work) return fail(PTYCHO_ERR_ARG, "work must not be null when keep is given");
    if (int rc = illum_check_sizes(ptheta, nscan, nval, nmodes, nprb, nz, n, true)) return rc;
    return do_scan_map(weight, out, values, keep, (const float*)scan, (const c32*)probe, (int)ptheta, (int)nscan, nval, nmodes,
                       (int)nprb, (int)nz, (int)n, raw != 0, work, (hipStream_t)stream);
}

int ptycho_integrate_begin(float* buf, double* state, const float* gy, const float* gx, const float* weight, size_t ptheta,
                           size_t nz, size_t n, double* work, void* stream) {
    if (!buf || !state || !gy || !gx || !work) return fail(PTYCHO_ERR_ARG, "buf, state, gy, gx and work must not be null");
    if (int rc = unwrap_check_sizes(ptheta, nz, n)) return rc;
    return do_integrate_begin(buf, state, gy, gx, weight, (int)ptheta, (int)nz, (int)n, work, (hipStream_t)stream);
}

int ptycho_integrate_finish(float* out, double* state, const float* buf, const float* weight, size_t ptheta, size_t nz,
                            size_t n, double* work, void* stream) {
    if (!out || !state || !buf || !work) return fail(PTYCHO_ERR_ARG, "out, state, buf and work must not be null");
    if (int rc = unwrap_check_sizes(ptheta, nz, n)) return rc;
    return do_integrate_finish(out, state, buf, weight, (int)ptheta, (int)nz, (int)n, work, (hipStream_t)stream);
}

// ---- free-space propagation and focus-series figures (k_propagate.hpp, libtike.hipfft.propagate) -------------------------
size_t ptycho_propagate_work_words(ptycho_handle h, size_t nfield, size_t nplane, int planes_wanted) {
    if (!h || h->freed || !prop_sizes_ok((size_t)h->ge.ndet, nfield, nplane)) return 0;
    if (planes_wanted || prop_fused(h)) return 0;
    return nfield * nplane * (size_t)h->ge.ndet * (size_t)h->ge.ndet;   // one complex64 per float64 word
}

int ptycho_propagate(ptycho_handle h, void* planes, double* metrics, const void* spec, size_t nfield, const double* zl,
                     size_t nplane, double q0, int method, void* work, void* stream) {
    if (int rc = check_args(h)) return rc;
    if (!spec || !zl || !work) return fail(PTYCHO_ERR_ARG, "spec, zl and work must not be null");
    if (!planes && !metrics) return fail(PTYCHO_ERR_ARG, "nothing to compute: planes and metrics are both null");
    if (!frc_size_ok(h->ge.ndet)) return fail(PTYCHO_ERR_ARG, "the handle's ndet must be in [16, 1024] or 2048");
    if (nfield == 0 || nplane == 0) return fail(PTYCHO_ERR_ARG, "nfield and nplane must be positive");
    if (!prop_sizes_ok((size_t)h->ge.ndet, nfield, nplane)) return fail(PTYCHO_ERR_ARG, "nfield * nplane must stay below 2^30");
    if (method != 0 && method != 1) return fail(PTYCHO_ERR_ARG, "method must be 0 (fresnel) or 1 (angular spectrum)");
    if (!(q0 >= 0.0) || !(q0 < INFINITY)) return fail(PTYCHO_ERR_ARG, "q0 must be finite and not negative");
    if (!aligned16(spec) || !aligned16(planes)) return fail(PTYCHO_ERR_ARG, "spec and planes must be 16-byte aligned");
    const PropArgs a{(c32*)planes, metrics, (const c32*)spec, zl, (c32*)work, (long long)nfield, (long long)nplane, q0, method};
    hipStream_t st = (hipStream_t)stream;
    if (h->bs_m) { PTY_DISPATCH_POW2(h->bs_m, (do_propagate_generic<NN>(h, a, st))); }
    PTY_DISPATCH(h->ge.ndet, (do_propagate<NN>(h, a, st)));
}

// ---- B-spline resampling: prefilter, affine warp, moments (k_resample.hpp, libtike.hipfft.resample): no handle ------------
static int resample_check_sizes(size_t nimg, size_t ny, size_t nx, const char* what) {
    if (nimg == 0 || nimg > kRsMaxImages) return fail(PTYCHO_ERR_ARG, "nimg must be in [1, 65535]");
    if (ny < 2 || nx < 2) return fail(PTYCHO_ERR_ARG, std::string(what) + " sides must be at least 2");
    if (!resample_sizes_ok(nimg, ny, nx))
        return fail(PTYCHO_ERR_ARG, std::string(what) + " sides must be at most 65536 and their product below 2^31");
    return PTYCHO_OK;
}

size_t ptycho_spline_work_words(size_t nimg, size_t ny, size_t nx, int cplx) {
    if (!resample_sizes_ok(nimg, ny, nx)) return 0;
    return (nimg * ny * nx * (cplx ? 2 : 1) + 1) / 2;
}

int ptycho_spline_prefilter(void* out, const void* in, size_t nimg, size_t ny, size_t nx, int cplx, int order, void* work,
                            void* stream) {
    if (!out || !in || !work) return fail(PTYCHO_ERR_ARG, "out, in and work must not be null");
    if (int rc = resample_check_sizes(nimg, ny, nx, "image")) return rc;
    if (order < 0 || order > 5) return fail(PTYCHO_ERR_ARG, "order must be in [0, 5]");
    if (work == out || work == in) return fail(PTYCHO_ERR_ARG, "work must be neither out nor in");
    hipStream_t st = (hipStream_t)stream;
    const int C = cplx ? 2 : 1;
    float* o = (float*)out;
    const float* i = (const float*)in;
    switch (order) {
        case 2: return do_spline_prefilter<2>(o, i, (int)nimg, (int)ny, (int)nx, C, (float*)work, st);
        case 3: return do_spline_prefilter<3>(o, i, (int)nimg, (int)ny, (int)nx, C, (float*)work, st);
        case 4: return do_spline_prefilter<4>(o, i, (int)nimg, (int)ny, (int)nx, C, (float*)work, st);
        case 5: return do_spline_prefilter<5>(o, i, (int)nimg, (int)ny, (int)nx, C, (float*)work, st);
        default: break;   // orders 0 and 1 interpolate the samples themselves
    }
    if (out != in) HIP_TRY(hipMemcpyAsync(out, in, nimg * ny * nx * C * sizeof(float), hipMemcpyDeviceToDevice, st));
    return PTYCHO_OK;
}

int ptycho_warp(void* out, const void* coef, const double* xf, size_t nimg, size_t ny, size_t nx, size_t oh, size_t ow,
                int cplx, int order, int flags, float cval_re, float cval_im, int* path, void* stream) {
    if (!out || !coef || !xf) return fail(PTYCHO_ERR_ARG, "out, coef and xf must not be null");
    if (int rc = resample_check_sizes(nimg, ny, nx, "image")) return rc;
    if (oh == 0 || ow == 0) return fail(PTYCHO_ERR_ARG, "output sides must be positive");
    if (oh > kRsMaxSide || ow > kRsMaxSide || oh * ow >= kRsMaxPixels)
        return fail(PTYCHO_ERR_ARG, "output sides must be at most 65536 and their product below 2^31");
    if (order < 0 || order > 5) return fail(PTYCHO_ERR_ARG, "order must be in [0, 5]");
    if (flags & ~(RS_MIRROR | RS_GLOBAL)) return fail(PTYCHO_ERR_ARG, "flags must be a combination of 1 (mirror) and 2 (global)");
    if (out == coef) return fail(PTYCHO_ERR_ARG, "out must not be coef");
    hipStream_t st = (hipStream_t)stream;
#define WARP_CASE(O)                                                                                                      \
    case O: return do_warp<O>(out, coef, xf, (int)nimg, (int)ny, (int)nx, (int)oh, (int)ow, cplx, flags, cval_re, cval_im, path, st)
    switch (order) {
        WARP_CASE(0);
        WARP_CASE(1);
        WARP_CASE(2);
        WARP_CASE(3);
        WARP_CASE(4);
        default: break;
    }
    return do_warp<5>(out, coef, xf, (int)nimg, (int)ny, (int)nx, (int)oh, (int)ow, cplx, flags, cval_re, cval_im, path, st);
#undef WARP_CASE
}

size_t ptycho_moments_work_words(size_t nimg, size_t ny, size_t nx) {
    if (!resample_sizes_ok(nimg, ny, nx)) return 0;
    return nimg * (size_t)rs_moment_blocks((long long)(ny * nx)) * kRsMomWords;
}

int ptycho_moments(double* sums, const void* x, const float* weight, size_t nimg, size_t ny, size_t nx, int cplx, int which,
                   double* work, void* stream) {
    if (!sums || !x || !work) return fail(PTYCHO_ERR_ARG, "sums, x and work must not be null");
    if (int rc = resample_check_sizes(nimg, ny, nx, "image")) return rc;
    if (which < 0 || which > 2) return fail(PTYCHO_ERR_ARG, "which must be 0 (value), 1 (positive) or 2 (power)");
    if (cplx && which != RS_POWER) return fail(PTYCHO_ERR_ARG, "a complex image has no value or positive part: which must be 2");
    return do_moments(sums, (const float*)x, weight, (int)nimg, (int)ny, (int)nx, cplx != 0, which, work, (hipStream_t)stream);
}

}  // extern "C"
