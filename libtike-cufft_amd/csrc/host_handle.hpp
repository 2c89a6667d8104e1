// host_handle.hpp -- the handle behind ptycho_hip.h and what every entry point needs around it: error text, the
// in-library profiler, the handle's allocations (scratch, position sort, mask) and the per-size dispatch macros.
// Included by ptycho_kernels.hip after the kernel headers; the struct is the C ABI's opaque type and so sits at
// global scope, everything else is internal.
struct ptycho_handle_s {
    Geom ge;
    c32* table = nullptr;     // exp(-2 pi i k / ndet)  (ndet not a power of two: k / bs_m)
    int bs_m = 0;             // 0: ndet is a power of two; else length of the Bluestein plan (k_generic.hpp)
    c32* bs_chirp = nullptr;  // exp(-i pi m^2 / ndet), m < ndet
    c32* bs_hfilt = nullptr;  // FFT_M of the circular conj-chirp, divided by M
    c32* scratch = nullptr;   // chunk * ndet^2 complex64
    long long chunk = 0;      // positions per launch pair
    // position sort (object / probe adjoint)
    int* order = nullptr;          // processing order: position order[k] is the k-th in (angle, column bucket, row) order
    int* sort_counts = nullptr;    // k_rank_positions: partial ranks [positions] + tickets [ceil(positions / 256)], self-clearing
    static constexpr int kSlots = 2 * kMaxModes;
    c32* work[kSlots] = {};   // CG work buffers (column-pass intermediates), all positions; 0/1 + per-mode pairs
    double* slot_maxw = nullptr;      // [kSlots] max |slot content| left by the PROJECT stage (deterministic option)
    bool slot_max_ok[kSlots] = {};    // ... and whether that word describes what the slot holds now
    void* zoom_phase = nullptr;           // registration: per-pattern phases + whole-pixel shifts
    c32* reg_ip = nullptr;                // native CG loop: image product of the registration [positions][ndet][ndet]
    unsigned long long* reg_best = nullptr;   // whole-pixel peaks [positions]
    double* reg_shifts = nullptr;         // sub-pixel shifts [positions][2]
    int use_window = 1;       // 0: direct-atomics object adjoint (k_cols<ADJ_OBJ>)
    int use_split = 1;        // ndet = 256: one radix-16 step of the DFT over y runs in the row pass
    int use_tile = 1;         // ndet <= 128: one-launch forward / probe adjoint, the tile stays in LDS (k_tile.hpp)
    int deterministic = 0;    // 1: adjoints accumulate in 64-bit fixed point (integer atomics): bitwise reproducible results
    long long* det_acc = nullptr;   // fixed-point image, 2 words per object (or probe) element, kept zero between calls
    double* det_words = nullptr;    // device: max |g|, max |probe or object| as float bits (k_cg_absmax)
    DetScale last_det{};            // scale of the adjoint whose sums sit in det_acc (k_det_finish / k_cg_dy_reduce fold them in)
    bool det_pending = false;       // native CG stages: the gradient is still in det_acc (option "defer_finish")
    int defer_finish = 0;           // 1: ptycho_cg_obj_grad / prb_grad leave the gradient in det_acc for ptycho_cg_*_dir
    int ls_fused_decide = 0;        // 1: line-search passes decide on their own totals (single GPU: nothing to all-reduce)
    bool max_prb_valid = false, max_psi_valid = false;   // state[MAX_PRB / MAX_PSI] were set by the *_grad stage of this step
    FoldBuf fold{};                 // fixed-order cross-workgroup sums (ptycho_common.hpp): n_cu * 8 rows + ticket
    int fold_rows = 0;
    int compact_modes = 0;    // multi-mode CG: 0 = slot pairs (2k, 2k+1); M = compact layout A(k) = k, one shared B = M
    int sort_chunks = 1;      // position order is chunk-major over this many equal position ranges (chunked line search)
    int use_fused = 0;        // ndet = 256 forward as one launch (k_fwd_fused256): 0 off (default: measured slower), 1 / 2 class tiles per pass
    c32* prbp = nullptr;      // fused forward: c * probe in a zero-bordered ndet x ndet frame, per angle
    int trust_order = 0;      // 1: caller vouches that scan is unchanged since the last sort
    int native_order = 0;     // 1: the native CG stages are running and track scan themselves (ptycho_cg_obj_finish re-sorts
                              // after it moved the positions); cleared by ptycho_fwd / ptycho_adj, whose callers own trust_order
    const float* order_scan = nullptr;   // scan pointer the current order was computed from
    unsigned* mask = nullptr;       // measured-pixel mask of the CG stages that read data (ptycho_set_mask), nullptr: none
    unsigned* mask_buf = nullptr;   // ... its buffer (k_pack_mask layout + a count word), kept across masks, freed by ptycho_free
    int model = MODEL_GAUSSIAN;     // likelihood of the CG stages that read data (option "model", CgModel)
#ifdef PTY_STAMPS
    unsigned long long* stamps = nullptr;   // diagnostic build: 24 words (forward column pass, object adjoint column pass)
#endif
    int device = 0;
    int n_cu = 256;
    bool freed = false;
    bool profile = false;
    struct Span { int kid; hipEvent_t a, b; };
    std::vector<Span> spans;
};

namespace {

thread_local std::string g_err;

// Launch-geometry and code-path knobs read from the environment exist only in the experiments build
// (`make -C libtike-cufft_amd/csrc experiments`, -DPTYCHO_EXPERIMENTS); the shipped library uses the defaults.
#ifdef PTYCHO_EXPERIMENTS
int exp_env(const char* name, int dflt) {
    const char* e = std::getenv(name);
    return e ? std::atoi(e) : dflt;
}
#else
constexpr int exp_env(const char*, int dflt) { return dflt; }
#endif

// kernel ids for the in-library profiler (ptycho_profile_read)
enum { K_COLS_FWD = 0, K_ROWS_FWD = 1, K_ROWS_INV = 2, K_COLS_ADJ_OBJ = 3, K_COLS_ADJ_PRB = 4, K_COLS_PLAIN = 5, K_SORT = 6, K_ROWS_STATS = 7, K_ROWS_PROJECT = 8, K_ROWS_LINESEARCH = 9, K_CG_SCALARS = 10, K_FWD_FUSED = 11, K_CG_UPDATE = 12, K_ROWS_CROSS = 13, K_COLS_ARGMAX = 14, K_ZOOM = 15, K_TILE_FWD = 16, K_TILE_ADJ_PRB = 17, K_COUNT = 18 };

int fail(int code, const std::string& msg) {
    g_err = msg;
    return code;
}

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return fail(PTYCHO_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_)); \
    } while (0)

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

// launch of a 256-thread kernel template <bool VEC> on the stream st: kernel<true> (16-byte accesses) where vec holds,
// else kernel<false>; returns from the calling launcher on a launch error (HIP_TRY)
#define VEC_LAUNCH(kernel, vec, grid, st, ...)                                                      \
    do {                                                                                            \
        if (vec) hipLaunchKernelGGL(kernel<true>, grid, dim3(256), 0, st, __VA_ARGS__);             \
        else hipLaunchKernelGGL(kernel<false>, grid, dim3(256), 0, st, __VA_ARGS__);                \
        HIP_TRY(hipGetLastError());                                                                 \
    } while (0)

// the host's half of a FramePart (frame_part.hpp) for checked sizes: the plan and the launch grid of the pass, where the
// pass writes (fpart, ppart), and after the pass the fold of whatever it left in work (nothing: one wave tile and one range)
template <class Part>
struct FrameFold {
    FramePlan p;
    double *frames, *pixels, *fpart, *ppart;
    long long ptheta, nscan, npix;
    FrameFold(double* frames_, double* pixels_, double* work, long long ptheta_, long long nscan_, long long npix_)
        : p(Part::plan(ptheta_, nscan_, npix_)), frames(frames_), pixels(pixels_), fpart(p.fwords ? work : frames_),
          ppart(p.pwords ? work + p.fwords : pixels_), ptheta(ptheta_), nscan(nscan_), npix(npix_) {}
    dim3 grid() const { return dim3((unsigned)p.ntiles, (unsigned)p.nranges, (unsigned)ptheta); }
    // pix: the kernel's own eighth argument, the slab Part::kMaps * npix (k_fit_fold) or npix (k_prepare_fold)
    template <class K>
    int fold(K kernel, long long pix, hipStream_t st) const {
        const long long nfout = p.fwords ? ptheta * nscan * Part::kCols : 0;
        const long long npout = p.pwords && pixels ? ptheta * Part::kMaps * npix : 0;
        const long long fblocks = (nfout + 255) / 256, pblocks = (npout + 255) / 256;
        if (fblocks + pblocks > 0) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)(fblocks + pblocks)), dim3(256), 0, st, frames, pixels,
                               (const double*)fpart, (const double*)ppart, nfout, p.nwt, npout, pix, p.nranges,
                               (unsigned)fblocks);
            HIP_TRY(hipGetLastError());
        }
        return PTYCHO_OK;
    }
};

// body of ptycho_fit_work_words / ptycho_prepare_work_words; ok: the sizes passed the caller's limits
template <class Part>
size_t frame_work_words(bool ok, size_t ptheta, size_t nscan, size_t npix) {
    if (!ok) return 0;
    const FramePlan p = Part::plan((long long)ptheta, (long long)nscan, (long long)npix);
    return (size_t)(p.fwords + p.pwords);
}

// prologue of an entry point: the handle is live and none of the operands is null
template <class... P>
int check_args(ptycho_handle h, const P*... operands) {
    if (!h) return fail(PTYCHO_ERR_ARG, "null handle");
    if (h->freed) return fail(PTYCHO_ERR_FREED, "handle used after ptycho_free");
    if ((... || (operands == nullptr))) return fail(PTYCHO_ERR_ARG, "null operand");
    return PTYCHO_OK;
}
// ... of a native CG stage: the device-resident state comes before the operands
template <class... P>
int check_stage(ptycho_handle h, const double* state, const P*... operands) {
    int rc = check_args(h);
    if (rc) return rc;
    if (!state) return fail(PTYCHO_ERR_ARG, "null state");
    return check_args(h, operands...);
}

// argument checks that several entry points share
inline int check_flg(int flg) { return flg == 0 || flg == 1 ? (int)PTYCHO_OK : fail(PTYCHO_ERR_ARG, "flg must be 0 (object) or 1 (probe)"); }
inline int check_which(int which) { return which == 0 || which == 1 ? (int)PTYCHO_OK : fail(PTYCHO_ERR_ARG, "which must be 0 (object) or 1 (probe)"); }
inline int check_ncand(int ncand) { return ncand >= 1 && ncand <= kMaxCand ? (int)PTYCHO_OK : fail(PTYCHO_ERR_ARG, "ncand must be in [1, 16]"); }

struct ProfSpan {   // brackets one launch with events when profiling is on
    ptycho_handle h;
    hipStream_t st;
    ptycho_handle_s::Span sp;
    bool on;
    ProfSpan(ptycho_handle h_, int kid, hipStream_t st_) : h(h_), st(st_), sp{kid, nullptr, nullptr}, on(h_->profile) {
        if (on) {
            on = hipEventCreate(&sp.a) == hipSuccess && hipEventCreate(&sp.b) == hipSuccess &&
                 hipEventRecord(sp.a, st) == hipSuccess;
        }
    }
    ~ProfSpan() {
        if (on && hipEventRecord(sp.b, st) == hipSuccess) h->spans.push_back(sp);
    }
};

long long default_chunk(const Geom& ge) {
    if (exp_env("PTYCHO_HIP_CHUNK", 0) > 0) return exp_env("PTYCHO_HIP_CHUNK", 0);
    // Large chunks stream best (measured: the row pass runs at ~5-6 TB/s for chunks
    // >= 256 MiB; small chunks only add launch gaps).  Cap the scratch at 4 GiB.
    const long long per = (long long)ge.ndet * ge.ndet * 8;
    long long c = (4ll << 30) / per;
    if (c < 16) c = 16;
    return c;
}

int alloc_scratch(ptycho_handle h) {
    if (h->scratch) {
        HIP_TRY(hipFree(h->scratch));
        h->scratch = nullptr;
    }
    const long long total = h->ge.npos();
    long long c = h->chunk < total ? h->chunk : total;
    if (c < 1) c = 1;
    HIP_TRY(hipMalloc((void**)&h->scratch, (size_t)c * h->ge.ndet * h->ge.ndet * sizeof(c32)));
    return PTYCHO_OK;
}

int free_scratch(ptycho_handle h) {   // options "chunk" and "release_scratch": launches in flight may still read it
    HIP_TRY(hipDeviceSynchronize());
    if (h->scratch) { HIP_TRY(hipFree(h->scratch)); h->scratch = nullptr; }
    return PTYCHO_OK;
}

// processing order of the windowed column passes: (angle, column bucket, row), one ranking launch (k_rank_positions)
int sort_positions(ptycho_handle h, const float* scan, hipStream_t st) {
    const int total = (int)h->ge.npos();
    // The order depends only on the scan positions.  A caller that knows they have not
    // changed since the previous call on this handle (option "trust_order") skips the sort.
    if ((h->trust_order || h->native_order) && h->order_scan == scan) return PTYCHO_OK;
    h->order_scan = scan;
    const int iblocks = (total + 255) / 256;
    int nslices = (2 * h->n_cu + iblocks - 1) / iblocks;
    if (nslices > iblocks) nslices = iblocks;   // = number of key tiles
    if (nslices < 1) nslices = 1;
    {
        ProfSpan ps(h, K_SORT, st);
        const int pc = (total + h->sort_chunks - 1) / h->sort_chunks;   // positions per chunk
        hipLaunchKernelGGL(k_rank_positions, dim3((unsigned)(iblocks * nslices)), dim3(256), 0, st, scan, h->ge, total, nslices,
                           h->sort_counts, h->sort_counts + total, h->order, pc);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

int alloc_sort(ptycho_handle h) {
    const size_t total = (size_t)h->ge.npos();
    const size_t nwords = total + (total + 255) / 256;
    HIP_TRY(hipMalloc((void**)&h->order, total * sizeof(int)));
    HIP_TRY(hipMalloc((void**)&h->sort_counts, nwords * sizeof(int)));
    HIP_TRY(hipMemset(h->sort_counts, 0, nwords * sizeof(int)));
    return PTYCHO_OK;
}

template <class T>
void free_and_null(T*& p) {
    if (p) (void)hipFree((void*)p);
    p = nullptr;
}

void release(ptycho_handle h) {
    h->mask = nullptr;   // points into mask_buf
    free_and_null(h->slot_maxw); free_and_null(h->mask_buf); free_and_null(h->det_acc); free_and_null(h->det_words);
    free_and_null(h->fold.part); free_and_null(h->fold.ticket);
    free_and_null(h->table); free_and_null(h->bs_chirp); free_and_null(h->bs_hfilt);
    free_and_null(h->scratch); free_and_null(h->order); free_and_null(h->sort_counts);
    free_and_null(h->zoom_phase); free_and_null(h->prbp);
    free_and_null(h->reg_ip); free_and_null(h->reg_best); free_and_null(h->reg_shifts);
    for (auto& w : h->work) free_and_null(w);
    for (auto& sp : h->spans) { (void)hipEventDestroy(sp.a); (void)hipEventDestroy(sp.b); }
    h->spans.clear();
}

// detector sizes with their own Stockham plan (fft_core.hpp): the powers of two 16 ... 2048 and five sizes with an odd factor
inline bool native_size(size_t n) {
    return ((n & (n - 1)) == 0 && n >= 16 && n <= 2048) || n == 48 || n == 80 || n == 96 || n == 112 || n == 192;
}
#define PTY_DISPATCH_POW2_CASES(CALL)                             \
        case 16: { constexpr int NN = 16; return CALL; }         \
        case 32: { constexpr int NN = 32; return CALL; }         \
        case 64: { constexpr int NN = 64; return CALL; }         \
        case 128: { constexpr int NN = 128; return CALL; }       \
        case 256: { constexpr int NN = 256; return CALL; }       \
        case 512: { constexpr int NN = 512; return CALL; }       \
        case 1024: { constexpr int NN = 1024; return CALL; }     \
        case 2048: { constexpr int NN = 2048; return CALL; }
#define PTY_DISPATCH(N_, CALL)                                   \
    switch (N_) {                                                \
        PTY_DISPATCH_POW2_CASES(CALL)                            \
        case 48: { constexpr int NN = 48; return CALL; }         \
        case 80: { constexpr int NN = 80; return CALL; }         \
        case 96: { constexpr int NN = 96; return CALL; }         \
        case 112: { constexpr int NN = 112; return CALL; }       \
        case 192: { constexpr int NN = 192; return CALL; }       \
        default: return fail(PTYCHO_ERR_ARG, "this entry point needs a detector size with a Stockham plan: a power of two in [16, 2048] or 48, 80, 96, 112, 192"); \
    }
// length of a Bluestein plan: always a power of two
#define PTY_DISPATCH_POW2(N_, CALL)                              \
    switch (N_) {                                                \
        PTY_DISPATCH_POW2_CASES(CALL)                            \
        default: return fail(PTYCHO_ERR_ARG, "internal: Bluestein plan length is not a power of two"); \
    }

// ptycho_set_mask: pack ndet^2 bytes (nonzero = measured) into h->mask and count the measured pixels
template <int N>
int pack_mask(ptycho_handle h, const unsigned char* m, hipStream_t st) {
    constexpr int W = N * Plan<N>::T;
    static_assert(W <= N * N / 12, "mask buffer size");
    unsigned* cnt = h->mask_buf + W;
    HIP_TRY(hipMemsetAsync(cnt, 0, sizeof(unsigned), st));
    hipLaunchKernelGGL((k_pack_mask<N>), dim3((unsigned)((W + 255) / 256)), dim3(256), 0, st, m, h->mask_buf, cnt);
    HIP_TRY(hipGetLastError());
    unsigned n = 0;
    HIP_TRY(hipMemcpyAsync(&n, cnt, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (n == 0) return fail(PTYCHO_ERR_ARG, "mask has no measured pixel (a / b would be 0 / 0)");
    h->mask = h->mask_buf;
    return PTYCHO_OK;
}

int set_mask_dispatch(ptycho_handle h, const unsigned char* m, hipStream_t st) {
    h->mask = nullptr;
    if (!h->mask_buf) {   // every plan has N T <= N^2 / 12 words; + the count word
        const size_t n = (size_t)h->ge.ndet * h->ge.ndet;
        HIP_TRY(hipMalloc((void**)&h->mask_buf, (n / 12 + 1) * sizeof(unsigned)));
    }
    PTY_DISPATCH(h->ge.ndet, (pack_mask<NN>(h, m, st)));
}

}  // namespace
