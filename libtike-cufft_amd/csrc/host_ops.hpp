// host_ops.hpp -- the operators behind ptycho_fwd / ptycho_adj / ptycho_fft2: launchers of the column, row and tile
// kernels with their measured launch geometry, the deterministic (fixed-point) begin / end, and the Bluestein path of
// the detector sizes without a Stockham plan.  Included by ptycho_kernels.hip after host_handle.hpp.
namespace {

// shortest run of sorted positions a windowed column workgroup takes (each run pays one window fill)
// 512 positions x 256^2 CG: 8 -> 1.44, 16 -> 1.36, 24 -> 1.51 ms per iteration.  Tiny problems (fewer than one workgroup per CU at
// runs of 16) take shorter runs, down to 4: a workgroup's positions are processed one after the other (~5 us each)
static int min_seglen(int np = 1 << 30, int nstrips = 1, int n_cu = 256) {
    static const int v = exp_env("PTYCHO_HIP_MINSEG", 16);
    return min_run(np, nstrips, n_cu, v);
}

template <int N, int DIR, int MODE>
int launch_cols(ptycho_handle h, ColArgs a, hipStream_t st) {
    using CC = ColCfg<N>;
    const int np = a.k_end - a.k_begin;
    if (np <= 0 || a.nstrips <= 0) return PTYCHO_OK;
    int target = h->n_cu * 8;
    int ng = target / a.nstrips;
    if (ng < 1) ng = 1;
    if (ng > np) ng = np;
    a.ngroups = ng;
    constexpr int kid = MODE == M_FWD ? K_COLS_FWD : MODE == M_ADJ_OBJ ? K_COLS_ADJ_OBJ : MODE == M_ADJ_PRB ? K_COLS_ADJ_PRB : K_COLS_PLAIN;
    {
        ProfSpan ps(h, kid, st);
        hipLaunchKernelGGL((k_cols<N, DIR, MODE>), dim3((unsigned)(a.nstrips * ng)), dim3(CC::NT), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

template <int N, bool SPLIT = false, int CW = 0>
int launch_adjwin(ptycho_handle h, ColArgs a, hipStream_t st, int wg_target = 0) {
    constexpr int NTHREADS = Plan<N>::T * (CW ? CW : ColCfg<N>::C);
    const int np = a.k_end - a.k_begin;
    if (np <= 0 || a.nstrips <= 0) return PTYCHO_OK;
    // contiguous runs of the sorted order; about 4 workgroups per CU in total
    // ndet 256: two rounds of resident workgroups (one round of runs of 128: within 1 %, six or eight rounds: +4 %);
    // ndet 128: ONE round (two workgroups per CU, runs of 32 positions): 0.234 -> 0.197 ms at 4096 x 128^2; 64 and 32: no gain / worse
    if (wg_target <= 0) wg_target = h->n_cu * (N == 128 ? 2 : 4);   // (512: runs of 128 instead of 64 positions: 1.728 -> 1.709 ms, profiles/r04/stamps.txt)
    const RunSplit rs = split_runs(np, a.nstrips, wg_target, min_seglen(np, a.nstrips, h->n_cu));
    static const int nt_mode_a = exp_env("PTYCHO_HIP_NT", 0);
    a.nt = nt_mode_a;
#ifdef PTY_STAMPS
    a.stamps = h->stamps;
#endif
    {
        ProfSpan ps(h, K_COLS_ADJ_OBJ, st);
        // ndet 256 and 512: overlap-add window in registers (k_cols_adjreg); the other sizes keep the LDS window
        if constexpr ((N == 256 || N == 512) && CW == 0)
            hipLaunchKernelGGL((k_cols_adjreg<N, SPLIT>), dim3((unsigned)(a.nstrips * rs.nseg)), dim3(NTHREADS), 0, st, a, rs.seglen);
        else
            hipLaunchKernelGGL((k_cols_adjwin<N, SPLIT, CW>), dim3((unsigned)(a.nstrips * rs.nseg)), dim3(NTHREADS), 0, st, a, rs.seglen);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

template <int N, int MODE, bool SPLIT = false, int CW = 0>
int launch_gatherwin(ptycho_handle h, ColArgs a, hipStream_t st, int wg_target = 0) {
    constexpr int NTHREADS = Plan<N>::T * (CW ? CW : ColCfg<N>::C);
    const int np = a.k_end - a.k_begin;
    if (np <= 0 || a.nstrips <= 0) return PTYCHO_OK;
    // whole rounds of resident workgroups (two per CU un-split, three split): a ragged last round costs 5-20 % (round 3: 1.5
    // rounds of the un-split forward pass made the CG iteration 8.43 -> 8.87 ms; one long round 8.49)
    if (wg_target <= 0) wg_target = h->n_cu * (SPLIT ? 6 : 4);
    RunSplit rs = split_runs(np, a.nstrips, wg_target, min_seglen(np, a.nstrips, h->n_cu));
#ifdef PTYCHO_EXPERIMENTS
    {   // experiment knob: fewer, longer runs
        const int want = exp_env("PTYCHO_HIP_COLSEGS", 0);
        if (want > 0) {
            rs.seglen = (np + want - 1) / want;
            if (rs.seglen > kRunMax) rs.seglen = kRunMax;
            rs.nseg = (np + rs.seglen - 1) / rs.seglen;
        }
    }
#endif
    static const int nt_mode_g = exp_env("PTYCHO_HIP_NT", 0);
    a.nt = nt_mode_g;
#ifdef PTY_STAMPS
    a.stamps = h->stamps;
#endif
    {
        ProfSpan ps(h, MODE == M_FWD ? K_COLS_FWD : K_COLS_ADJ_PRB, st);
        hipLaunchKernelGGL((k_cols_gatherwin<N, MODE, SPLIT, 1, CW>), dim3((unsigned)(a.nstrips * rs.nseg)), dim3(NTHREADS), 0, st, a, rs.seglen);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

template <int N, int DIR>
int launch_rows(ptycho_handle h, RowArgs a, hipStream_t st) {
    constexpr int B = 256 / Plan<N>::T;
    if (a.nrows <= 0) return PTYCHO_OK;
    long long nb = (a.nrows + B - 1) / B;
    long long grid = nb < (long long)h->n_cu * 8 ? nb : (long long)h->n_cu * 8;
    // nontemporal row-pass loads and stores: the rows are streamed once (measured 3-4 % on the pair;
    // nontemporal column-pass accesses made no difference).  PTYCHO_HIP_NT overrides (bit mask).
    static const int nt_mode = exp_env("PTYCHO_HIP_NT", 3);
    a.nt = nt_mode;
    {
        ProfSpan ps(h, DIR < 0 ? K_ROWS_FWD : K_ROWS_INV, st);
        hipLaunchKernelGGL((k_rows<N, DIR>), dim3((unsigned)grid), dim3(256), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

template <int N, int DIR>
int launch_rows_split(ptycho_handle h, RowArgs a, hipStream_t st) {
    if (a.nrows <= 0) return PTYCHO_OK;
    const long long nitems = (a.nrows / N) * 16;
    // measured at 4096 x 256^2: forward best with ~32 workgroups per CU in the grid (0.73 ms vs 0.75
    // at 8), adjoint best with one item per workgroup (0.70 ms vs 0.78); PTYCHO_HIP_ROWGRID overrides.  Swept again with the
    // forward pass's 16 requests per item in one batch (profiles/r19/rows_split_issue.txt): forward 0.744 / 0.719 / 0.700 /
    // 0.713 / 0.702 ms at 8 / 16 / 32 / 64 / 128; adjoint 0.775 / 0.757 / 0.717 / 0.702 ms at 8 / 16 / 64 / 128 against
    // 0.707 - 0.722 at 256, one spread of its runs and so not adopted.  Both values stay.
    static const int env_mult = exp_env("PTYCHO_HIP_ROWGRID", 0);
    const int mult = env_mult > 0 ? env_mult : (DIR < 0 ? 32 : 256);
    long long grid = nitems < (long long)h->n_cu * mult ? nitems : (long long)h->n_cu * mult;
    {
        ProfSpan ps(h, DIR < 0 ? K_ROWS_FWD : K_ROWS_INV, st);
        hipLaunchKernelGGL((k_rows_split<N, DIR>), dim3((unsigned)grid), dim3(256), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

// the strips of C detector columns that the probe touches
inline void strip_range(const Geom& ge, int C, int& strip0, int& nstrips) {
    strip0 = ge.pad / C;
    const int last = (ge.pad + ge.nprb - 1) / C;
    nstrips = last - strip0 + 1;
}

// ---- the column pass of an operator or a CG stage: the path (col_path.hpp), its arguments, one launcher per direction ----
// force_window: the multi-mode forward stage is windowed wherever the window fits, whatever option window says
template <int N>
ColPath col_path_for(ptycho_handle h, ColMode mode, bool allow_split, bool force_window = false) {
    return col_path(N, WinCfg<N>::fits, h->use_window || force_window, h->use_split, allow_split, mode);
}

// what every column launch shares: table, geometry, positions and their order (nullptr: as they come), range of positions,
// strips of C columns
ColArgs col_args(ptycho_handle h, const float* scan, long long k_begin, long long k_end, const int* order, int C) {
    ColArgs ca{};
    ca.scan = scan; ca.table = h->table; ca.ge = h->ge; ca.order = order;
    ca.k_begin = (int)k_begin; ca.k_end = (int)k_end;
    strip_range(h->ge, C, ca.strip0, ca.nstrips);
    return ca;
}
template <int N>
ColArgs col_args(ptycho_handle h, const float* scan, long long k_begin, long long k_end, ColPath p, ColMode mode) {
    return col_args(h, scan, k_begin, k_end, col_path_sorts(p, mode) ? h->order : nullptr, col_strip_width(p, mode, ColCfg<N>::C));
}

// The if constexpr guards keep kernels that do not exist (no window at 1024 / 2048, split at 256 only) from being instantiated.
template <int N>
int launch_fwd_cols(ptycho_handle h, const ColArgs& ca, hipStream_t st, bool allow_split, bool force_window = false) {
    switch (col_path_for<N>(h, COL_FWD, allow_split, force_window)) {
        case COLS_PLAIN: return launch_cols<N, -1, M_FWD>(h, ca, st);
        case COLS_GATHERWIN:
            if constexpr (WinCfg<N>::fits) return launch_gatherwin<N, M_FWD>(h, ca, st);
            break;
        case COLS_GATHERWIN_SPLIT:
            // exactly one resident round of workgroups (two per CU), runs of 64 positions at 4096: 0.42 -> 0.395 ms against
            // two rounds of shorter runs; 1.5 or 3 rounds (a ragged tail) cost 10-20 % (profiles/r03/knob_sweep.txt)
            if constexpr (N == 256) return launch_gatherwin<N, M_FWD, true, kSplitFwdC>(h, ca, st, h->n_cu * 2);
            break;
        default: break;
    }
    return fail(PTYCHO_ERR_ARG, "internal: no forward column pass for this path");
}

template <int N>
int launch_adj_cols(ptycho_handle h, const ColArgs& ca, int flg, hipStream_t st, bool allow_split) {
    switch (col_path_for<N>(h, flg == 0 ? COL_ADJ_OBJ : COL_ADJ_PRB, allow_split)) {
        case COLS_PLAIN: return flg == 0 ? launch_cols<N, +1, M_ADJ_OBJ>(h, ca, st) : launch_cols<N, +1, M_ADJ_PRB>(h, ca, st);
        case COLS_ADJWIN:
        case COLS_ADJREG:   // launch_adjwin picks k_cols_adjreg at 256 and 512
            if constexpr (WinCfg<N>::fits) return launch_adjwin<N>(h, ca, st);
            break;
        case COLS_GATHERWIN:
            if constexpr (WinCfg<N>::fits) return launch_gatherwin<N, M_ADJ_PRB>(h, ca, st);
            break;
        case COLS_ADJREG_SPLIT:
            if constexpr (N == 256) return launch_adjwin<N, true>(h, ca, st);
            break;
        case COLS_GATHERWIN_SPLIT:
            if constexpr (N == 256) return launch_gatherwin<N, M_ADJ_PRB, true>(h, ca, st);
            break;
    }
    return fail(PTYCHO_ERR_ARG, "internal: no adjoint column pass for this path");
}

#ifdef PTYCHO_EXPERIMENTS
int do_fwd_fused(ptycho_handle h, c32* g, const c32* f, const float* scan, const c32* prb, hipStream_t st) {
    const Geom& ge = h->ge;
    const int total = (int)ge.npos();
    const int N = ge.ndet;
    if (!h->prbp) HIP_TRY(hipMalloc((void**)&h->prbp, (size_t)ge.ptheta * N * N * sizeof(c32)));
    // positions in sorted order: the workgroups in flight then touch neighbouring object rows (L2 hits)
    int rc = sort_positions(h, scan, st);
    if (rc) return rc;
    const int npix = ge.ptheta * N * N;
    hipLaunchKernelGGL(k_pad_probe, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, prb, h->prbp, ge);
    FusedArgs fa{};
    fa.f = f; fa.g = g; fa.prbp = h->prbp; fa.scan = scan; fa.table = h->table; fa.order = h->order; fa.ge = ge; fa.total = total;
    const int tiles = h->use_fused >= 2 ? 2 : 1;
    const int nitems = total * (4 / tiles);
    const int grid = nitems < h->n_cu ? nitems : h->n_cu;
    {
        ProfSpan ps(h, K_FWD_FUSED, st);
        if (tiles == 2) hipLaunchKernelGGL((k_fwd_fused256<2>), dim3((unsigned)grid), dim3(1024), 0, st, fa);
        else hipLaunchKernelGGL((k_fwd_fused256<1>), dim3((unsigned)grid), dim3(1024), 0, st, fa);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}
#endif

// ---- one-launch operators for ndet <= 128 (k_tile.hpp): persistent workgroups, as many as fit a CU's LDS ----
template <int N>
unsigned tile_grid(ptycho_handle h, long long npos, int max_per_cu = 0) {
    using CF = TileCfg<N>;
    int per_cu = (int)((160 * 1024) / CF::lds_bytes);
    if (per_cu * CF::NT > 2048) per_cu = 2048 / CF::NT;
    if (max_per_cu > 0 && per_cu > max_per_cu) per_cu = max_per_cu;
    if (per_cu < 1) per_cu = 1;
    long long wg = (npos + CF::TPW - 1) / CF::TPW;
    const long long cap = (long long)h->n_cu * per_cu;
    return (unsigned)(wg < cap ? (wg < 1 ? 1 : wg) : cap);
}
template <int N>
int launch_fwd_tile(ptycho_handle h, c32* g, const c32* f, const float* scan, const c32* prb, hipStream_t st) {
    const Geom& ge = h->ge;
    TileArgs ta{};
    ta.obj = f; ta.prb = prb; ta.g = g; ta.scan = scan; ta.table = h->table; ta.ge = ge;
    ta.npos = (int)(ge.npos());
    {
        ProfSpan ps(h, K_TILE_FWD, st);
        hipLaunchKernelGGL((k_fwd_tile<N>), dim3(tile_grid<N>(h, ta.npos)), dim3(TileCfg<N>::NT), 0, st, ta);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}
template <int N>
int launch_adjprb_tile(ptycho_handle h, c32* prb_out, const c32* g, const float* scan, const c32* f, hipStream_t st) {
    const Geom& ge = h->ge;
    TileArgs ta{};
    ta.obj = f; ta.g = const_cast<c32*>(g); ta.out = prb_out; ta.scan = scan; ta.table = h->table; ta.ge = ge;
    ta.npos = (int)(ge.npos());
    {
        ProfSpan ps(h, K_TILE_ADJ_PRB, st);
                // every workgroup ends with one atomic pair per probe pixel, all on the same ndet^2 addresses: few, long-running
        // workgroups (four per CU: 1.90 ms at 16384 x 16^2, 0.27 at 32^2, 0.108 at 4096 x 64^2; one / two: 0.040, 0.093, 0.096)
        hipLaunchKernelGGL((k_adjprb_tile<N>), dim3(tile_grid<N>(h, ta.npos, N <= 16 ? 1 : 2)), dim3(TileCfg<N>::NT), 0, st, ta);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

// ---- deterministic adjoints (option "deterministic"): set-up before / fold-in after the column pass ----
inline unsigned fold_grid(ptycho_handle h, long long n, int per_cu) {   // grid of a kernel that folds: <= fold_rows workgroups
    long long g = (n + 255) / 256;
    long long cap = (long long)h->n_cu * per_cu;
    if (cap > h->fold_rows) cap = h->fold_rows;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}
// max |x| as float bits into *word (fixed-order fold); scale_ab: x *= scale_ab[0] / scale_ab[1] on the way
void launch_absmax(ptycho_handle h, const c32* x, long long n, int per_cu, double* word, const double* scale_ab, hipStream_t st) {
    hipLaunchKernelGGL(k_cg_absmax, dim3(fold_grid(h, n, per_cu)), dim3(256), 0, st, (c32*)x, n, word, (double*)nullptr, scale_ab, h->fold);
}
// do the adjoints of the native CG stages run in fixed point?  (the windowed kernels carry the integer atomics)
inline bool det_fixed_point(ptycho_handle h) { return h->deterministic && h->use_window && h->ge.ndet <= 512; }
// windowed: the column pass about to run carries the integer atomics; the operand that is not written (probe for the object
// adjoint, object for the probe adjoint) scales the fixed point beside gsrc
int det_begin(ptycho_handle h, ColArgs& ca, bool windowed, const c32* gsrc, long long gcount, const c32* f, const c32* prb, int flg, hipStream_t st,
              const double* known_gmax = nullptr,   // max |gsrc| / max |other| are already on the device (k_cg_absmax format)
              const double* known_omax = nullptr) {
    const Geom& ge = h->ge;
    if (!windowed)
        return fail(PTYCHO_ERR_ARG, h->bs_m ? "option deterministic needs the windowed object adjoint (option window, nprb <= ~1000)"
                                            : "option deterministic needs the windowed adjoint kernels (ndet <= 512)");
    const c32* other = flg == 0 ? prb : f;
    const long long ocount = flg == 0 ? ge.prb_elems() : ge.obj_elems();
    const size_t nobj = (size_t)ge.obj_elems(), nprb = (size_t)ge.prb_elems();
    // option "defer_finish": a gradient that ptycho_cg_obj_grad / prb_grad left in the fixed-point image has not been
    // folded in yet (ptycho_cg_obj_dir / prb_dir do that); another deterministic adjoint would add into the same image
    if (h->det_pending)
        return fail(PTYCHO_ERR_ARG, "a deferred gradient is pending in the fixed-point image: call ptycho_cg_obj_dir / ptycho_cg_prb_dir first");
    if (!h->det_acc) {
        const size_t words = 2 * (nobj > nprb ? nobj : nprb);
        HIP_TRY(hipMalloc((void**)&h->det_acc, words * sizeof(long long)));
        HIP_TRY(hipMemset(h->det_acc, 0, words * sizeof(long long)));
        HIP_TRY(hipMalloc((void**)&h->det_words, 2 * sizeof(double)));
        HIP_TRY(hipMemset(h->det_words, 0, 2 * sizeof(double)));
    }
    if (!known_gmax) launch_absmax(h, gsrc, gcount, 8, h->det_words, nullptr, st);
    if (!known_omax) launch_absmax(h, other, ocount, 4, h->det_words + 1, nullptr, st);
    HIP_TRY(hipGetLastError());
    // additions per element: every position of an angle may touch it, four bilinear taps (object) / once (probe)
    const long long nadd = flg == 0 ? 4ll * ge.nscan : (long long)ge.nscan;
    int head = 1;
    while ((1ll << head) < nadd && head < 30) ++head;
    h->last_det = DetScale{known_gmax ? known_gmax : (const double*)h->det_words,
                           known_omax ? known_omax : (const double*)(h->det_words + 1), ge.ndet, head};
    ca.det_acc = h->det_acc;
    ca.det = h->last_det;
    return PTYCHO_OK;
}
int det_end(ptycho_handle h, c32* f, c32* prb, int flg, hipStream_t st, int add = 1) {
    c32* dst = flg == 0 ? f : prb;
    const long long n = flg == 0 ? h->ge.obj_elems() : h->ge.prb_elems();
    long long g = (n + 255) / 256;
    if (g > (long long)h->n_cu * 4) g = (long long)h->n_cu * 4;
    hipLaunchKernelGGL(k_det_finish, dim3((unsigned)g), dim3(256), 0, st, dst, h->det_acc, n, h->last_det, add);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

inline unsigned small_grid(ptycho_handle h, long long n) {
    long long g = (n + 255) / 256;
    const long long cap = (long long)h->n_cu * 4;
    if (g > cap) g = cap;
    return (unsigned)(g < 1 ? 1 : g);
}

template <int N>
int do_fwd(ptycho_handle h, c32* g, const c32* f, const float* scan, const c32* prb, hipStream_t st) {
    const Geom& ge = h->ge;
    if constexpr (N <= 128) {
        // the tile fits one CU's LDS: one launch, no intermediate in HBM, no position sort (16-byte rows of g)
        if (h->use_tile && ((size_t)g % 16) == 0 && ge.n >= 2 && (long long)ge.nz * ge.n < (1ll << 28)) return launch_fwd_tile<N>(h, g, f, scan, prb, st);
    }
#ifdef PTYCHO_EXPERIMENTS
    if constexpr (N == 256) {
        // single launch, no intermediate in HBM; needs 16-byte aligned object rows
        if (h->use_fused && ge.n % 2 == 0 && ((size_t)f % 16) == 0) return do_fwd_fused(h, g, f, scan, prb, st);
    }
#endif
    const ColPath path = col_path_for<N>(h, COL_FWD, true);
    int rc = col_path_sorts(path, COL_FWD) ? sort_positions(h, scan, st) : (int)PTYCHO_OK;
    if (rc) return rc;
    // The column pass writes straight into g and the row pass transforms g in place, so the
    // forward operator needs no scratch and is issued as one launch pair over all positions.
    ColArgs ca = col_args<N>(h, scan, 0, ge.npos(), path, COL_FWD);
    ca.src = f; ca.dst = g; ca.aux = prb;
    // the row pass's column limits follow the strips (32 columns wide where the pass is split)
    const int C = col_strip_width(path, COL_FWD, ColCfg<N>::C);
    RowArgs ra{};
    ra.src = g; ra.dst = g; ra.table = h->table; ra.tile_index = nullptr;
    ra.nrows = ge.npos() * N; ra.xa = ca.strip0 * C; ra.xb = (ca.strip0 + ca.nstrips) * C; ra.wa = 0; ra.wb = N;
    rc = launch_fwd_cols<N>(h, ca, st, true);
    if (rc) return rc;
    if constexpr (N == 256) {
        if (col_path_split(path)) return launch_rows_split<N, -1>(h, ra, st);
    }
    return launch_rows<N, -1>(h, ra, st);
}

template <int N>
int do_adj(ptycho_handle h, c32* f, const c32* g, const float* scan, c32* prb, int flg, hipStream_t st) {
    constexpr int C = ColCfg<N>::C;
    const Geom& ge = h->ge;
    const long long total = ge.npos();
    const ColMode mode = flg == 0 ? COL_ADJ_OBJ : COL_ADJ_PRB;
    const ColPath path = col_path_for<N>(h, mode, true);
    const RowPath rows = row_path(N, path, mode, h->use_tile, aligned16(g));
    if constexpr (N <= 128) {
        // probe adjoint with the tile in LDS: one launch, g read once, no scratch, no position sort
        if (flg == 1 && h->use_tile && !h->deterministic && ((size_t)g % 16) == 0 && (long long)ge.nz * ge.n < (1ll << 28))
            return launch_adjprb_tile<N>(h, prb, g, scan, f, st);
    }
    // positions are visited in sorted order (angle, column bucket, row): neighbours in the
    // object are neighbours in time, which is what the LDS overlap-add window needs
    int rc = sort_positions(h, scan, st);
    if (rc) return rc;
    if (!h->scratch) {   // the row pass's output (up to 4 GiB), allocated by the first call that gets here
        rc = alloc_scratch(h);
        if (rc) return rc;
    }
    ColArgs det{};
    if (h->deterministic) {
        rc = det_begin(h, det, path != COLS_PLAIN, g, total * N * N, f, prb, flg, st);
        if (rc) return rc;
    }
    for (long long k0 = 0; k0 < total; k0 += h->chunk) {
        const long long k1 = k0 + h->chunk < total ? k0 + h->chunk : total;
        ColArgs ca = col_args<N>(h, scan, k0, k1, path, mode);
        ca.src = h->scratch; ca.dst = flg == 0 ? f : prb; ca.aux = flg == 0 ? prb : f;
        ca.det_acc = det.det_acc; ca.det = det.det;
        RowArgs ra{};
        ra.src = g; ra.dst = h->scratch; ra.table = h->table; ra.tile_index = h->order + k0;
        ra.nrows = (k1 - k0) * N; ra.xa = 0; ra.xb = N; ra.wa = ca.strip0 * C; ra.wb = (ca.strip0 + ca.nstrips) * C;
        if constexpr (N == 256) {
            if (rows == ROWS_SPLIT) rc = launch_rows_split<N, +1>(h, ra, st);
        }
        if constexpr (N <= 128) {
            // whole tiles through LDS, 16 bytes per lane (k_tile.hpp): 0.34 -> 0.047 ms at 16384 x 32^2
            if (rows == ROWS_TILE || rows == ROWS_SLAB) {
                ProfSpan ps(h, K_ROWS_INV, st);
                if constexpr (!is_pow2(N) && N >= 80) {   // 16-row slabs, one wave per workgroup (k_rows_slab)
                    const long long items = (k1 - k0) * (N / 16);
                    const long long cap = (long long)h->n_cu * 10;
                    hipLaunchKernelGGL((k_rows_slab<N, +1>), dim3((unsigned)(items < cap ? items : cap)), dim3(16 * Plan<N>::T), 0, st, g, h->scratch,
                                       (const int*)(h->order + k0), (int)(k1 - k0), (const c32*)h->table);
                } else {
                    hipLaunchKernelGGL((k_rows_tile<N, +1>), dim3(tile_grid<N>(h, k1 - k0)), dim3(TileCfg<N>::NT), 0, st, g, h->scratch,
                                       (const int*)(h->order + k0), (int)(k1 - k0), (const c32*)h->table);
                }
                HIP_TRY(hipGetLastError());
            }
        }
        if (rows == ROWS_PLAIN) rc = launch_rows<N, +1>(h, ra, st);
        if (!rc) rc = launch_adj_cols<N>(h, ca, flg, st, true);
        if (rc) return rc;
    }
    if (h->deterministic) return det_end(h, f, prb, flg, st);
    return PTYCHO_OK;
}

template <int N>
int do_fft2(ptycho_handle h, c32* dst, const c32* src, long long nbatch, int dir, hipStream_t st) {
    constexpr int C = ColCfg<N>::C;
    if constexpr (N <= 128) {
        // the tile fits one CU's LDS: both passes in one launch (k_tile.hpp)
        if (h->use_tile && ((size_t)src % 16) == 0 && ((size_t)dst % 16) == 0 && nbatch < (1ll << 30)) {
            ProfSpan ps(h, K_COLS_PLAIN, st);
            if (dir < 0)
                hipLaunchKernelGGL((k_rows_tile<N, -1, true>), dim3(tile_grid<N>(h, nbatch)), dim3(TileCfg<N>::NT), 0, st, src, dst,
                                   (const int*)nullptr, (int)nbatch, (const c32*)h->table);
            else
                hipLaunchKernelGGL((k_rows_tile<N, +1, true>), dim3(tile_grid<N>(h, nbatch)), dim3(TileCfg<N>::NT), 0, st, src, dst,
                                   (const int*)nullptr, (int)nbatch, (const c32*)h->table);
            HIP_TRY(hipGetLastError());
            return PTYCHO_OK;
        }
    }
    RowArgs ra{};
    ra.src = src; ra.dst = dst; ra.table = h->table; ra.nrows = nbatch * N; ra.tile_index = nullptr;
    ra.xa = 0; ra.xb = N; ra.wa = 0; ra.wb = N;
    int rc = dir < 0 ? launch_rows<N, -1>(h, ra, st) : launch_rows<N, +1>(h, ra, st);
    if (rc) return rc;
    // column pass in place, in slices small enough for 32-bit position indices
    const long long slice = 1 << 20;
    for (long long b0 = 0; b0 < nbatch; b0 += slice) {
        const long long b1 = b0 + slice < nbatch ? b0 + slice : nbatch;
        ColArgs ca = col_args(h, nullptr, 0, b1 - b0, nullptr, C);
        ca.src = dst + (size_t)b0 * N * N; ca.dst = dst + (size_t)b0 * N * N; ca.strip0 = 0; ca.nstrips = N / C;   // every strip
        rc = dir < 0 ? launch_cols<N, -1, M_PLAIN>(h, ca, st) : launch_cols<N, +1, M_PLAIN>(h, ca, st);
        if (rc) return rc;
    }
    return PTYCHO_OK;
}

// ---- detector sizes that are not a power of two (k_generic.hpp) ------------------------------------
template <int M, int DIR>
int launch_lines(ptycho_handle h, const c32* src, c32* dst, long long ntiles, bool columns, const int* tile_index, hipStream_t st) {
    const int n = h->ge.ndet;
    LineArgs a{};
    a.src = src; a.dst = dst; a.table = h->table; a.chirp = h->bs_chirp; a.hfilt = h->bs_hfilt;
    a.nlines = ntiles * n; a.n = n; a.ls = columns ? 1 : n; a.es = columns ? n : 1; a.tile_index = tile_index;
    constexpr int T = Plan<M>::T, B = (256 / T) > 0 ? (256 / T) : 1;
    const long long nb = (a.nlines + B - 1) / B;
    const long long grid = nb < (long long)h->n_cu * 8 ? nb : (long long)h->n_cu * 8;
    {
        ProfSpan ps(h, DIR < 0 ? K_ROWS_FWD : K_ROWS_INV, st);
        hipLaunchKernelGGL((k_lines_bluestein<M, DIR>), dim3((unsigned)grid), dim3(256), 0, st, a);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

template <int M>
int do_fwd_generic(ptycho_handle h, c32* g, const c32* f, const float* scan, const c32* prb, hipStream_t st) {
    const Geom& ge = h->ge;
    const long long total = ge.npos();
    const long long npix = total * ge.ndet * ge.ndet;
    {
        ProfSpan ps(h, K_COLS_FWD, st);
        hipLaunchKernelGGL(k_near_generic, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, f, prb, scan, g, ge, npix);
    }
    HIP_TRY(hipGetLastError());
    int rc = launch_lines<M, -1>(h, g, g, total, false, nullptr, st);
    if (rc) return rc;
    return launch_lines<M, -1>(h, g, g, total, true, nullptr, st);
}

template <int M>
int do_adj_generic(ptycho_handle h, c32* f, const c32* g, const float* scan, c32* prb, int flg, hipStream_t st) {
    const Geom& ge = h->ge;
    const long long total = ge.npos();
    const size_t tile = (size_t)ge.ndet * ge.ndet;
    // object adjoint: LDS overlap-add window over runs of sorted positions (k_adjwin_generic) when the window fits
    const size_t win_bytes = (size_t)(ge.nprb + 8) * (16 + kBucketPx) * sizeof(c32);
    if (!h->scratch) {
        int rc0 = alloc_scratch(h);
        if (rc0) return rc0;
    }
    bool windowed = flg == 0 && h->use_window && win_bytes + sizeof(RunMeta) + 256 <= 160 * 1024;
    if (windowed && win_bytes > 48 * 1024 &&
        hipFuncSetAttribute((const void*)k_adjwin_generic, hipFuncAttributeMaxDynamicSharedMemorySize, (int)win_bytes) != hipSuccess) {
        (void)hipGetLastError();
        windowed = false;
    }
    if (windowed) {
        int rc = sort_positions(h, scan, st);
        if (rc) return rc;
    }
    ColArgs det{};
    if (h->deterministic) {   // per-workgroup sums into the 64-bit fixed-point image (integer atomics), folded in at the end
        int rc = det_begin(h, det, windowed || flg == 1, g, total * (long long)tile, f, prb, flg, st);   // the probe adjoint has no window
        if (rc) return rc;
    }
    for (long long k0 = 0; k0 < total; k0 += h->chunk) {
        const long long k1 = k0 + h->chunk < total ? k0 + h->chunk : total;
        // windowed: the chunk is a range of the SORTED order, its tiles are gathered through order[]
        int rc = launch_lines<M, +1>(h, windowed ? g : g + (size_t)k0 * tile, h->scratch, k1 - k0, false, windowed ? h->order + k0 : nullptr, st);
        if (rc) return rc;
        rc = launch_lines<M, +1>(h, h->scratch, h->scratch, k1 - k0, true, nullptr, st);
        if (rc) return rc;
        if (windowed) {
            ColArgs ca = col_args(h, scan, k0, k1, h->order, 16);
            ca.src = h->scratch; ca.dst = f; ca.aux = prb; ca.strip0 = 0; ca.nstrips = (ge.nprb + 15) / 16;   // strips of the probe
            ca.det_acc = det.det_acc; ca.det = det.det;
            const int np = (int)(k1 - k0);
            const RunSplit rs = split_runs(np, ca.nstrips, h->n_cu * 4, min_seglen(np, ca.nstrips, h->n_cu));
            ProfSpan ps(h, K_COLS_ADJ_OBJ, st);
            hipLaunchKernelGGL(k_adjwin_generic, dim3((unsigned)(ca.nstrips * rs.nseg)), dim3(256), win_bytes, st, ca, rs.seglen);
        } else if (flg == 0) {
            const long long npix = (k1 - k0) * ge.nprb * ge.nprb;
            ProfSpan ps(h, K_COLS_ADJ_OBJ, st);
            hipLaunchKernelGGL(k_adj_obj_generic, dim3((unsigned)((npix + 255) / 256)), dim3(256), 0, st, f, (const c32*)prb, scan,
                               (const c32*)h->scratch, ge, (int)k0, npix);
        } else {
            const int npp = ge.nprb * ge.nprb;
            int groups = (int)((k1 - k0 + 63) / 64);
            if (groups > 1024) groups = 1024;
            const int pgroup = (int)((k1 - k0 + groups - 1) / groups);
            ProfSpan ps(h, K_COLS_ADJ_PRB, st);
            hipLaunchKernelGGL(k_adj_prb_generic, dim3((unsigned)((npp + 255) / 256), (unsigned)groups), dim3(256), 0, st,
                               (const c32*)f, prb, scan, (const c32*)h->scratch, ge, (int)k0, (int)k1, pgroup, det.det_acc, det.det);
        }
        HIP_TRY(hipGetLastError());
    }
    if (h->deterministic) return det_end(h, f, prb, flg, st);
    return PTYCHO_OK;
}

template <int M>
int do_fft2_generic(ptycho_handle h, c32* dst, const c32* src, long long nbatch, int dir, hipStream_t st) {
    int rc = dir < 0 ? launch_lines<M, -1>(h, src, dst, nbatch, false, nullptr, st)
                     : launch_lines<M, +1>(h, src, dst, nbatch, false, nullptr, st);
    if (rc) return rc;
    return dir < 0 ? launch_lines<M, -1>(h, dst, dst, nbatch, true, nullptr, st)
                   : launch_lines<M, +1>(h, dst, dst, nbatch, true, nullptr, st);
}

}  // namespace
