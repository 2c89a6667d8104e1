// host_cg.hpp -- the CG stages: work slots, the column passes into / out of them, the fused row stages (one builder
// per epilogue, shared by the public stage entries and the native, device-resident loop), the registration (cross,
// arg-max, zoomed DFT) and the multi-mode helpers.  Included by ptycho_kernels.hip after host_ops.hpp.
namespace {

// ---- CG-stage helpers ----------------------------------------------------------------
inline int slot_a(ptycho_handle h, int k) { return h->compact_modes ? k : 2 * k; }
inline int slot_b(ptycho_handle h, int k) { return h->compact_modes ? h->compact_modes : 2 * k + 1; }
inline bool slot_ready(ptycho_handle h, int slot) { return slot >= 0 && slot < ptycho_handle_s::kSlots && h->work[slot]; }
template <class... S>
int need_slots(ptycho_handle h, S... slots) {   // a stage that reads them: an earlier stage filled every one
    return (... && slot_ready(h, slots)) ? (int)PTYCHO_OK : fail(PTYCHO_ERR_ARG, "work slot is empty");
}
int ensure_work(ptycho_handle h, int slot) {   // called by every stage that is about to write the slot
    if (slot < 0 || slot >= ptycho_handle_s::kSlots) return fail(PTYCHO_ERR_ARG, "work slot out of range");
    h->slot_max_ok[slot] = false;
    if (!h->work[slot]) {
        // kMaxModes spare tiles: the M chunk parts of the shared slot of the compact layout take M ceil(total / M) tiles
        const size_t total = (size_t)h->ge.npos() + kMaxModes;
        HIP_TRY(hipMalloc((void**)&h->work[slot], total * h->ge.ndet * h->ge.ndet * sizeof(c32)));
        HIP_TRY(hipMemset(h->work[slot], 0, total * h->ge.ndet * h->ge.ndet * sizeof(c32)));
    }
    return PTYCHO_OK;
}

// allow_split of the stages' column passes (col_path.hpp): never, the fused row stages transform the whole of x
constexpr bool kCgSplit = false;

// npos_limit > 0: only the first npos_limit positions (natural order = sorted order for whole angles: the sort key is
// angle major) -- the position correction needs angle 0 only (ptycho.py:399-403)
template <int N>
int do_cg_fwd_cols(ptycho_handle h, int slot, const c32* f, const float* scan, const c32* prb, hipStream_t st, long long npos_limit = 0) {
    const long long total = h->ge.npos();
    const ColPath path = col_path_for<N>(h, COL_FWD, kCgSplit);
    int rc = col_path_sorts(path, COL_FWD) ? sort_positions(h, scan, st) : (int)PTYCHO_OK;
    if (rc) return rc;
    ColArgs ca = col_args<N>(h, scan, 0, (npos_limit > 0 && npos_limit < total) ? npos_limit : total, path, COL_FWD);
    ca.src = f; ca.dst = h->work[slot]; ca.aux = prb;
    return launch_fwd_cols<N>(h, ca, st, kCgSplit);
}

// finish: 1 = add the result to f / prb (public entry point: the caller zero-filled it); 0 = store it (no zero fill
// needed); -1 = leave it in the fixed-point image for ptycho_cg_*_dir (deterministic option only)
template <int N>
int do_cg_adj_cols(ptycho_handle h, int slot, c32* f, const float* scan, c32* prb, int flg, hipStream_t st,
                   const double* known_omax = nullptr, int finish = 1) {
    const long long total = h->ge.npos();
    const ColMode mode = flg == 0 ? COL_ADJ_OBJ : COL_ADJ_PRB;
    const ColPath path = col_path_for<N>(h, mode, kCgSplit);
    int rc = sort_positions(h, scan, st);
    if (rc) return rc;
    ColArgs ca = col_args<N>(h, scan, 0, total, path, mode);
    ca.src = h->work[slot]; ca.natural_tiles = 1; ca.dst = flg == 0 ? f : prb; ca.aux = flg == 0 ? prb : f;
    if (h->deterministic) {
        rc = det_begin(h, ca, path != COLS_PLAIN, h->work[slot], total * N * N, f, prb, flg, st,
                       h->slot_max_ok[slot] ? h->slot_maxw + slot : nullptr, known_omax);
        if (rc) return rc;
    }
    rc = launch_adj_cols<N>(h, ca, flg, st, kCgSplit);
    if (!rc && h->deterministic) {
        if (finish < 0) h->det_pending = true;
        else rc = det_end(h, f, prb, flg, st, finish);
    }
    return rc;
}

// The <FW, MASK, MODEL> variant of a fused row stage, one question at a time: MASK where the handle has a measured-pixel
// mask and the stage reads data; the Poisson likelihood where it is set and the stage has variants of its own (PROJECT
// and the line searches); FW where the launch covers the detector.  Every variant has the same launch shape, and none
// but these is instantiated.
// FW (unconditional masked loads): line search 0.292 -> 0.252 ms per pass, cross 1.65 -> 1.61, statistics 0.540 -> 0.517
// (rocprofv3, 4096 x 256^2), projection 0.98 -> 1.01 -- it is always launched predicated and has no full-width variant;
// 8.39 -> 8.33 ms per CG iteration by the wall clock
template <int N, int EP, bool MASK = false, int MODEL = MODEL_GAUSSIAN>
void launch_rows_fused(ptycho_handle h, const RowFusedArgs& a, long long grid, hipStream_t st) {
    if constexpr (!MASK && EP != EP_CROSS) {
        if (h->mask) return launch_rows_fused<N, EP, true, MODEL>(h, a, grid, st);
    }
    if constexpr (MODEL == MODEL_GAUSSIAN && (EP == EP_PROJECT || EP == EP_LINESEARCH || EP == EP_LINESEARCH_M)) {
        if (h->model == MODEL_POISSON_ML) return launch_rows_fused<N, EP, MASK, MODEL_POISSON_ML>(h, a, grid, st);
    }
    if constexpr (EP != EP_PROJECT) {
        if (a.xa == 0 && a.xb == N) {
            hipLaunchKernelGGL((k_rows_fused<N, EP, true, MASK, MODEL>), dim3((unsigned)grid), dim3(256), 0, st, a);
            return;
        }
    }
    hipLaunchKernelGGL((k_rows_fused<N, EP, false, MASK, MODEL>), dim3((unsigned)grid), dim3(256), 0, st, a);
}

template <int N, int EP>
int do_cg_rows(ptycho_handle h, RowFusedArgs a, hipStream_t st) {
    constexpr int C = ColCfg<N>::C;
    constexpr int B = 256 / Plan<N>::T;
    int strip0, nstrips;
    strip_range(h->ge, C, strip0, nstrips);
    a.table = h->table;
    if (a.nrows <= 0) a.nrows = h->ge.npos() * N;   // preset: a range of positions (chunked line search)
    a.xa = strip0 * C; a.xb = (strip0 + nstrips) * C;
    long long nb = (a.nrows + B - 1) / B;
    long long grid = nb < (long long)h->n_cu * 8 ? nb : (long long)h->n_cu * 8;
    {   // small problems: at least 16 batches per workgroup while two workgroups per CU remain -- start-up (twiddle table),
        // reduction and fold are per workgroup (512 positions x 256^2: 1.37 -> 1.27 ms per CG iteration)
        long long want = nb / 16;
        if (want < (long long)h->n_cu * 2) want = (long long)h->n_cu * 2;
        if (want < grid) grid = want;
        if (grid > nb) grid = nb;
    }
    if (grid > h->fold_rows) grid = h->fold_rows;
    a.fold = h->fold;
    a.mask = h->mask;   // read by the MASK variants only
    {
        ProfSpan ps(h, (EP == EP_STATS || EP == EP_STATS_M) ? K_ROWS_STATS : EP == EP_PROJECT ? K_ROWS_PROJECT : (EP == EP_LINESEARCH || EP == EP_LINESEARCH_M) ? K_ROWS_LINESEARCH : K_ROWS_CROSS, st);
        launch_rows_fused<N, EP>(h, a, grid, st);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

template <int N>
int do_cg_argmax(ptycho_handle h, int slot, unsigned long long* best, hipStream_t st, bool zeroed = false, int npos_limit = 0) {
    using CC = ColCfg<N>;
    const int npos = npos_limit > 0 ? npos_limit : (int)h->ge.npos();
    constexpr int nstrips = N / CC::C;
    int ng = (h->n_cu * 8) / nstrips;
    if (ng < 1) ng = 1;
    if (ng > npos) ng = npos;
    if (!zeroed) HIP_TRY(hipMemsetAsync(best, 0, (size_t)npos * sizeof(unsigned long long), st));
    {
        ProfSpan ps(h, K_COLS_ARGMAX, st);
        hipLaunchKernelGGL((k_cols_argmax<N>), dim3((unsigned)(nstrips * ng)), dim3(CC::NT), 0, st,
                           (const c32*)h->work[slot], (const c32*)h->table, best, npos, ng);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

// (CW: round 4 tried the two-probe pass of the CG iteration on 32-column strips in one resident round of workgroups -- 512 threads,
// 140 KiB of LDS, one workgroup per CU --: 8.35 against 8.26 ms per iteration, profiles/r04/cg_experiments.txt; 16 columns stay)
template <int N, int NM, int CW = 0>
int launch_gatherwin_modes(ptycho_handle h, ColArgs a, hipStream_t st) {
    constexpr int NTHREADS = Plan<N>::T * (CW ? CW : ColCfg<N>::C);
    const int np = a.k_end - a.k_begin;
    if (np <= 0 || a.nstrips <= 0) return PTYCHO_OK;
    const RunSplit rs = split_runs(np, a.nstrips, h->n_cu * 4, min_seglen(np, a.nstrips, h->n_cu));
    a.nt = 0;
#ifdef PTY_STAMPS
    a.stamps = h->stamps;
#endif
    {
        ProfSpan ps(h, K_COLS_FWD, st);
        hipLaunchKernelGGL((k_cols_gatherwin<N, M_FWD, false, NM, CW>), dim3((unsigned)(a.nstrips * rs.nseg)), dim3(NTHREADS), 0, st, a, rs.seglen);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

template <int N>
int do_cg_fwd_cols_modes(ptycho_handle h, int nmodes, c32* const* dst, const c32* f, const float* scan, const c32* const* prbs,
                         int k_begin, int k_end, hipStream_t st, const double* skip) {
    int rc = sort_positions(h, scan, st);
    if (rc) return rc;
    ColArgs ca = col_args(h, scan, k_begin, k_end, h->order, ColCfg<N>::C);
    ca.src = f; ca.skip = skip;
    static const int nm_max = exp_env("PTYCHO_HIP_NMMAX", 4);   // comparison knob (2 / 1 modes per pass: profiles/r04/cfg3_experiments.txt)
    int k = 0;
    while (k < nmodes) {
        const int left = nmodes - k;
        if constexpr (WinCfg<N>::fits && N <= 512) {
            if (left >= 4 && nm_max >= 4) {
                for (int j = 0; j < 4; ++j) { ca.auxm[j] = prbs[k + j]; ca.dstm[j] = dst[k + j]; }
                rc = launch_gatherwin_modes<N, 4>(h, ca, st);
                if (rc) return rc;
                k += 4;
                continue;
            }
            if (left >= 2 && nm_max >= 2) {
                for (int j = 0; j < 2; ++j) { ca.auxm[j] = prbs[k + j]; ca.dstm[j] = dst[k + j]; }
                rc = launch_gatherwin_modes<N, 2>(h, ca, st);
                if (rc) return rc;
                k += 2;
                continue;
            }
        }
        // one mode: the single-probe pass, windowed wherever the window fits (as the passes above are, whatever option window says)
        ColArgs cb = ca;
        cb.aux = prbs[k]; cb.dst = dst[k];
        if constexpr (!WinCfg<N>::fits) {
            if (k_begin != 0 || k_end != h->ge.npos()) return fail(PTYCHO_ERR_ARG, "position ranges need the windowed column pass (ndet <= 512)");
            cb.order = nullptr;   // k_cols<FWD> takes the positions as they come
        }
        rc = launch_fwd_cols<N>(h, cb, st, kCgSplit, true);
        if (rc) return rc;
        ++k;
    }
    return PTYCHO_OK;
}

// ---- fused row stages: one builder per epilogue ---------------------------------------------------------------------
// overwrite = 0: the public stage entries, whose callers zero-filled the sums they accumulate into; 1: the native loop,
// where the stage's last workgroup STORES the sums (no zero fill of the state).
int stats_stage(ptycho_handle h, int slot, const void* data, double* sums, int overwrite, hipStream_t st) {
    RowFusedArgs a{};
    a.s1 = h->work[slot]; a.data = (const float*)data; a.sums = sums; a.overwrite = overwrite;
    PTY_DISPATCH(h->ge.ndet, (do_cg_rows<NN, EP_STATS>(h, a, st)));
}

int intensity_stage(ptycho_handle h, int nmodes, void* inten, const void* data, double* sums, hipStream_t st) {
    RowFusedArgs a{};
    for (int k = 0; k < nmodes; ++k) {
        if (int rc = need_slots(h, slot_a(h, k))) return rc;
        a.sm[k] = h->work[slot_a(h, k)];
    }
    a.nmodes = nmodes;
    a.acc1 = (float*)inten; a.data = (const float*)data; a.sums = sums;
    PTY_DISPATCH(h->ge.ndet, (do_cg_rows<NN, EP_STATS_M>(h, a, st)));
}

// inten != nullptr: several probe modes (the summed intensity of all of them; first: the source slot is still unscaled)
int project_stage(ptycho_handle h, int src_slot, int dst_slot, const void* data, const void* inten, const double* ab, int first,
                  double* cost, int overwrite, hipStream_t st) {
    int rc = ensure_work(h, dst_slot);
    if (rc) return rc;
    RowFusedArgs a{};
    a.s1 = h->work[src_slot]; a.out = h->work[dst_slot]; a.data = (const float*)data; a.sums = cost; a.ab = ab; a.overwrite = overwrite;
    a.inten = (const float*)inten;
    a.first = first;
    if (h->deterministic) {   // the stage leaves max |dst slot| on the device for the adjoint column pass that follows
        // option "defer_finish": the pending gradient's fixed-point scale reads the max word of the slot its adjoint consumed; a
        // projection issued before ptycho_cg_obj_dir / prb_dir folded the gradient in would overwrite that word
        if (h->det_pending)
            return fail(PTYCHO_ERR_ARG, "a deferred gradient is pending in the fixed-point image: call ptycho_cg_obj_dir / ptycho_cg_prb_dir first");
        if (!h->slot_maxw) {
            HIP_TRY(hipMalloc((void**)&h->slot_maxw, ptycho_handle_s::kSlots * sizeof(double)));
            HIP_TRY(hipMemset(h->slot_maxw, 0, ptycho_handle_s::kSlots * sizeof(double)));
        }
        a.maxword = h->slot_maxw + dst_slot;   // stored (not accumulated) by the stage's last workgroup
    }
    h->slot_max_ok[dst_slot] = a.maxword != nullptr;
    PTY_DISPATCH(h->ge.ndet, (do_cg_rows<NN, EP_PROJECT>(h, a, st)));
}

// What a line search tries and where its costs go.  state == nullptr: the caller's candidates; else the search on the
// device-resident state of the native loop (ls_on_state): the kernel reads its step lengths from the state.
struct LsSearch {
    const double* ab;
    double gamma0;
    int ncand;
    double* sums;
    double* state;
    int overwrite;
};
inline LsSearch ls_on_state(double* state, const double* ab, int overwrite) {
    return LsSearch{ab, 1.0, kMaxCand, state + PTYCHO_ST_COSTS, state, overwrite};
}
inline void ls_operands(RowFusedArgs& a, const void* data, const void* inten, const LsSearch& s) {
    a.data = (const float*)data; a.inten = (const float*)inten; a.ab = s.ab; a.sums = s.sums; a.st = s.state;
    a.gamma0 = (float)s.gamma0; a.ncand = s.ncand; a.overwrite = s.overwrite;
}

// One probe.  On the state, decide_next >= 0: the pass's last workgroup also replays line_search_sqr on the totals and
// sizes the pass that follows (single GPU); < 0: the caller all-reduces the costs and calls k_cg_ls_decide.
int linesearch_stage(ptycho_handle h, int slot1, int slot2, const void* data, const LsSearch& s, hipStream_t st, int which = 0,
                     int decide_next = -1) {
    if (int rc = need_slots(h, slot1, slot2)) return rc;
    RowFusedArgs a{};
    a.s1 = h->work[slot1]; a.s2 = h->work[slot2];
    ls_operands(a, data, nullptr, s);
    if (s.state) {
        a.decide = decide_next >= 0 ? 1 : 0;
        a.decide_which = which;
        a.decide_gamma_word = which == 0 ? (int)PTYCHO_ST_GAMMA_PSI : (int)PTYCHO_ST_GAMMA_PRB;
        a.decide_next = decide_next;
    }
    PTY_DISPATCH(h->ge.ndet, (do_cg_rows<NN, EP_LINESEARCH>(h, a, st)));
}

// Several probe modes, slot pairs of modes [mode0, mode0 + nmodes) ...
int linesearch_modes_stage(ptycho_handle h, int mode0, int nmodes, const void* data, const void* inten, const LsSearch& s, hipStream_t st) {
    RowFusedArgs a{};
    for (int k = 0; k < nmodes; ++k) {
        if (int rc = need_slots(h, slot_a(h, mode0 + k), slot_b(h, mode0 + k))) return rc;
        a.sm[2 * k] = h->work[slot_a(h, mode0 + k)];
        a.sm[2 * k + 1] = h->work[slot_b(h, mode0 + k)];
    }
    a.nmodes = nmodes;
    ls_operands(a, data, inten, s);
    PTY_DISPATCH(h->ge.ndet, (do_cg_rows<NN, EP_LINESEARCH_M>(h, a, st)));
}

// ... and all modes of one chunk of positions in the compact slot layout (mode k of the chunk at tile k * pc of the shared slot)
int linesearch_chunk_stage(ptycho_handle h, int chunk, const void* data, const LsSearch& s, hipStream_t st) {
    const int M = h->compact_modes;
    const long long total = h->ge.npos();
    const long long pc = (total + h->sort_chunks - 1) / h->sort_chunks;
    const long long p0 = chunk * pc, p1 = (chunk + 1) * pc < total ? (chunk + 1) * pc : total;
    if (p1 <= p0) return PTYCHO_OK;
    const size_t tile = (size_t)h->ge.ndet * h->ge.ndet;
    RowFusedArgs a{};
    for (int k = 0; k < M; ++k) {
        if (int rc = need_slots(h, slot_a(h, k), slot_b(h, 0))) return rc;
        a.sm[2 * k] = h->work[slot_a(h, k)] + (size_t)p0 * tile;
        a.sm[2 * k + 1] = h->work[slot_b(h, 0)] + (size_t)k * pc * tile;
    }
    a.nmodes = M;
    ls_operands(a, (const float*)data + (size_t)p0 * tile, nullptr, s);
    a.nrows = (p1 - p0) * h->ge.ndet;
    PTY_DISPATCH(h->ge.ndet, (do_cg_rows<NN, EP_LINESEARCH_M>(h, a, st)));
}

// slot2 <- slot1 + gamma slot2 and the image product of the registration; gamma on the host, or on the device (gamma_dev).
// angle0: the native loop's call -- angle 0 only (ptycho.py:399-403: fwd(...)[0], scan[0, :] += shifts), and the arg-max
// pass that follows finds its peaks cleared
int cross_stage(ptycho_handle h, int slot1, int slot2, c32* image_product, double gamma, const double* gamma_dev, hipStream_t st,
                bool angle0 = false) {
    if (int rc = need_slots(h, slot1, slot2)) return rc;
    RowFusedArgs a{};
    a.s1 = h->work[slot1]; a.s2 = h->work[slot2]; a.out = h->work[slot2]; a.ip = image_product;
    a.gamma0 = (float)gamma; a.gamma_dev = gamma_dev;
    if (angle0) {
        a.best_zero = h->reg_best; a.nbest = h->ge.nscan;
        a.nrows = (long long)h->ge.nscan * h->ge.ndet;
    }
    h->slot_max_ok[slot2] = false;
    PTY_DISPATCH(h->ge.ndet, (do_cg_rows<NN, EP_CROSS>(h, a, st)));
}
// the public cross stages: image_product == NULL puts it in work slot 2 (free during the position correction)
int cross_public(ptycho_handle h, int slot1, int slot2, double gamma, const double* gamma_dev, void* image_product, hipStream_t st) {
    if (!image_product) {
        int rc = ensure_work(h, 2);
        if (rc) return rc;
        if (slot1 == 2 || slot2 == 2) return fail(PTYCHO_ERR_ARG, "slot 2 is taken by the image product");
        image_product = h->work[2];
    }
    return cross_stage(h, slot1, slot2, (c32*)image_product, gamma, gamma_dev, st);
}

// ---- registration: arg-max of the cross-correlation, then the zoomed DFT around the peak ------------------------------
// zeroed: best was cleared by the CROSS stage; npos_limit > 0: only the first positions (angle 0)
int argmax_stage(ptycho_handle h, int slot, unsigned long long* best, hipStream_t st, bool zeroed = false, int npos_limit = 0) {
    PTY_DISPATCH(h->ge.ndet, (do_cg_argmax<NN>(h, slot, best, st, zeroed, npos_limit)));
}

// scan_add: scan[0, :] += shifts (ptycho.py:403) by the kernel that finds them (native CG stages)
int zoom_impl(ptycho_handle h, const void* image_product, const void* best, const void* vt, const void* lz, int nc, int ups,
              double upsample_factor, void* shifts, float* scan_add, void* stream, int npos_limit = 0) {
    int rc = check_args(h);
    if (rc) return rc;
    if (!image_product) {   // NULL: work slot 2 (see cross_public)
        if ((rc = need_slots(h, 2))) return rc;
        image_product = h->work[2];
    }
    if (!best || !vt || !lz || !shifts) return fail(PTYCHO_ERR_ARG, "null operand");
    const int N = h->ge.ndet;
    const int nthreads = N > 256 ? N : 256;
    if (N % 16 != 0 || N > 1024) return fail(PTYCHO_ERR_ARG, "zoomed DFT kernel needs ndet %% 16 == 0 and ndet <= 1024");
    if (ups < 1 || ups > nthreads || nc < 0 || nc > kZoomRK || !(upsample_factor >= 1.0))
        return fail(PTYCHO_ERR_ARG, "zoomed DFT window, rank split or upsample factor out of range");
    const int npos_all = (int)h->ge.npos();
    const int npos = npos_limit > 0 ? npos_limit : npos_all;
    hipStream_t st = (hipStream_t)stream;
    if (!h->zoom_phase) {   // px, py: complex128 [npos][N] each; coarse shifts: float64 [npos][2]
        HIP_TRY(hipMalloc(&h->zoom_phase, (size_t)npos_all * N * 2 * sizeof(double2) + (size_t)npos_all * 2 * sizeof(double)));
        HIP_TRY(hipMemset(h->zoom_phase, 0, (size_t)npos_all * N * 2 * sizeof(double2) + (size_t)npos_all * 2 * sizeof(double)));
    }
    double2* ppx = (double2*)h->zoom_phase;
    double2* ppy = ppx + (size_t)npos * N;
    double* coarse = (double*)(ppy + (size_t)npos * N);
    {
        ProfSpan ps(h, K_ZOOM, st);
        hipLaunchKernelGGL(k_zoom_prepare, dim3((unsigned)npos), dim3(N < 256 ? N : 256), 0, st,
                           (const unsigned long long*)best, N, ups, upsample_factor, ppx, ppy, coarse);
        static const bool no_mfma = exp_env("PTYCHO_HIP_ZOOM_SCALAR", 0) != 0;   // comparison knob
        auto launch = [&](auto kernel, int nt, size_t lds_bytes) {   // one workgroup of nt threads per position
            hipLaunchKernelGGL(kernel, dim3((unsigned)npos), dim3(nt), lds_bytes, st, (const c32*)image_product, ppx, ppy, (const double*)vt,
                               (const double*)lz, N, nc, ups, (int*)nullptr, coarse, upsample_factor, (double*)shifts, scan_add);
        };
        if (N % 64 == 0 && !no_mfma) {
            if (N <= 256) launch(k_zoom_mfma<256>, 256, 0);
            else if (N <= 512) launch(k_zoom_mfma<512>, 512, 0);
            else launch(k_zoom_mfma<1024>, 1024, 0);
        } else if (N <= 256) launch(k_zoom_argmax<256, 8>, 256, (size_t)N * 8 * sizeof(double2));
        else if (N <= 512) launch(k_zoom_argmax<512, 4>, 512, (size_t)N * 4 * sizeof(double2));
        else launch(k_zoom_argmax<1024, 2>, 1024, (size_t)N * 2 * sizeof(double2));
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

// ---- native CG stages (include/ptycho_hip.h, "device-resident CG iteration") ------------------------------------------
// sizes (groups of 16 step lengths) of the pass that ptycho_cg_ls_next(pass) issues: <= 16 step lengths first (sized from the
// last accepted index), then 16, 32, 64 more: 2^-106 < 1e-32 is covered.  For callers that pay a collective per pass:
// 6 then 7 (32, then the 80 that are left), or 5 (all 112 at once).
constexpr int kLsNext[8] = {0, 1, 2, 4, 0, kLsGroupsMax, 2, 5};

// one line-search pass over slots 0 / 1 on the device-resident state
int ls_pass(ptycho_handle h, const void* data, int use_ab, double* state, hipStream_t st, int which, int decide_next) {
    return linesearch_stage(h, 0, 1, data, ls_on_state(state, use_ab ? state + PTYCHO_ST_A : nullptr, 1), st, which, decide_next);
}

// Column passes of fwd(obj, probe) -> slot_p and fwd(obj, ones) -> slot_o in ONE launch that gathers the object patch
// once per position (k_cols_gatherwin<..., NM = 2>): the position correction's operands (ptycho.py:399-402) ride along
// with the passes the object step makes anyway.  Falls back to two passes where the shared-gather kernel does not apply.
template <int N>
int do_fwd_cols_pair(ptycho_handle h, int slot_p, int slot_o, const c32* f, const float* scan, const c32* prb, const c32* ones, hipStream_t st) {
    c32* dst[2] = {h->work[slot_p], h->work[slot_o]};
    const c32* pr[2] = {prb, ones};
    return do_cg_fwd_cols_modes<N>(h, 2, dst, f, scan, pr, 0, (int)h->ge.npos(), st, nullptr);
}
int fwd_cols_pair(ptycho_handle h, int slot_p, int slot_o, const void* f, const void* scan, const void* prb, const void* ones, hipStream_t st) {
    int rc = ensure_work(h, slot_p);
    if (!rc) rc = ensure_work(h, slot_o);
    if (rc) return rc;
    PTY_DISPATCH(h->ge.ndet, (do_fwd_cols_pair<NN>(h, slot_p, slot_o, (const c32*)f, (const float*)scan, (const c32*)prb, (const c32*)ones, st)));
}
// npos_limit = 0: all positions; the position correction needs angle 0 only (nscan)
int fwd_cols_stage(ptycho_handle h, int slot, const void* f, const void* scan, const void* prb, hipStream_t st, long long npos_limit = 0) {
    int rc = ensure_work(h, slot);
    if (rc) return rc;
    PTY_DISPATCH(h->ge.ndet, (do_cg_fwd_cols<NN>(h, slot, (const c32*)f, (const float*)scan, (const c32*)prb, st, npos_limit)));
}
int adj_cols_stage(ptycho_handle h, int slot, void* f, const void* scan, void* prb, int flg, const double* known_omax, int finish, hipStream_t st) {
    PTY_DISPATCH(h->ge.ndet, (do_cg_adj_cols<NN>(h, slot, (c32*)f, (const float*)scan, (c32*)prb, flg, st, known_omax, finish)));
}

// Gradient of the object (flg 0) / probe (flg 1) from the projected slot 1: zero fill unless the adjoint runs in fixed
// point, where the sums are stored, or stay in the fixed-point image for the *_dir stage (option "defer_finish")
int grad_stage(ptycho_handle h, void* f, const void* scan, void* prb, int flg, const double* known_omax, hipStream_t st) {
    const Geom& ge = h->ge;
    const bool det = det_fixed_point(h);
    if (!det) {   // float atomics accumulate into the gradient
        const size_t n = flg == 0 ? (size_t)ge.obj_elems() : (size_t)ge.prb_elems();
        HIP_TRY(hipMemsetAsync(flg == 0 ? f : prb, 0, n * sizeof(c32), st));
    }
    return adj_cols_stage(h, 1, f, scan, prb, flg, known_omax, det ? (h->defer_finish ? -1 : 0) : 1, st);
}

// Dai-Yuan direction of the object (which = 0: normalised by max |probe|) or the probe (1: by max |psi|, nscan, nmodes):
// the sums, with a deferred gradient folded in from the fixed-point image, then the update, which also resets the line search
void dy_direction(ptycho_handle h, double* state, int which, int first, void* grad, void* grad0, void* dir, long long n, float div2, float mul3,
                  hipStream_t st) {
    const double* maxword = state + (which == 0 ? PTYCHO_ST_MAX_PRB : PTYCHO_ST_MAX_PSI);
    double* dy = state + (which == 0 ? PTYCHO_ST_DY_OBJ : PTYCHO_ST_DY_PRB);
    hipLaunchKernelGGL(k_cg_dy_reduce, dim3(fold_grid(h, n, 4)), dim3(256), 0, st, (c32*)grad, (const c32*)dir, (const c32*)grad0, n, maxword,
                       div2, mul3, dy, first, h->det_pending ? h->det_acc : (long long*)nullptr, h->last_det, h->fold);
    h->det_pending = false;
    hipLaunchKernelGGL(k_cg_dy_update, dim3(small_grid(h, n)), dim3(256), 0, st, (c32*)dir, (c32*)grad0, (const c32*)grad, n, (const double*)dy, first,
                       state, which);
}

// x += gamma d with gamma on the device (state word)
int axpy_state(ptycho_handle h, void* x, const void* d, long long n, const double* gamma, hipStream_t st) {
    hipLaunchKernelGGL(k_cg_axpy, dim3(small_grid(h, n)), dim3(256), 0, st, (c32*)x, (const c32*)d, n, gamma);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

// ---- bodies of the native stage entry points (ptycho_cg_obj_* / prb_* / ls_*), behind their argument checks ----
int obj_begin_native(ptycho_handle h, double* state, const void* psi, const void* scan, const void* prb, const void* ones_prb,
                     const void* data, hipStream_t st) {
    h->native_order = 1;   // the native loop keeps track of scan itself (ptycho_cg_obj_finish invalidates the order)
    h->det_pending = false;
    int rc = ones_prb ? fwd_cols_pair(h, 0, 2, psi, scan, prb, ones_prb, st)   // + slot 2 <- column pass of fwd(psi, 1)
                      : fwd_cols_stage(h, 0, psi, scan, prb, st);
    if (rc) return rc;
    return stats_stage(h, 0, data, state + PTYCHO_ST_A, 1, st);
}

int obj_grad_native(ptycho_handle h, double* state, const void* scan, void* prb, const void* data, void* grad, hipStream_t st) {
    // probe *= a / b (ptycho.py:344) and max |probe| (the gradient normalisation of :356 and the fixed-point scale) in one pass
    launch_absmax(h, (const c32*)prb, h->ge.prb_elems(), 4, state + PTYCHO_ST_MAX_PRB, state + PTYCHO_ST_A, st);
    h->max_prb_valid = true;
    int rc = project_stage(h, 0, 1, data, nullptr, state + PTYCHO_ST_A, 0, state + PTYCHO_ST_COST, 1, st);
    if (rc) return rc;
    return grad_stage(h, grad, scan, prb, 0, state + PTYCHO_ST_MAX_PRB, st);
}

int obj_dir_native(ptycho_handle h, double* state, int first, const void* scan, const void* prb, const void* ones_prb, const void* data,
                   void* grad, void* grad0, void* dpsi, hipStream_t st) {
    if (!h->max_prb_valid) launch_absmax(h, (const c32*)prb, h->ge.prb_elems(), 4, state + PTYCHO_ST_MAX_PRB, nullptr, st);
    h->max_prb_valid = false;
    dy_direction(h, state, 0, first, grad, grad0, dpsi, h->ge.obj_elems(), 0.0f, 0.0f, st);
    int rc = ones_prb ? fwd_cols_pair(h, 1, 3, dpsi, scan, prb, ones_prb, st)   // + slot 3 <- column pass of fwd(dpsi, 1)
                      : fwd_cols_stage(h, 1, dpsi, scan, prb, st);
    if (rc) return rc;
    return ls_pass(h, data, 1, state, st, 0, h->ls_fused_decide ? kLsNext[1] : -1);
}

int ls_begin_native(double* state, int which, hipStream_t st) {
    hipLaunchKernelGGL(k_cg_ls_begin, dim3(1), dim3(1), 0, st, state, which);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}
int ls_decide_native(double* state, int which, int next_groups, hipStream_t st) {
    hipLaunchKernelGGL(k_cg_ls_decide, dim3(1), dim3(1), 0, st, state, which,
                       which == 0 ? (int)PTYCHO_ST_GAMMA_PSI : (int)PTYCHO_ST_GAMMA_PRB, next_groups);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}
int ls_next_native(ptycho_handle h, double* state, int which, int pass, const void* data, int use_ab, hipStream_t st) {
    if (h->ls_fused_decide) {
        // the pass before this call has decided on its own totals and sized this one: just issue it
        if (pass > 3) return pass == 4 ? (int)PTYCHO_OK : fail(PTYCHO_ERR_ARG, "option ls_fused_decide: passes 1, 2, 3, 4 only");
        return ls_pass(h, data, use_ab, state, st, which, kLsNext[pass + 1]);
    }
    int rc = ls_decide_native(state, which, kLsNext[pass], st);
    if (rc || pass == 4) return rc;
    return ls_pass(h, data, use_ab, state, st, which, -1);
}

// psi += gamma dpsi, after the position correction of angle 0 (ptycho.py:399-403) where it is asked for
int obj_finish_native(ptycho_handle h, double* state, int correct_positions, void* psi, const void* dpsi, void* scan, const void* ones_prb,
                      const void* vt, const void* lz, int nc, int ups, double upsample_factor, hipStream_t st) {
    const Geom& ge = h->ge;
    if (correct_positions) {
        if (!ones_prb || !vt || !lz) return fail(PTYCHO_ERR_ARG, "null operand");
        const size_t npos = (size_t)ge.nscan;
        if (!h->reg_ip) {
            HIP_TRY(hipMalloc((void**)&h->reg_ip, npos * ge.ndet * ge.ndet * sizeof(c32)));
            HIP_TRY(hipMalloc((void**)&h->reg_best, npos * sizeof(unsigned long long)));
            HIP_TRY(hipMalloc((void**)&h->reg_shifts, npos * 2 * sizeof(double)));
        }
        // ptycho.py:399-402: tmp1 = fwd(psi, 1), tmp2 = fwd(psi + gamma dpsi, 1) = tmp1 + gamma fwd(dpsi, 1)
        // 2: ptycho_cg_reg_prepare (or ptycho_cg_obj_begin2) left the column pass of tmp1 in slot 2;
        // 3: and ptycho_cg_obj_dir2 the column pass of fwd(dpsi, 1) in slot 3
        const int s1 = correct_positions >= 2 ? 2 : 0, s2 = correct_positions == 3 ? 3 : 1;
        int rc = s1 == 0 ? fwd_cols_stage(h, 0, psi, scan, ones_prb, st, ge.nscan) : (int)PTYCHO_OK;
        if (!rc && s2 == 1) rc = fwd_cols_stage(h, 1, dpsi, scan, ones_prb, st, ge.nscan);
        if (!rc) rc = cross_stage(h, s1, s2, h->reg_ip, 0.0, state + PTYCHO_ST_GAMMA_PSI, st, true);
        if (!rc) rc = argmax_stage(h, s2, h->reg_best, st, true, ge.nscan);
        // the kernel that finds the shifts also adds them to scan[0, :] (ptycho.py:403)
        if (!rc) rc = zoom_impl(h, h->reg_ip, h->reg_best, vt, lz, nc, ups, upsample_factor, h->reg_shifts, (float*)scan, st, ge.nscan);
        if (rc) return rc;
        h->order_scan = nullptr;   // the positions moved: the next column pass sorts again
    }
    return axpy_state(h, psi, dpsi, ge.obj_elems(), state + PTYCHO_ST_GAMMA_PSI, st);
}

int prb_grad_native(ptycho_handle h, double* state, const void* psi, const void* scan, const void* prb, const void* data, void* gprb,
                    hipStream_t st) {
    int rc = fwd_cols_stage(h, 0, psi, scan, prb, st);
    if (rc) return rc;
    // max |psi|: the gradient normalisation of ptycho.py:431 and the fixed-point scale of the probe adjoint
    launch_absmax(h, (const c32*)psi, h->ge.obj_elems(), 4, state + PTYCHO_ST_MAX_PSI, nullptr, st);
    h->max_psi_valid = true;
    rc = project_stage(h, 0, 1, data, nullptr, nullptr, 0, state + PTYCHO_ST_COST2, 1, st);
    if (rc) return rc;
    return grad_stage(h, (void*)psi, scan, gprb, 1, state + PTYCHO_ST_MAX_PSI, st);
}

int prb_dir_native(ptycho_handle h, double* state, int first, double nscan_total, double nmodes, const void* psi, const void* scan,
                   const void* data, void* gprb, void* gprb0, void* dprb, hipStream_t st) {
    if (!h->max_psi_valid) launch_absmax(h, (const c32*)psi, h->ge.obj_elems(), 4, state + PTYCHO_ST_MAX_PSI, nullptr, st);
    h->max_psi_valid = false;
    dy_direction(h, state, 1, first, gprb, gprb0, dprb, h->ge.prb_elems(), (float)nscan_total, (float)nmodes, st);
    int rc = fwd_cols_stage(h, 1, psi, scan, dprb, st);
    if (rc) return rc;
    return ls_pass(h, data, 0, state, st, 1, h->ls_fused_decide ? kLsNext[1] : -1);
}

// ---- several probe modes per column pass; compact slot layout with a chunked line search ----

int fwd_cols_modes_impl(ptycho_handle h, int nmodes, int mode0, const void* f, const void* scan,
                        const void* const* prbs, int into_b, int chunk, void* stream, const double* skip) {
    int rc = check_args(h);
    if (rc) return rc;
    if (!f || !scan || !prbs || nmodes < 1 || mode0 < 0 || mode0 + nmodes > kMaxModes) return fail(PTYCHO_ERR_ARG, "bad operand");
    const long long total = h->ge.npos();
    const size_t tile = (size_t)h->ge.ndet * h->ge.ndet;
    c32* dst[kMaxModes];
    const c32* pr[kMaxModes];
    int k_begin = 0, k_end = (int)total;
    if (into_b) {   // B sub-slots: mode k of the positions of this chunk at tile k * pc of the shared slot
        if (!h->compact_modes || nmodes != h->compact_modes || mode0 != 0 || chunk < 0 || chunk >= h->sort_chunks)
            return fail(PTYCHO_ERR_ARG, "chunked column pass needs the compact slot layout and all modes");
        const long long pc = (total + h->sort_chunks - 1) / h->sort_chunks;
        k_begin = (int)(chunk * pc);
        k_end = (int)((chunk + 1) * pc < total ? (chunk + 1) * pc : total);
        rc = ensure_work(h, slot_b(h, 0));
        if (rc) return rc;
        for (int k = 0; k < nmodes; ++k) dst[k] = h->work[slot_b(h, 0)] + (size_t)k * pc * tile - (size_t)k_begin * tile;
    } else {
        for (int k = 0; k < nmodes; ++k) {
            rc = ensure_work(h, slot_a(h, mode0 + k));
            if (rc) return rc;
            dst[k] = h->work[slot_a(h, mode0 + k)];
        }
    }
    for (int k = 0; k < nmodes; ++k) {
        if (!prbs[k]) return fail(PTYCHO_ERR_ARG, "null probe");
        pr[k] = (const c32*)prbs[k];
    }
    hipStream_t st = (hipStream_t)stream;
    PTY_DISPATCH(h->ge.ndet, (do_cg_fwd_cols_modes<NN>(h, nmodes, dst, (const c32*)f, (const float*)scan, pr, k_begin, k_end, st, skip)));
}

// body of ptycho_cg_ls_obj_chunk: direction column passes of this chunk, all modes side by side in the shared slot (skipped
// once the search is resolved), then their line-search pass; the chunks of one pass accumulate, the first one stores
int ls_obj_chunk_native(ptycho_handle h, double* state, int chunk, const void* dpsi, const void* scan, const void* const* prbs,
                        const void* data, const double* ab, void* stream) {
    int rc = fwd_cols_modes_impl(h, h->compact_modes, 0, dpsi, scan, prbs, 1, chunk, stream, state + PTYCHO_ST_LS_RESOLVED);
    if (rc) return rc;
    return linesearch_chunk_stage(h, chunk, data, ls_on_state(state, ab, chunk == 0 ? 1 : 0), (hipStream_t)stream);
}

// ---- orthogonal probe modes (k_modes.hpp): no handle ----
template <int M>
int do_orthogonalize_modes(c32* const* x, int narr, int ptheta, long long npix, double* v, double* powers, hipStream_t st) {
    hipLaunchKernelGGL((k_mode_gram_eig<M>), dim3((unsigned)ptheta), dim3(256), 0, st, (const c32*)x[0], npix, v, powers);
    HIP_TRY(hipGetLastError());
    if constexpr (M > 1) {
        ModeRotateArgs a{};
        for (int i = 0; i < narr; ++i) a.x[i] = x[i];
        a.v = v;
        a.npix = npix;
        a.blocks = (npix + 255) / 256;
        a.ptheta = ptheta;
        hipLaunchKernelGGL((k_mode_rotate<M>), dim3((unsigned)(a.blocks * ptheta * narr)), dim3(256), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return PTYCHO_OK;
}
// nmodes in [1, kOrthoMaxModes] (the caller checked) to the template argument, every case named once
template <int M = 1>
int orthogonalize_modes(int nmodes, c32* const* x, int narr, int ptheta, long long npix, double* v, double* powers, hipStream_t st) {
    if constexpr (M < kOrthoMaxModes) {
        if (nmodes != M) return orthogonalize_modes<M + 1>(nmodes, x, narr, ptheta, npix, v, powers, st);
    }
    return do_orthogonalize_modes<M>(x, narr, ptheta, npix, v, powers, st);
}

}  // namespace
