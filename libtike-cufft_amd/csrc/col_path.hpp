// col_path.hpp -- which column-pass kernel, and which row pass beside it, an operator or a CG stage runs at a detector size
// with a Stockham plan.  The one statement of the rule: launch_fwd_cols / launch_adj_cols (host_ops.hpp) switch on it, and
// host_colpath.cpp sweeps it on the CPU against the table of every case.  Plain C++ (no HIP types); rules, not launchers.
#pragma once

namespace pty {

enum ColMode { COL_FWD, COL_ADJ_OBJ, COL_ADJ_PRB };

enum ColPath {               // named after the kernels (k_cols_plain.hpp, k_cols_window.hpp)
    COLS_PLAIN,              // k_cols<MODE>: no window; the adjoints add with one atomic per tap
    COLS_GATHERWIN,          // k_cols_gatherwin<FWD / ADJ_PRB>: object strip in an LDS window
    COLS_ADJWIN,             // k_cols_adjwin: overlap-add window in LDS
    COLS_ADJREG,             // k_cols_adjreg: overlap-add window in registers
    COLS_GATHERWIN_SPLIT,    // ndet 256, one radix-16 step of the DFT over y runs in the row pass (k_rows_split)
    COLS_ADJREG_SPLIT
};

constexpr int kSplitFwdC = 32;   // strip width of the split forward pass; every other path takes ColCfg<N>::C

// fits: WinCfg<N>::fits; use_window, use_split: the handle's options; allow_split: the caller takes a row pass that does
// a step of the DFT over y (the operators do; the fused row stages of the CG transform the whole of x, so they do not)
constexpr ColPath col_path(int N, bool fits, bool use_window, bool use_split, bool allow_split, ColMode mode) {
    if (!fits || !use_window) return COLS_PLAIN;
    const bool split = N == 256 && use_split && allow_split;
    if (mode == COL_ADJ_OBJ) return N == 256 ? (split ? COLS_ADJREG_SPLIT : COLS_ADJREG) : N == 512 ? COLS_ADJREG : COLS_ADJWIN;
    return split ? COLS_GATHERWIN_SPLIT : COLS_GATHERWIN;
}

constexpr bool col_path_split(ColPath p) { return p == COLS_GATHERWIN_SPLIT || p == COLS_ADJREG_SPLIT; }
// the windowed kernels and both plain adjoints walk the sorted order; only the plain forward pass takes the positions as they come
constexpr bool col_path_sorts(ColPath p, ColMode mode) { return p != COLS_PLAIN || mode != COL_FWD; }
// detector columns per strip (c: ColCfg<N>::C)
constexpr int col_strip_width(ColPath p, ColMode mode, int c) { return p == COLS_GATHERWIN_SPLIT && mode == COL_FWD ? kSplitFwdC : c; }

// The row pass beside the column pass.  The forward row pass runs in place on g; the adjoint's reads g (16-byte aligned:
// whole tiles through LDS, k_tile.hpp) and writes the chunk scratch.
enum RowPath {
    ROWS_PLAIN,   // k_rows
    ROWS_SPLIT,   // k_rows_split, with the split column passes
    ROWS_TILE,    // k_rows_tile: adjoint, ndet <= 128, option tile
    ROWS_SLAB     // k_rows_slab: ... at 80, 96, 112 (16-row slabs, one wave per workgroup)
};
constexpr RowPath row_path(int N, ColPath p, ColMode mode, bool use_tile, bool g_aligned16) {
    if (col_path_split(p)) return ROWS_SPLIT;
    if (mode == COL_FWD || N > 128 || !use_tile || !g_aligned16) return ROWS_PLAIN;
    return (N & (N - 1)) != 0 && N >= 80 ? ROWS_SLAB : ROWS_TILE;
}

}  // namespace pty
