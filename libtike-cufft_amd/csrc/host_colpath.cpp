// Host sweep of col_path / row_path (col_path.hpp): every detector size with a Stockham plan x option window x option split
// x "the caller allows split" x mode, against the tables below.  The tables are the ladders that do_fwd, do_adj (host_ops.hpp)
// and do_cg_fwd_cols, do_cg_adj_cols, do_cg_fwd_cols_modes (host_cg.hpp) each wrote out before the rule existed, one row per
// branch; they are what a review of a new path reads.  Then the invariants those ladders only implied.
// No GPU involved; prints OK and exits 0, or the cases that differ and exits 1.
#include <cstdio>

#include "col_path.hpp"

using namespace pty;

// the sizes, with WinCfg<N>::fits (the LDS window of k_cols_window.hpp fits 160 KiB) and ColCfg<N>::C (columns per strip)
struct Size { int N; bool fits; int C; };
static const Size kSizes[] = {{16, true, 16},  {32, true, 32},  {48, true, 48},  {64, true, 64},   {80, true, 16},
                              {96, true, 16},  {112, true, 16}, {128, true, 32}, {192, true, 16},  {256, true, 16},
                              {512, true, 16}, {1024, false, 16}, {2048, false, 8}};

// Column pass.  Options: 1 on, 0 off, -1 either.  The first row that matches a case is the expected answer.
struct ColRow { int n_lo, n_hi, window, split, allow; ColPath fwd, obj, prb; };
static const ColRow kCols[] = {
    // ndet     window split allow   forward               object adjoint     probe adjoint
    {1024, 2048, -1,   -1,   -1,     COLS_PLAIN,           COLS_PLAIN,        COLS_PLAIN},             // the window does not fit
    {16,   512,   0,   -1,   -1,     COLS_PLAIN,           COLS_PLAIN,        COLS_PLAIN},             // option window off
    {256,  256,   1,    1,    1,     COLS_GATHERWIN_SPLIT, COLS_ADJREG_SPLIT, COLS_GATHERWIN_SPLIT},   // the operators at 256
    {256,  512,   1,   -1,   -1,     COLS_GATHERWIN,       COLS_ADJREG,       COLS_GATHERWIN},         // window in registers (launch_adjwin)
    {16,   192,   1,   -1,   -1,     COLS_GATHERWIN,       COLS_ADJWIN,       COLS_GATHERWIN},         // window in LDS
};

// Row pass of the adjoints (inverse, g -> scratch).  tile: option tile and g 16-byte aligned.
struct RowRow { int n_lo, n_hi, split_cols, tile; RowPath rows; };
static const RowRow kRows[] = {
    // ndet     split  tile
    {256,  256,  1,    -1,   ROWS_SPLIT},   // beside the split column passes
    {80,   112,  0,     1,   ROWS_SLAB},    // 80, 96, 112: sizes with an odd factor from 80 up (48 takes whole tiles)
    {16,   128,  0,     1,   ROWS_TILE},
    {16,   2048, 0,    -1,   ROWS_PLAIN},
};

static bool is(int want, bool have) { return want < 0 || (want != 0) == have; }

int main() {
    long long cases = 0, errors = 0;
    const ColMode modes[] = {COL_FWD, COL_ADJ_OBJ, COL_ADJ_PRB};
    const char* mode_name[] = {"FWD", "ADJ_OBJ", "ADJ_PRB"};
    for (const Size& s : kSizes)
        for (int window = 0; window < 2; ++window)
            for (int split = 0; split < 2; ++split)
                for (int allow = 0; allow < 2; ++allow)
                    for (ColMode m : modes) {
                        const ColPath p = col_path(s.N, s.fits, window, split, allow, m);
                        const ColRow* row = nullptr;
                        for (const ColRow& r : kCols)
                            if (!row && s.N >= r.n_lo && s.N <= r.n_hi && is(r.window, window) && is(r.split, split) && is(r.allow, allow)) row = &r;
                        int bad = !row || p != (m == COL_FWD ? row->fwd : m == COL_ADJ_OBJ ? row->obj : row->prb);
                        // what the ladders only implied
                        const bool windowed = p != COLS_PLAIN;
                        bad += col_path_split(p) && !(s.N == 256 && window && split && allow);           // split only at 256, with the window
                        bad += (p == COLS_ADJREG || p == COLS_ADJREG_SPLIT) && !((s.N == 256 || s.N == 512) && m == COL_ADJ_OBJ);
                        bad += (p == COLS_ADJWIN) && m != COL_ADJ_OBJ;
                        bad += (m == COL_ADJ_OBJ) && (p == COLS_GATHERWIN || p == COLS_GATHERWIN_SPLIT);
                        bad += windowed && !(s.fits && window);                                          // no window where it does not fit
                        const int w = col_strip_width(p, m, s.C);
                        bad += w != ((m == COL_FWD && p == COLS_GATHERWIN_SPLIT) ? 32 : s.C);            // 32 columns: the split forward only
                        bad += col_path_sorts(p, m) != (m != COL_FWD || windowed);                      // the plain forward alone does not sort
                        // the row pass beside it
                        for (int tile = 0; tile < 2; ++tile)
                            for (int aligned = 0; aligned < 2; ++aligned) {
                                const RowPath rp = row_path(s.N, p, m, tile, aligned);
                                RowPath want = ROWS_PLAIN;
                                if (m == COL_FWD) want = col_path_split(p) ? ROWS_SPLIT : ROWS_PLAIN;   // do_fwd: in place on g
                                else {
                                    const RowRow* rr = nullptr;
                                    for (const RowRow& r : kRows)
                                        if (!rr && s.N >= r.n_lo && s.N <= r.n_hi && is(r.split_cols, col_path_split(p)) && is(r.tile, tile && aligned)) rr = &r;
                                    bad += !rr;
                                    if (rr) want = rr->rows;
                                }
                                bad += rp != want;
                                bad += (rp == ROWS_SPLIT) != col_path_split(p);
                                ++cases;
                            }
                        if (bad) std::printf("N=%d window=%d split=%d allow=%d %s: path %d, %d errors\n", s.N, window, split, allow, mode_name[m], (int)p, bad);
                        errors += bad;
                        ++cases;
                    }
    std::printf("host_colpath: %lld cases, %lld errors\n", cases, errors);
    if (!errors) std::printf("OK\n");
    return errors ? 1 : 0;
}
