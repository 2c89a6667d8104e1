// adjreg_map.hpp -- the object adjoint's overlap-add window held in registers (k_cols_adjreg, k_cols_window.hpp):
// who owns which window pixel, when a group of rows is retired, and the combine of one position.
//
// Plain C++ like fft_core.hpp (include it first: c32, PTY_FN), so that host_adjreg.cpp can run the very same arithmetic
// for every thread of a workgroup on the host (tests/test_adjreg_cpu.py).
//
// The window is WC = C + kBucketPx object columns by HW = G * RPG object rows.  Thread tid owns column cw = tid % WC of
// the RPG consecutive rows of group g = tid / WC (threads with g >= G own nothing).  Rows are addressed relative to a
// workgroup-uniform anchor: group g holds the object rows == [g RPG, (g + 1) RPG) (mod HW) from the anchor, and the
// oldest live row Ybase only moves by whole groups, so a thread's rows are always consecutive object rows.
#pragma once

namespace pty {

constexpr int kBucketPx = 4;   // BX: column bucket of the sort key, and window slack

template <int N_, int NT_>
struct AdjRegCfg {
    static constexpr int N = N_, NT = NT_;
    static constexpr int C = 16;                        // probe columns per strip (ColCfg<N>::C at 256 and 512)
    static constexpr int WC = C + kBucketPx;            // window columns
    static constexpr int G = NT / WC;                   // row groups
    static constexpr int RPG = (N + G - 2) / (G - 1);   // rows per group: the smallest with G RPG >= N + RPG
    static constexpr int HW = G * RPG;                  // window rows; a position at sy < Ybase + RPG reaches row sy + nprb < Ybase + HW
    // T tile in LDS: detector row i at row i + 1 (rows 0 and N + 1 stay zero), strip column c at column c + kBucketPx.
    // Pitch WC: the kBucketPx zero columns right of a row ARE the zero columns left of the next one.
    // Banks: a ds_write_b64 is served in groups of 16 lanes = the 16 columns of one row, 32 consecutive dwords, no conflict
    // at any pitch.  The combine reads 20 consecutive c32 per group of lanes and 3.2 groups per wave, RPG rows = RPG * 2 * P
    // dwords apart: 960 at 256 and 880 at 512, = 0 and 48 (mod 64).  A 32-lane half of a ds_read_b64 then holds 40 dwords of one
    // group and 24 of the next on overlapping banks: two-way, for every pitch (48 P and 44 P are never = 40 mod 64).
    static constexpr int P = WC;
    static constexpr int COL0 = kBucketPx;
    static constexpr int TILE = (N + 2) * P + kBucketPx;   // elements, with the zero columns right of the last row
    // Retire of a slide by SG = one group goes through an LDS stage of RPG rows (adjreg_stage_slot) and all threads issue the
    // atomics; its 20 owner lanes issuing RPG rows of atomics while the other waves wait at the barrier measured 6 % slower,
    // and so did staging two groups (profiles/r06/adjreg.txt).  Longer slides and the whole window are retired by their owners.
    static constexpr int SG = 1;
    static constexpr int STAGE = SG * RPG * WC;
    static_assert(G >= 2 && HW >= N + RPG, "window too low");
};

struct AdjRegWin {
    int t, X0, Ybase, gb;   // angle (< 0: nothing accumulated yet), first object column, oldest live row and the group that holds it
};

// Groups to retire before the position (angle t, first object column Xa, first object row sy) is combined: the groups that
// end at or below sy, or all G of them when the position does not fit the window and re-anchors it.
template <class Cfg>
PTY_FN int adjreg_retire_count(const AdjRegWin& w, int t, int Xa, int sy) {
    const bool fits = t == w.t && Xa >= w.X0 && Xa + Cfg::C < w.X0 + Cfg::WC && sy >= w.Ybase && sy - w.Ybase < Cfg::HW;
    return fits ? (sy - w.Ybase) / Cfg::RPG : Cfg::G;
}

// Window after nret groups were retired; x0pad = object column of strip column 0 at sx = 0.
template <class Cfg>
PTY_FN void adjreg_advance(AdjRegWin& w, int nret, int t, int sx, int sy, int x0pad) {
    if (nret >= Cfg::G) {
        w.t = t;
        w.X0 = (sx / kBucketPx) * kBucketPx + x0pad;
        w.Ybase = sy;
        w.gb = 0;
    } else {
        w.Ybase += nret * Cfg::RPG;
        w.gb = (w.gb + nret) % Cfg::G;
    }
}

// Place of group g in the window's row order (0: the group at Ybase), and its first object row.
template <class Cfg>
PTY_FN int adjreg_rank(const AdjRegWin& w, int g) {
    const int k = g - w.gb;
    return k < 0 ? k + Cfg::G : k;
}
template <class Cfg>
PTY_FN int adjreg_row0(const AdjRegWin& w, int g) { return w.Ybase + adjreg_rank<Cfg>(w, g) * Cfg::RPG; }

// Stage slot of row r of the group at place `rank`: the staged rows are the object rows Ybase + slot / WC, columns X0 + slot % WC.
template <class Cfg>
PTY_FN int adjreg_stage_slot(int rank, int r, int cw) { return (rank * Cfg::RPG + r) * Cfg::WC + cw; }

// LDS row of detector row i; everything outside the tile lands on one of the two zero rows.
template <class Cfg>
PTY_FN int adjreg_tile_row(int i) {
    const int r = i + 1;
    return r < 0 ? 0 : (r > Cfg::N + 1 ? Cfg::N + 1 : r);
}

// Combine of one position (kernels.cu:73-80) for the thread that owns column cw of group g:
//   acc[r] += T[y][cc] w00 + T[y][cc-1] w01 + T[y-1][cc] w10 + T[y-1][cc-1] w11,  y = Y - sy, cc = cw - (Xa - X0),
// for its rows Y = row0 + r.  RPG + 1 independent reads of two neighbouring c32; no LDS write.
template <class Cfg>
PTY_FN void adjreg_combine(c32* acc, const c32* tile, const AdjRegWin& w, int g, int cw, int Xa, int sy, int pad, float fy, float fx) {
    constexpr int RPG = Cfg::RPG, P = Cfg::P;
    constexpr int B = 4, NB = (RPG + B - 1) / B;   // rows per batch; two batches in flight
    const float w00 = (1.0f - fx) * (1.0f - fy), w01 = fx * (1.0f - fy);
    const float w10 = (1.0f - fx) * fy, w11 = fx * fy;
    const int i0 = adjreg_row0<Cfg>(w, g) - sy + pad;                 // detector row of T[y] for acc[0]
    const c32* tp = tile + (cw + Cfg::COL0 - 1 - (Xa - w.X0));        // T[.][cc - 1]; T[.][cc] is its right neighbour
    const c32* tq = tp + adjreg_tile_row<Cfg>(i0 - 1) * P;
    c32 up0 = tq[1], up1 = tq[0];                                     // T[y-1][cc], T[y-1][cc-1]
    c32 t0[2][B], t1[2][B];
    auto request = [&](int b) {
#pragma unroll
        for (int u = 0; u < B; ++u) {
            if (b * B + u < RPG) {
                const c32* tr = tp + adjreg_tile_row<Cfg>(i0 + b * B + u) * P;
                t0[b & 1][u] = tr[1]; t1[b & 1][u] = tr[0];
            }
        }
        asm volatile("" ::: "memory");   // the compiler keeps the batches in this order: registers for two of them, not for all RPG rows
    };
    request(0);
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        if (b + 1 < NB) request(b + 1);
#pragma unroll
        for (int u = 0; u < B; ++u) {
            if (b * B + u < RPG) {
                acc[b * B + u] = acc[b * B + u] + (t0[b & 1][u] * w00 + t1[b & 1][u] * w01 + up0 * w10 + up1 * w11);
                up0 = t0[b & 1][u]; up1 = t1[b & 1][u];
            }
        }
    }
}

// ---------------------------------------------------------------------------
// Tile ring of k_cols_adjreg<256, split>: the strip tile of the NEXT position (N rows x C columns, 32 KiB) is requested by
// LDS-DMA (global_load_lds_dwordx4: 16 bytes per lane, no register destination) into one LDS segment per wave.  A wave
// requests exactly the rows its own threads consume, so its own wait orders the ring and no barrier is involved.
//   thread tid = (c = tid % C, j0 = tid / C) consumes rows j0 + m T, m < E (Fft::load of a radix-16 step);
//   a wave holds four consecutive j0: 64 rows x 128 B = PIECES requests of 1 KiB;
//   lane L of request i supplies row rr = 8 i + L / 8 of the wave's rows (rr = 4 m + j0 % 4), column pair L % 8;
//   the hardware writes the request lane-linearly (segment + 1 KiB i + 16 L bytes): the image is [64 rows][16 columns],
//   and thread tid finds its element m at word 64 m + tid % 64 of the segment (consecutive lanes, consecutive words).
// ---------------------------------------------------------------------------
template <int N_>
struct AdjRingCfg {
    static constexpr int N = N_, C = 16, E = 16, T = N / E;
    static constexpr int WAVE = 64, NW = T * C / WAVE;   // waves per workgroup
    static constexpr int JW = WAVE / C;                  // j0 values per wave
    static constexpr int PIECES = 8;                     // requests per wave and tile
    static constexpr int PIECE = WAVE * 2;               // elements per request (16 bytes per lane)
    static constexpr int SEG = PIECES * PIECE;           // elements per wave segment
    static constexpr int RING = NW * SEG;                // elements in all
    static constexpr int ROW_STEP = (WAVE / 8 / JW) * T; // source rows between a lane's requests i and i + 1
    static_assert(RING == N * C && SEG == JW * E * C, "the ring holds one strip tile");
};

// source of lane `lane` in request i of wave `wave`: tile row, and first of its two strip columns
template <class R>
PTY_FN int adjring_src_row(int wave, int i, int lane) {
    const int rr = 8 * i + lane / 8;
    return wave * R::JW + rr % R::JW + (rr / R::JW) * R::T;
}
template <class R>
PTY_FN int adjring_src_col(int lane) { return 2 * (lane % 8); }
// ring element the hardware writes that lane's first column to (the second follows it)
template <class R>
PTY_FN int adjring_dst_slot(int wave, int i, int lane) { return wave * R::SEG + i * R::PIECE + 2 * lane; }
// ring element that holds thread tid's point m (tile row tid / C + m T, strip column tid % C)
template <class R>
PTY_FN int adjring_read_slot(int tid, int m) { return (tid / R::WAVE) * R::SEG + m * R::WAVE + tid % R::WAVE; }

}  // namespace pty
