// Host-side check of the tile ring of k_cols_adjreg (AdjRingCfg, adjreg_map.hpp): walks every wave, request and lane of one
// workgroup with the very functions the kernel uses, fills an emulated LDS ring the way the hardware does (a request
// writes 16 bytes per lane, lane-linearly, from a per-lane source address) and reads it back as the threads do.
// Checked at ndet = 256, for the rows of both radix-16 steps (Fft::load<1>: split kernel, Fft::load<0>: un-split):
//   every element of the strip tile is requested exactly once, from a 16-byte-aligned source;
//   every element lands inside its own wave's segment;
//   a lane's requests are ROW_STEP rows apart (the kernel advances a scalar base by that much);
//   every thread's 16 reads return the rows Fft::load names for it, of its own column.
// Built by tests/test_adjdma_cpu.py with clang++ (no GPU involved).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "fft_core.hpp"
#include "adjreg_map.hpp"

using namespace pty;

template <int N, int ST>
static bool check(const char* name) {
    using P = Plan<N>;
    using F = Fft<P, +1>;
    using R = AdjRingCfg<N>;
    constexpr int C = R::C, NT = P::T * C;
    static_assert(P::E == R::E && P::T == R::T, "the ring is cut for the plan's threads");
    long long bad = 0;
    const size_t scratch_base = 4096;   // hipMalloc'ed: at least 256-byte aligned; any multiple of 16 serves the check
    for (int strip = 0; strip < N / C; ++strip) {
        const int x0 = strip * C;
        // the tile in global memory: element (row, column) carries its own coordinates
        std::vector<int> ring(R::RING, -1);      // row * C + strip column of the element a slot received
        std::vector<int> requested(N * C, 0);
        for (int wave = 0; wave < R::NW; ++wave)
            for (int i = 0; i < R::PIECES; ++i)
                for (int lane = 0; lane < R::WAVE; ++lane) {
                    const int row = adjring_src_row<R>(wave, i, lane), col = adjring_src_col<R>(lane);
                    const int slot = adjring_dst_slot<R>(wave, i, lane);
                    if (row < 0 || row >= N || col < 0 || col + 1 >= C) { ++bad; continue; }
                    const size_t src = scratch_base + ((size_t)row * N + x0 + col) * sizeof(c32);
                    if (src % 16 != 0) ++bad;
                    if (row != adjring_src_row<R>(wave, 0, lane) + i * R::ROW_STEP) ++bad;
                    // the hardware's destination: segment of the wave + 1 KiB per request + 16 bytes per lane
                    if (slot != wave * R::SEG + i * R::PIECE + 2 * lane) ++bad;
                    if (slot < wave * R::SEG || slot + 1 >= (wave + 1) * R::SEG) { ++bad; continue; }
                    for (int e = 0; e < 2; ++e) {
                        if (ring[slot + e] != -1) ++bad;
                        ring[slot + e] = row * C + col + e;
                        ++requested[row * C + col + e];
                    }
                }
        for (int e = 0; e < N * C; ++e)
            if (requested[e] != 1) ++bad;
        // read-out: thread tid's point m is the m-th row Fft::load asks for
        for (int tid = 0; tid < NT; ++tid) {
            const int c = tid % C, j0 = tid / C;
            F fft;
            c32 rows[P::E];
            fft.template load<ST>(rows, j0, [&](int i) { return c32{(float)i, 0.0f}; });
            for (int m = 0; m < P::E; ++m) {
                const int slot = adjring_read_slot<R>(tid, m);
                if (slot < (tid / R::WAVE) * R::SEG || slot >= (tid / R::WAVE + 1) * R::SEG) { ++bad; continue; }
                if (ring[slot] != (int)rows[m].x * C + c) ++bad;
            }
        }
    }
    std::printf("N=%d %s waves=%d requests=%d segment=%zu B ring=%zu B row_step=%d bad=%lld %s\n", N, name, R::NW, R::PIECES,
                (size_t)R::SEG * sizeof(c32), (size_t)R::RING * sizeof(c32), R::ROW_STEP, bad, bad == 0 ? "ok" : "BAD");
    return bad == 0;
}

int main() {
    bool ok = true;
    ok = check<256, 1>("split") && ok;
    ok = check<256, 0>("unsplit") && ok;
    std::printf("%s\n", ok ? "OK" : "FAIL");
    return ok ? 0 : 1;
}
