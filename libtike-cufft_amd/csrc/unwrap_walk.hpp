// unwrap_walk.hpp -- host walk of the tile / halo index logic of k_unwrap_setup and k_unwrap_apply (k_unwrap.hpp): for
// every tile the 256 threads stage their own pixels and the halo exactly as the kernels do, then read the four
// neighbours of every owned pixel from the staged slots.  No GPU involved: host_unwrap.cpp and host_dpc.cpp edges call it.
//
// errors counts: pixels owned a number of times other than 1, edges (pairs of neighbouring pixels inside the image)
// visited a number of times other than 1 from either end, global reads or writes outside the image, LDS slots outside
// the tile array, slots that two threads stage, neighbour slots read that no thread of the tile had staged or that hold
// another pixel than the neighbour, and what the hook returns.
#pragma once

#include <vector>

#include "k_unwrap.hpp"

namespace pty {

struct UnwWalk {
    long long errors = 0, tiles = 0, owned = 0, visits = 0;
};

// edge(e, lo, hi) -> errors: once per owned pixel and neighbour inside the image; e: 0 left, 1 right, 2 up, 3 down, the
// order in which the kernels take the four neighbours; lo, hi: the pixels y * n + x that the kernels' slot pair (a, b)
// holds, a the lower slot, i.e. the edge's left / upper pixel first
template <class Edge>
UnwWalk walk_unwrap_tiles(const int nz, const int n, Edge&& edge) {
    UnwWalk w;
    const size_t plane = (size_t)nz * n;
    std::vector<unsigned char> own(plane, 0);
    // edge e of pixel p: the visit of that edge from p's end
    std::vector<unsigned char> seen(plane * 4, 0);
    const int ntx = unwrap_tiles_x(n), nty = unwrap_tiles_y(nz);
    w.tiles = unwrap_tiles(nz, n);
    if (w.tiles != (long long)ntx * nty) ++w.errors;
    const int slots = kUnwLdsH * kUnwLdsW;
    const int dy[4] = {0, 0, -1, 1}, dx[4] = {-1, 1, 0, 0}, ds[4] = {-1, 1, -kUnwLdsW, kUnwLdsW};
    for (long long b = 0; b < w.tiles; ++b) {
        const int by = (int)(b / ntx), bx = (int)(b % ntx);
        // which pixel a slot holds: -2 not staged, -1 staged as "outside the image" (weight 0), else y * n + x
        std::vector<long long> lds(slots, -2);
        auto stage = [&](int y, int x) {
            const int s = unwrap_slot(y, x, by, bx);
            if (s < 0 || s >= slots) { ++w.errors; return; }
            if (lds[s] != -2) ++w.errors;                              // two threads stage one slot
            lds[s] = unwrap_inside(y, x, nz, n) ? (long long)y * n + x : -1;   // the kernels read global memory only if inside
        };
        for (int tid = 0; tid < 256; ++tid) {
            int y, x, hy, hx;
            unwrap_own(tid, by, bx, y, x);
            for (int k = 0; k < kUnwVec; ++k) stage(y, x + k);
            if (unwrap_halo(tid, by, bx, hy, hx)) stage(hy, hx);
        }
        for (int tid = 0; tid < 256; ++tid) {
            int y, x;
            unwrap_own(tid, by, bx, y, x);
            const int have = !(y < nz) ? 0 : (n - x >= kUnwVec ? kUnwVec : (n - x > 0 ? n - x : 0));
            for (int k = 0; k < have; ++k) {
                if (!unwrap_inside(y, x + k, nz, n)) { ++w.errors; continue; }   // a write outside the image
                const long long p = (long long)y * n + (x + k);
                if (own[p] < 255) ++own[p];
                ++w.owned;
                const int s = unwrap_slot(y, x + k, by, bx);
                if (lds[s] != p) ++w.errors;
                for (int e = 0; e < 4; ++e) {
                    const int sn = s + ds[e];
                    if (sn < 0 || sn >= slots || lds[sn] == -2) { ++w.errors; continue; }
                    const bool in = unwrap_inside(y + dy[e], x + k + dx[e], nz, n);
                    const long long q = in ? (long long)(y + dy[e]) * n + (x + k + dx[e]) : -1;
                    if (lds[sn] != q) { ++w.errors; continue; }   // outside: weight 0, the kernels take no difference
                    if (!in) continue;
                    w.errors += edge(e, lds[sn < s ? sn : s], lds[sn < s ? s : sn]);
                    if (seen[(size_t)p * 4 + e] < 255) ++seen[(size_t)p * 4 + e];
                    ++w.visits;
                }
            }
        }
    }
    for (int y = 0; y < nz; ++y)
        for (int x = 0; x < n; ++x) {
            const size_t p = (size_t)y * n + x;
            if (own[p] != 1) ++w.errors;
            for (int e = 0; e < 4; ++e)
                if (seen[p * 4 + e] != (unwrap_inside(y + dy[e], x + dx[e], nz, n) ? 1 : 0)) ++w.errors;
        }
    // every edge once from each end: 2 (nz (n - 1) + (nz - 1) n) visits
    if (w.visits != 2 * ((long long)nz * (n - 1) + (long long)(nz - 1) * n)) ++w.errors;
    if (w.owned != (long long)plane) ++w.errors;
    return w;
}

}  // namespace pty
