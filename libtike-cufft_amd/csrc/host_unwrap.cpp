// Host build of the tile / halo index logic of k_unwrap_setup and k_unwrap_apply (k_unwrap.hpp): the walk of
// unwrap_walk.hpp with nothing more to check per edge.  Built by tests/test_unwrap_cpu.py with clang++ (no GPU involved).
//   host_unwrap            sweeps nz, n from 2 to a few tile sizes + 1 and prints "host_unwrap: E errors, S shapes"
//   host_unwrap nz n       one shape: "errors tiles owned edge_visits"
// errors counts: pixels owned a number of times other than 1, edges (pairs of neighbouring pixels inside the image) visited
// a number of times other than 1 from either end, global reads or writes outside the image, LDS slots outside the tile
// array, slots that two threads stage, and neighbour slots read that no thread of the tile had staged.
#include <cstdio>
#include <cstdlib>

#include "unwrap_walk.hpp"

using namespace pty;

static UnwWalk walk(const int nz, const int n) {
    return walk_unwrap_tiles(nz, n, [](int, long long, long long) { return 0; });
}

int main(int argc, char** argv) {
    if (argc == 3) {
        const int nz = std::atoi(argv[1]), n = std::atoi(argv[2]);
        if (nz < 2 || n < 2) return 2;
        const UnwWalk w = walk(nz, n);
        std::printf("%lld %lld %lld %lld\n", w.errors, w.tiles, w.owned, w.visits);
        return w.errors ? 1 : 0;
    }
    long long errors = 0, shapes = 0;
    for (int nz = 2; nz <= 3 * kUnwTileH + 1; ++nz)
        for (int n = 2; n <= 3 * kUnwTileW + 1; ++n) {
            errors += walk(nz, n).errors;
            ++shapes;
        }
    std::printf("host_unwrap: %lld errors, %lld shapes\n", errors, shapes);
    return errors ? 1 : 0;
}
