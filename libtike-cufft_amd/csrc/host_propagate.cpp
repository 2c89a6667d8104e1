// Host build of the plain C++ of k_propagate.hpp: the phase of the transfer function (prop_turns) against a long double
// evaluation, and the arithmetic that says which threads of k_prop_tile<N> reduce together (PropCfg, prop_group).  Built by
// tests/test_propagate_cpu.py with clang++ (no GPU involved).  Prints "host_propagate: P phases, G threads, 0 errors".
//
// Phases.  For |k| <= 1024, |zl| up to 1e9 and q on both sides of 1 the reference forms q0 k2 in double, as the kernel
// does (q is an input of both), and everything after it in long double: -zl q / 2, or -zl q / (1 + sqrt(1 - q)) (the form
// zl (sqrt(1 - q) - 1) would cost the reference itself zl 1e-19 turns).  The kernel's four roundings after q (1 - q, the
// root, the sum, the quotient) and the product move t by a few eps of the unreduced phase: the bound is
// 8 eps |t| + eps turns, compared modulo one turn.
// The evanescent decision (q > 1) must be the same.
//
// Groups.  For every tile size: every thread of the workgroup lies in exactly one (tile, group); a group has GW members,
// one of them with r = 0; a tile has NG groups; every xor partner tid ^ o, o < GW, lies in the same group and the same
// wave of 64; the tile index agrees with the kernels' tid / TT.
#include <cfloat>
#include <cmath>
#include <cstdio>
#include <vector>

#include "fft_core.hpp"
#include "frame_part.hpp"

using namespace pty;

namespace {
#include "k_propagate.hpp"
}

static long long check_phases(long long& count) {
    long long errors = 0;
    const int ks[] = {0, 1, 2, 3, 7, 8, 31, 64, 100, 255, 511, 512, 1000, 1023, 1024};
    const double zls[] = {0.0, 1.0, -1.0, 0.3, 1234.5678, -98765.4321, 1e7, -1e7, 3.3e8, 1e9, -1e9};
    // q0 such that the corner (1024, 1024) has q = 2: the band straddles 1; and paraxial values
    const double q0s[] = {0.0, 1e-12, 3.7e-9, 1e-7, 4.76837158203125e-07, 9.5367431640625e-07, 1.1e-6, 1e-3, 0.25, 1.0, 3.0};
    for (const int aky : ks)
        for (const int akx : ks)
            for (int sy = -1; sy <= 1; sy += 2)
                for (const double q0 : q0s)
                    for (const double zl : zls)
                        for (int method = 0; method < 2; ++method) {
                            const int ky = sy * aky, kx = -sy * akx;
                            double t = 0.0;
                            const bool ok = prop_turns(method, zl, q0, ky, kx, t);
                            const double q = q0 * (double)((long long)ky * ky + (long long)kx * kx);
                            ++count;
                            const bool want_ok = method == 0 || q <= 1.0;
                            if (ok != want_ok) { ++errors; continue; }
                            if (!ok) {
                                if (t != 0.0) ++errors;
                                continue;
                            }
                            const long double ql = q, zll = zl;
                            const long double full = method == 0 ? -0.5L * zll * ql : -zll * ql / (1.0L + sqrtl(1.0L - ql));
                            long double diff = (long double)t - full;
                            diff -= rintl(diff);
                            const long double tol = 8.0L * DBL_EPSILON * fabsl(full) + DBL_EPSILON;
                            if (!(fabsl(diff) <= tol) || !(std::fabs(t) <= 0.5)) ++errors;
                        }
    // index -> frequency: numpy.fft.fftfreq(s) * s
    for (int s = 1; s <= 2048; ++s)
        for (int i = 0; i < s; ++i) {
            const int want = i < (s + 1) / 2 ? i : i - s;
            if (prop_freq(i, s) != want) ++errors;
        }
    return errors;
}

template <int N>
static long long check_groups(long long& count) {
    using PC = PropCfg<N>;
    long long errors = 0;
    std::vector<int> members(PC::TPW * PC::NG, 0), leaders(PC::TPW * PC::NG, 0);
    if (PC::NT != PC::TT * PC::TPW || PC::NG * PC::GW != PC::TT || PC::GW > 64 || PC::NT > 1024) ++errors;
    if (PC::NG > 1 && PC::TPW != 1) ++errors;   // the LDS fold of the groups assumes the tile owns the workgroup
    for (int tid = 0; tid < PC::NT; ++tid) {
        int w, g, r;
        prop_group(tid, PC::TT, PC::GW, w, g, r);
        ++count;
        if (w != tid / PC::TT || w < 0 || w >= PC::TPW || g < 0 || g >= PC::NG || r < 0 || r >= PC::GW) { ++errors; continue; }
        ++members[w * PC::NG + g];
        if (r == 0) ++leaders[w * PC::NG + g];
        if (r != (tid & 63) % PC::GW) ++errors;   // the group starts at a multiple of GW inside its wave
        for (int o = 1; o < PC::GW; ++o) {
            const int other = tid ^ o;
            int w2, g2, r2;
            if (other >= PC::NT || other / 64 != tid / 64) { ++errors; continue; }
            prop_group(other, PC::TT, PC::GW, w2, g2, r2);
            if (w2 != w || g2 != g) ++errors;
        }
    }
    for (size_t k = 0; k < members.size(); ++k)
        if (members[k] != PC::GW || leaders[k] != 1) ++errors;
    return errors;
}

int main() {
    long long phases = 0, threads = 0, errors = check_phases(phases);
    errors += check_groups<16>(threads) + check_groups<32>(threads) + check_groups<48>(threads) + check_groups<64>(threads) +
              check_groups<80>(threads) + check_groups<96>(threads) + check_groups<112>(threads) + check_groups<128>(threads);
    std::printf("host_propagate: %lld phases, %lld threads, %lld errors\n", phases, threads, errors);
    return errors ? 1 : 0;
}
