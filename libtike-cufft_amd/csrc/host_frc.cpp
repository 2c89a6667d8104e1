// Host build of the ring enumeration of k_frc.hpp (frc_ring_row, walked over the rows exactly as k_frc_rings walks them).
// Built by tests/test_frc_cpu.py with clang++ (no GPU involved).  stdin: crop sides S; stdout per S: "S errors n_0 ..
// n_{S/2}", where errors counts the pixels visited outside the DFT's frequencies, visited in a ring other than
// rint(hypot(fy, fx)), or visited a number of times other than 1 (rint(hypot) <= S / 2) or 0 (beyond), and n_k is the
// number of pixels the enumeration put in ring k.
#include <cmath>
#include <cstdio>
#include <vector>

#include "k_frc.hpp"

using namespace pty;

int main() {
    int s = 0;
    while (std::scanf("%d", &s) == 1) {
        if (!frc_size_ok(s)) return 2;
        const int K = frc_rings(s), fmin = frc_fmin(s), fmax = frc_fmax(s);
        std::vector<int> visits((size_t)s * s, 0);
        std::vector<long long> count(K, 0);
        long long errors = 0;
        for (int k = 0; k < K; ++k) {
            const int row_lo = -k > fmin ? -k : fmin, row_hi = k < fmax ? k : fmax;
            for (int fy = row_lo; fy <= row_hi; ++fy) {
                int iv[4];
                frc_ring_row(k, fy, s, iv[0], iv[1], iv[2], iv[3]);
                for (int h = 0; h < 2; ++h) {
                    for (int fx = iv[2 * h]; fx <= iv[2 * h + 1]; ++fx) {
                        if (fx < fmin || fx > fmax) {
                            ++errors;
                            continue;
                        }
                        if ((int)std::rint(std::hypot((double)fy, (double)fx)) != k) ++errors;
                        ++visits[(size_t)(fy < 0 ? fy + s : fy) * s + (fx < 0 ? fx + s : fx)];
                        ++count[k];
                    }
                }
            }
        }
        for (int fy = fmin; fy <= fmax; ++fy)
            for (int fx = fmin; fx <= fmax; ++fx) {
                const int want = std::rint(std::hypot((double)fy, (double)fx)) <= s / 2 ? 1 : 0;
                if (visits[(size_t)(fy < 0 ? fy + s : fy) * s + (fx < 0 ? fx + s : fx)] != want) ++errors;
            }
        std::printf("%d %lld", s, errors);
        for (int k = 0; k < K; ++k) std::printf(" %lld", count[k]);
        std::printf("\n");
    }
    return 0;
}
