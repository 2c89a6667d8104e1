// Host build of the Jacobi eigen solve of k_modes.hpp (jacobi_herm + eig_finish, one thread walking every index).
// Built by tests/test_ortho_cpu.py with clang++ (no GPU involved).  stdin: a sequence of "M" followed by the M x M
// Hermitian matrix as M*M (re, im) pairs, row-major; stdout per matrix: "sweeps", the M eigenvalues (descending), then V
// as M*M (re, im) pairs, row-major (column j = eigenvector of eigenvalue j).
#include <cstdio>
#include <vector>

#include "k_modes.hpp"

using namespace pty;

int main() {
    int M = 0;
    while (std::scanf("%d", &M) == 1) {
        if (M < 1 || M > kOrthoMaxModes) return 2;
        std::vector<double> gr(M * M), gi(M * M), vr(M * M), vi(M * M), out(2 * M * M), lam(M);
        for (int k = 0; k < M * M; ++k)
            if (std::scanf("%lf %lf", &gr[k], &gi[k]) != 2) return 3;
        const HostTeam tm;
        const int sweeps = jacobi_herm(tm, gr.data(), gi.data(), vr.data(), vi.data(), M);
        eig_finish(tm, gr.data(), vr.data(), vi.data(), M, out.data(), out.data() + 1, 2, lam.data());
        std::printf("%d\n", sweeps);
        for (int j = 0; j < M; ++j) std::printf("%.17g\n", lam[j]);
        for (int k = 0; k < M * M; ++k) std::printf("%.17g %.17g\n", out[2 * k], out[2 * k + 1]);
    }
    return 0;
}
