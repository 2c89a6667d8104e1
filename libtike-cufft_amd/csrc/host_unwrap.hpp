// host_unwrap.hpp -- launchers of the phase-unwrapping kernels (k_unwrap.hpp) for checked arguments; the exported
// functions and their argument checks are in ptycho_kernels.hip.
#pragma once

namespace {

static_assert(PTYCHO_UNWRAP_STATE_WORDS == kUnwStateWords, "state words of ptycho_unwrap_*");

bool unwrap_sizes_ok(size_t ptheta, size_t nz, size_t n) {
    return ptheta >= 1 && ptheta <= kUnwMaxAngles && nz >= 2 && n >= 2 && nz < kUnwMaxPixels && n < kUnwMaxPixels &&
           nz * n < kUnwMaxPixels;
}

// 16-byte accesses: rows of a multiple of four floats and every base on a 16-byte boundary
bool unwrap_vec(int n, std::initializer_list<const void*> ptrs) {
    if (n % kUnwVec != 0) return false;
    for (const void* p : ptrs)
        if (p && !aligned16(p)) return false;
    return true;
}

struct UnwGrid {
    long long tiles, flat;
    int ntx;
    dim3 tile_grid, flat_grid;
};
UnwGrid unwrap_grid(int ptheta, int nz, int n) {
    UnwGrid g;
    g.tiles = unwrap_tiles(nz, n);
    g.flat = ((long long)nz * n + 256 * kUnwVec - 1) / (256 * kUnwVec);
    g.ntx = unwrap_tiles_x(n);
    g.tile_grid = dim3((unsigned)g.tiles, (unsigned)ptheta);
    g.flat_grid = dim3((unsigned)g.flat, (unsigned)ptheta);
    return g;
}

int unwrap_scalars(double* state, const double* work, int ptheta, long long rows, long long tiles, int stage, int maxiter,
                   double tol, hipStream_t st) {
    hipLaunchKernelGGL(k_unwrap_scalars, dim3((unsigned)ptheta), dim3(256), 0, st, state, work, rows, tiles, stage, maxiter, tol);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

// setup and its one-workgroup-per-angle fold: two launches
int do_unwrap_begin(float* buf, double* state, const float* phase, const float* weight, int ptheta, int nz, int n,
                    double* work, hipStream_t st) {
    const UnwGrid g = unwrap_grid(ptheta, nz, n);
    const bool vec = unwrap_vec(n, {buf, phase, weight});
    VEC_LAUNCH(k_unwrap_setup, vec, g.tile_grid, st, buf, phase, weight, nz, n, g.ntx, work, (const float*)nullptr);
    return unwrap_scalars(state, work, ptheta, g.tiles, g.tiles, 0, 0, 0.0, st);
}

// four launches per iteration (apply, fold, update, fold) and one more fold that applies the stopping tests, so that an
// angle at maxiter (maxiter = 0 included) is marked even when niter = 0
int do_unwrap_iterate(float* buf, double* state, const float* weight, int ptheta, int nz, int n, int niter, int maxiter,
                      double tol, double* work, hipStream_t st) {
    const UnwGrid g = unwrap_grid(ptheta, nz, n);
    const bool vec = unwrap_vec(n, {buf, weight});
    const size_t plane = (size_t)nz * (size_t)n;
    for (int i = 0; i < niter; ++i) {
        VEC_LAUNCH(k_unwrap_apply, vec, g.tile_grid, st, buf, (const double*)state, weight, nz, n, g.ntx, maxiter, work);
        if (int rc = unwrap_scalars(state, work, ptheta, g.tiles, g.tiles, 1, maxiter, tol, st)) return rc;
        VEC_LAUNCH(k_unwrap_update, vec, g.flat_grid, st, buf, (const double*)state, plane, g.tiles, work);
        if (int rc = unwrap_scalars(state, work, ptheta, g.flat, g.tiles, 2, maxiter, tol, st)) return rc;
    }
    return unwrap_scalars(state, work, ptheta, 0, g.tiles, 4, maxiter, tol, st);
}

// the sums of c, their fold, out: three launches
int do_unwrap_finish(float* out, double* state, const float* buf, const float* phase, const float* weight, int congruent,
                     int ptheta, int nz, int n, double* work, hipStream_t st) {
    const UnwGrid g = unwrap_grid(ptheta, nz, n);
    const bool vec = unwrap_vec(n, {out, buf, phase, weight});
    const size_t plane = (size_t)nz * (size_t)n;
    VEC_LAUNCH(k_unwrap_offset, vec, g.flat_grid, st, buf, phase, weight, plane, g.tiles, work);
    if (int rc = unwrap_scalars(state, work, ptheta, g.flat, g.tiles, 3, 0, 0.0, st)) return rc;
    VEC_LAUNCH(k_unwrap_finish, vec, g.flat_grid, st, out, (const double*)state, buf, phase, plane, congruent);
    return PTYCHO_OK;
}

int do_unwrap_residues(signed char* charge, long long* count, const float* phase, const float* weight, int ptheta, int nz,
                       int n, hipStream_t st) {
    HIP_TRY(hipMemsetAsync(count, 0, (size_t)ptheta * sizeof(long long), st));
    const long long loops = (long long)(nz - 1) * (n - 1);
    const dim3 grid((unsigned)((loops + 255) / 256), (unsigned)ptheta);
    hipLaunchKernelGGL(k_unwrap_residues, grid, dim3(256), 0, st, charge, (unsigned long long*)count, phase, weight, nz, n);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

}  // namespace
