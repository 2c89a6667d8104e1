// host_resample.hpp -- launchers of the resampling kernels (k_resample.hpp) for checked arguments; the exported functions
// and their argument checks are in ptycho_kernels.hip.
#pragma once

namespace {

static_assert(PTYCHO_SPLINE_SEGMENT == kRsSeg, "segment length of ptycho_spline_prefilter");
static_assert(PTYCHO_WARP_MIRROR == RS_MIRROR && PTYCHO_WARP_GLOBAL == RS_GLOBAL, "flags of ptycho_warp");

bool resample_sizes_ok(size_t nimg, size_t ny, size_t nx) {
    return nimg >= 1 && nimg <= kRsMaxImages && ny >= 2 && nx >= 2 && ny <= kRsMaxSide && nx <= kRsMaxSide &&
           ny * nx < kRsMaxPixels;
}

// 16-byte accesses: rows of a multiple of four floats and every base on a 16-byte boundary
bool resample_vec(int W, std::initializer_list<const void*> ptrs) {
    if (W % 4 != 0) return false;
    for (const void* p : ptrs)
        if (!aligned16(p)) return false;
    return true;
}

// columns in -> work, rows work -> out: out may be in
template <int ORDER>
int do_spline_prefilter(float* out, const float* in, int nimg, int ny, int nx, int C, float* work, hipStream_t st) {
    double zd[2];
    rs_poles(ORDER, zd);
    const float z0 = (float)zd[0], z1 = (float)zd[1], gain = (float)rs_gain(ORDER);
    const int W = nx * C;
    const bool vec = resample_vec(W, {out, in, work});
    const dim3 cgrid((unsigned)((W + kRsColW - 1) / kRsColW), (unsigned)rs_segments(ny), (unsigned)nimg);
    if (vec) hipLaunchKernelGGL((k_spline_cols<ORDER, true>), cgrid, dim3(256), 0, st, work, in, ny, W, z0, z1, gain);
    else hipLaunchKernelGGL((k_spline_cols<ORDER, false>), cgrid, dim3(256), 0, st, work, in, ny, W, z0, z1, gain);
    HIP_TRY(hipGetLastError());
    const int rows = kRsRowLines / C;
    const dim3 rgrid((unsigned)rs_segments(nx), (unsigned)((ny + rows - 1) / rows), (unsigned)nimg);
    const float* src = work;
    if (C == 1) {
        if (vec) hipLaunchKernelGGL((k_spline_rows<ORDER, 1, true>), rgrid, dim3(256), 0, st, out, src, ny, nx, z0, z1, gain);
        else hipLaunchKernelGGL((k_spline_rows<ORDER, 1, false>), rgrid, dim3(256), 0, st, out, src, ny, nx, z0, z1, gain);
    } else {
        if (vec) hipLaunchKernelGGL((k_spline_rows<ORDER, 2, true>), rgrid, dim3(256), 0, st, out, src, ny, nx, z0, z1, gain);
        else hipLaunchKernelGGL((k_spline_rows<ORDER, 2, false>), rgrid, dim3(256), 0, st, out, src, ny, nx, z0, z1, gain);
    }
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

template <int ORDER>
int do_warp(void* out, const void* coef, const double* xf, int nimg, int ny, int nx, int oh, int ow, int cplx, int flags,
            float cre, float cim, int* path, hipStream_t st) {
    const dim3 grid((unsigned)((ow + kRsTile - 1) / kRsTile), (unsigned)((oh + kRsTile - 1) / kRsTile), (unsigned)nimg);
    if (cplx) hipLaunchKernelGGL((k_warp<ORDER, true>), grid, dim3(256), 0, st, out, coef, xf, ny, nx, oh, ow, flags, cre, cim, path);
    else hipLaunchKernelGGL((k_warp<ORDER, false>), grid, dim3(256), 0, st, out, coef, xf, ny, nx, oh, ow, flags, cre, cim, path);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

int do_moments(double* sums, const float* x, const float* weight, int nimg, int ny, int nx, int cplx, int which,
               double* work, hipStream_t st) {
    const int nb = rs_moment_blocks((long long)ny * nx);
    hipLaunchKernelGGL(k_moments, dim3((unsigned)nb, (unsigned)nimg), dim3(256), 0, st, work, x, weight, ny, nx, cplx, which);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_moments_fold, dim3((unsigned)nimg), dim3(64), 0, st, sums, (const double*)work, nb);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

}  // namespace
