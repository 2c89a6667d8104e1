// host_gauge.hpp -- launchers of the illumination map and the gauge fit / apply kernels (k_gauge.hpp) for checked
// arguments; the exported functions and their argument checks are in ptycho_kernels.hip.
#pragma once

namespace {

static_assert(PTYCHO_GAUGE_WORK_PER_ANGLE == kGaugeMaxBlocks * kGaugeStride, "work rows of ptycho_gauge_fit");

// one workgroup per 64 x 16 tile of every angle's object: the grid of k_illumination and of k_scan_map
dim3 illum_grid(int ptheta, int nz, int n) {
    return dim3((unsigned)((n + kIllTileW - 1) / kIllTileW), (unsigned)((nz + kIllTileH - 1) / kIllTileH), (unsigned)ptheta);
}

int do_illumination(float* out, const float* scan, const c32* probe, int ptheta, int nscan, int nmodes, int nprb, int nz,
                    int n, hipStream_t st) {
    hipLaunchKernelGGL(k_illumination, illum_grid(ptheta, nz, n), dim3(256), 0, st, out, scan, probe, nscan, nmodes, nprb, nz, n);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

// pass 1, its finish, pass 2 (which reads the ramp and the centre from gauge on the device), its finish: four launches
int do_gauge_fit(double* gauge, const c32* psi, const c32* ref, const float* weight, int ptheta, int nz, int n, double* work,
                 hipStream_t st) {
    const int nb = gauge_blocks(nz);
    const dim3 grid((unsigned)nb, (unsigned)ptheta);
    hipLaunchKernelGGL(k_gauge_sums, grid, dim3(256), 0, st, work, psi, ref, weight, nz, n);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_gauge_finish, dim3((unsigned)ptheta), dim3(256), 0, st, gauge, (const double*)work, nb, 1);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_gauge_offset, grid, dim3(256), 0, st, work, psi, ref, weight, nz, n, (const double*)gauge);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_gauge_finish, dim3((unsigned)ptheta), dim3(256), 0, st, gauge, (const double*)work, nb, 2);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

int do_gauge_apply(c32* x, const double* gauge, int ptheta, int ny, int nx, int which, hipStream_t st) {
    const int xb = (nx + 255) / 256;
    const dim3 grid((unsigned)((long long)xb * ny), (unsigned)ptheta);
    hipLaunchKernelGGL(k_gauge_apply, grid, dim3(256), 0, st, x, gauge, ny, nx, xb, which);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

}  // namespace
