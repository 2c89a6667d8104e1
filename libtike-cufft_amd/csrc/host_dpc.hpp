// host_dpc.hpp -- launchers of the frame-moment, scan-map and gradient-integration kernels (k_dpc.hpp) for checked
// arguments; the exported functions and their argument checks are in ptycho_kernels.hip.
#pragma once

namespace {

// the pass, then the fold of the wave tiles (FrameFold, host_handle.hpp); there is no pixel part
int do_frame_moments(double* moments, const float* data, const unsigned char* mask, double darkfield, long long ptheta,
                     long long nscan, long long ndet, double* work, hipStream_t st) {
    const long long npix = ndet * ndet;
    const FrameFold<MomPart> f(moments, nullptr, work, ptheta, nscan, npix);
    const MomArgs a{f.fpart, data, mask, darkfield >= 0.0 ? darkfield * darkfield : -1.0, npix, f.p.nwt, (int)nscan,
                    (int)f.p.flen, (int)ndet};
    // 16-byte loads: every frame starts on a multiple of four pixels and the array on 16 bytes
    VEC_LAUNCH(k_frame_moments, npix % MomPart::kLanePix == 0 && aligned16(data), f.grid(), st, a);
    return f.fold(k_frame_moments_fold, 0, st);
}

// the copy of scan without the excluded positions (if keep is given), the weight by k_illumination itself, the channels
// (raw: the numerators as they are, not divided by the weight)
int do_scan_map(float* weight, float* out, const float* values, const unsigned char* keep, const float* scan,
                const c32* probe, int ptheta, int nscan, int nval, int nmodes, int nprb, int nz, int n, int raw, float* work,
                hipStream_t st) {
    if (keep) {
        const size_t count = (size_t)ptheta * (size_t)nscan;
        hipLaunchKernelGGL(k_scan_keep, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, work, scan, keep, count);
        HIP_TRY(hipGetLastError());
        scan = work;
    }
    if (int rc = do_illumination(weight, scan, probe, ptheta, nscan, nmodes, nprb, nz, n, st)) return rc;
    const dim3 grid = illum_grid(ptheta, nz, n);
#define MAP_LAUNCH(NV) \
    hipLaunchKernelGGL(k_scan_map<NV>, grid, dim3(256), 0, st, out, (const float*)weight, values, scan, probe, nscan, nmodes, nprb, nz, n, raw)
    switch (nval) {
        case 1: MAP_LAUNCH(1); break;
        case 2: MAP_LAUNCH(2); break;
        case 3: MAP_LAUNCH(3); break;
        default: MAP_LAUNCH(4); break;
    }
#undef MAP_LAUNCH
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

// the unwrapper's setup with the gradient as the source of the edge differences, and its fold: two launches
int do_integrate_begin(float* buf, double* state, const float* gy, const float* gx, const float* weight, int ptheta, int nz,
                       int n, double* work, hipStream_t st) {
    const UnwGrid g = unwrap_grid(ptheta, nz, n);
    const bool vec = unwrap_vec(n, {buf, gy, gx, weight});
    if (vec) hipLaunchKernelGGL((k_unwrap_setup<true, UnwGradSrc>), g.tile_grid, dim3(256), 0, st, buf, gy, weight, nz, n, g.ntx, work, gx);
    else hipLaunchKernelGGL((k_unwrap_setup<false, UnwGradSrc>), g.tile_grid, dim3(256), 0, st, buf, gy, weight, nz, n, g.ntx, work, gx);
    HIP_TRY(hipGetLastError());
    return unwrap_scalars(state, work, ptheta, g.tiles, g.tiles, 0, 0, 0.0, st);
}

// the sums of c, their fold, out: three launches
int do_integrate_finish(float* out, double* state, const float* buf, const float* weight, int ptheta, int nz, int n,
                        double* work, hipStream_t st) {
    const UnwGrid g = unwrap_grid(ptheta, nz, n);
    const bool vec = unwrap_vec(n, {out, buf, weight});
    const size_t plane = (size_t)nz * (size_t)n;
    VEC_LAUNCH(k_integrate_offset, vec, g.flat_grid, st, buf, weight, plane, g.tiles, work);
    hipLaunchKernelGGL(k_integrate_mean, dim3((unsigned)ptheta), dim3(256), 0, st, state, (const double*)work, g.flat, g.tiles);
    HIP_TRY(hipGetLastError());
    VEC_LAUNCH(k_integrate_finish, vec, g.flat_grid, st, out, (const double*)state, buf, plane);
    return PTYCHO_OK;
}

}  // namespace
