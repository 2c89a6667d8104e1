// host_fit.hpp -- launchers of the fit-residual kernels (k_fit.hpp) for checked arguments; the exported functions and
// their argument checks are in ptycho_kernels.hip.
#pragma once

namespace {

inline bool fit_aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

int do_fit_accumulate(float* inten, const c32* g, size_t count, int add, hipStream_t st) {
    const int vec = fit_aligned16(inten) && fit_aligned16(g);
    hipLaunchKernelGGL(k_fit_accumulate, dim3((unsigned)((count + 1023) / 1024)), dim3(256), 0, st, inten, g, count, add, vec);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

// the pass, then the fold of whatever the pass left in work (nothing: one wave tile and one range)
int do_fit_frames(double* frames, double* pixels, const float* inten, const c32* g, const float* data,
                  const unsigned char* mask, const double* ab, long long ptheta, long long nscan, long long npix,
                  double* work, hipStream_t st) {
    const FitPlan p = fit_plan(ptheta, nscan, npix);
    double* fpart = p.fwords ? work : frames;
    double* ppart = p.pwords ? work + p.fwords : pixels;
    const FitArgs a{fpart, ppart, inten, g, data, mask, ab, npix, p.nwt, (int)nscan, (int)p.flen};
    // 16-byte loads: every frame starts on a multiple of four pixels and the arrays on 16 bytes
    const bool vec = npix % kFitLanePix == 0 && fit_aligned16(data) && (!inten || fit_aligned16(inten)) &&
                     (!g || fit_aligned16(g));
    const dim3 grid((unsigned)p.ntiles, (unsigned)p.nranges, (unsigned)ptheta);
    if (vec && pixels) hipLaunchKernelGGL((k_fit_frames<true, true>), grid, dim3(256), 0, st, a);
    else if (vec) hipLaunchKernelGGL((k_fit_frames<true, false>), grid, dim3(256), 0, st, a);
    else if (pixels) hipLaunchKernelGGL((k_fit_frames<false, true>), grid, dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_fit_frames<false, false>), grid, dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    const long long nfout = p.fwords ? ptheta * nscan * kFitCols : 0;
    const long long npout = p.pwords && pixels ? ptheta * kFitMaps * npix : 0;
    const long long fblocks = (nfout + 255) / 256, pblocks = (npout + 255) / 256;
    if (fblocks + pblocks > 0) {
        hipLaunchKernelGGL(k_fit_fold, dim3((unsigned)(fblocks + pblocks)), dim3(256), 0, st, frames, pixels,
                           (const double*)fpart, (const double*)ppart, nfout, p.nwt, npout, kFitMaps * npix, p.nranges,
                           (unsigned)fblocks);
        HIP_TRY(hipGetLastError());
    }
    return PTYCHO_OK;
}

}  // namespace
