// host_fit.hpp -- launchers of the fit-residual kernels (k_fit.hpp) for checked arguments; the exported functions and
// their argument checks are in ptycho_kernels.hip.
#pragma once

namespace {

int do_fit_accumulate(float* inten, const c32* g, size_t count, int add, hipStream_t st) {
    const int vec = aligned16(inten) && aligned16(g);
    hipLaunchKernelGGL(k_fit_accumulate, dim3((unsigned)((count + 1023) / 1024)), dim3(256), 0, st, inten, g, count, add, vec);
    HIP_TRY(hipGetLastError());
    return PTYCHO_OK;
}

// the pass, then the fold (FrameFold, host_handle.hpp)
int do_fit_frames(double* frames, double* pixels, const float* inten, const c32* g, const float* data,
                  const unsigned char* mask, const double* ab, long long ptheta, long long nscan, long long npix,
                  double* work, hipStream_t st) {
    const FrameFold<FitPart> f(frames, pixels, work, ptheta, nscan, npix);
    const FitArgs a{f.fpart, f.ppart, inten, g, data, mask, ab, npix, f.p.nwt, (int)nscan, (int)f.p.flen};
    // 16-byte loads: every frame starts on a multiple of four pixels and the arrays on 16 bytes
    const bool vec = npix % FitPart::kLanePix == 0 && aligned16(data) && (!inten || aligned16(inten)) && (!g || aligned16(g));
    if (vec && pixels) hipLaunchKernelGGL((k_fit_frames<true, true>), f.grid(), dim3(256), 0, st, a);
    else if (vec) hipLaunchKernelGGL((k_fit_frames<true, false>), f.grid(), dim3(256), 0, st, a);
    else if (pixels) hipLaunchKernelGGL((k_fit_frames<false, true>), f.grid(), dim3(256), 0, st, a);
    else hipLaunchKernelGGL((k_fit_frames<false, false>), f.grid(), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return f.fold(k_fit_fold, FitPart::kMaps * npix, st);
}

}  // namespace
