// host_prepare.hpp -- launcher of the frame-preparation kernels (k_prepare.hpp) for checked arguments; the exported
// functions and their argument checks are in ptycho_kernels.hip.
#pragma once

namespace {

template <typename T>
void prep_launch(const PrepArgs& a, const dim3 grid, const bool vec, hipStream_t st) {
    const bool v = vec && ((uintptr_t)a.raw & (4 * sizeof(T) - 1)) == 0;
#define PTY_PREP_BIN(B)                                                                       \
    if (v) hipLaunchKernelGGL((k_prepare<T, B, true>), grid, dim3(256), 0, st, a);            \
    else hipLaunchKernelGGL((k_prepare<T, B, false>), grid, dim3(256), 0, st, a)
    if (a.g.bin == 1) { PTY_PREP_BIN(1); }
    else if (a.g.bin == 2) { PTY_PREP_BIN(2); }
    else { PTY_PREP_BIN(4); }
#undef PTY_PREP_BIN
}

// the pass, then the fold (FrameFold, host_handle.hpp)
int do_prepare_frames(float* data, unsigned char* mask, double* frames, double* pixels, const void* raw, int dtype,
                      const long long* index, const float* dark, const float* gain, const unsigned char* bad,
                      long long ptheta, long long nraw, long long nscan, const PrepGeom& g, float sat, float scale,
                      int clip, double* work, hipStream_t st) {
    const long long npix = (long long)g.ndet * g.ndet;
    const FrameFold<PrepPart> f(frames, pixels, work, ptheta, nscan, npix);
    // 16-byte stores: every frame starts on a multiple of four pixels and the array on 16 bytes
    const bool vst = npix % PrepPart::kLanePix == 0 && aligned16(data);
    const PrepArgs a{data, mask, f.fpart, f.ppart, raw, index, dark, gain, bad, g, npix, f.p.nwt, nraw, (int)nscan,
                     (int)f.p.flen, sat, scale, clip, vst ? 1 : 0, pixels ? 1 : 0};
    const bool vec = vst && prep_runs_aligned(g);
    switch (dtype) {
        case kPrepU16: prep_launch<unsigned short>(a, f.grid(), vec, st); break;
        case kPrepU32: prep_launch<unsigned int>(a, f.grid(), vec, st); break;
        case kPrepI32: prep_launch<int>(a, f.grid(), vec, st); break;
        default: prep_launch<float>(a, f.grid(), vec, st); break;
    }
    HIP_TRY(hipGetLastError());
    return f.fold(k_prepare_fold, npix, st);
}

}  // namespace
