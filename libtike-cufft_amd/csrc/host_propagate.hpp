// host_propagate.hpp -- launchers of the propagation kernels (k_propagate.hpp) for checked arguments; the exported
// functions and their argument checks are in ptycho_kernels.hip.
#pragma once

namespace {

// sides ptycho_fft2 takes from 16 up, and a pair count that fits the kernels' 32-bit pair index
bool prop_sizes_ok(size_t s, size_t nfield, size_t nplane) {
    return frc_size_ok((long long)s) && nfield >= 1 && nplane >= 1 && nfield < kPropMaxPairs && nplane < kPropMaxPairs &&
           nfield * nplane < kPropMaxPairs;
}

// the one-launch path: a side with a plan whose tile fits a compute unit's LDS, option "tile" on (as do_fft2 chooses)
bool prop_fused(ptycho_handle h) { return !h->bs_m && h->ge.ndet <= 128 && h->use_tile; }

// k_prop_apply into buf, the in-place inverse transform of the caller, k_prop_metrics
template <class Inverse>
int prop_two_pass(ptycho_handle h, const PropArgs& a, hipStream_t st, Inverse inverse) {
    const int s = h->ge.ndet;
    const long long npairs = a.nfield * a.nplane, npix = (long long)s * s;
    c32* buf = a.planes ? a.planes : a.work;
    const dim3 grid((unsigned)((npix + 255) / 256), (unsigned)(a.nplane < 65535 ? a.nplane : 65535));
    hipLaunchKernelGGL(k_prop_apply, grid, dim3(256), 0, st, buf, a.spec, a.zl, a.nfield, a.nplane, s, a.q0, a.method);
    HIP_TRY(hipGetLastError());
    if (int rc = inverse(buf, npairs)) return rc;
    if (a.metrics) {
        const long long cap = (long long)h->n_cu * 8;
        hipLaunchKernelGGL(k_prop_metrics, dim3((unsigned)(npairs < cap ? npairs : cap)), dim3(256), 0, st, a.metrics,
                           (const c32*)buf, npairs, s);
        HIP_TRY(hipGetLastError());
    }
    return PTYCHO_OK;
}

template <int N>
int do_propagate(ptycho_handle h, const PropArgs& a, hipStream_t st) {
    if constexpr (N <= 128) {
        if (prop_fused(h)) {
            hipLaunchKernelGGL((k_prop_tile<N>), dim3(tile_grid<N>(h, a.nfield * a.nplane)), dim3(TileCfg<N>::NT), 0, st, a,
                               (const c32*)h->table);
            HIP_TRY(hipGetLastError());
            return PTYCHO_OK;
        }
    }
    return prop_two_pass(h, a, st, [&](c32* buf, long long nb) { return do_fft2<N>(h, buf, buf, nb, +1, st); });
}

template <int M>
int do_propagate_generic(ptycho_handle h, const PropArgs& a, hipStream_t st) {
    return prop_two_pass(h, a, st, [&](c32* buf, long long nb) { return do_fft2_generic<M>(h, buf, buf, nb, +1, st); });
}

}  // namespace
