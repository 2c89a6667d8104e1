// host_scangrad.hpp -- launcher of the scan-position gradient (k_scangrad.hpp) for checked arguments; the exported function
// and its argument checks are in ptycho_kernels.hip.
#pragma once

namespace {

// positions in chunks of work_tiles: the chunk's inverse transform into work (ptycho_fft2, whatever the detector size),
// then one workgroup per position.  Everything on st, nothing synchronises.
int do_adj_scan(ptycho_handle h, float* out, const c32* g, const c32* f, const float* scan, const c32* prb, c32* work,
                size_t work_tiles, hipStream_t st) {
    const Geom& ge = h->ge;
    const long long total = ge.npos();
    const size_t tile = (size_t)ge.ndet * ge.ndet;
    const long long chunk = work_tiles < ((size_t)1 << 20) ? (long long)work_tiles : 1ll << 20;   // one grid, 32-bit indices
    for (long long k0 = 0; k0 < total; k0 += chunk) {
        const long long nb = k0 + chunk < total ? chunk : total - k0;
        if (int rc = ptycho_fft2(h, work, g + (size_t)k0 * tile, (size_t)nb, +1, (void*)st)) return rc;
        const SgArgs a{out, work, f, scan, prb, k0, ge.nscan, ge.nz, ge.n, ge.ndet, ge.nprb, ge.pad};
        hipLaunchKernelGGL(k_scangrad, dim3((unsigned)nb), dim3(kSgThreads), 0, st, a);
        HIP_TRY(hipGetLastError());
    }
    return PTYCHO_OK;
}

}  // namespace
