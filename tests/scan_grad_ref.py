"""References for the scan-position gradient (``PtychoHIP.adj_scan`` / ``fwd_autograd``), shared by
tests/test_scan_grad_cpu.py and tests/test_hip_scan_grad.py.  No GPU involved.

* ``adj_scan_ref``: the formula of include/ptycho_hip.h (``ptycho_adj_scan``) in NumPy on the oracle's own pieces
  (``_adj_nearplane``, ``split_positions``), ``"double"`` or ``"single"``; the float32 version forms every product and every
  sum in float32.
* ``fwd_torch``: ``oracle.ptycho_oracle.fwd`` restated in differentiable torch on the CPU (complex128 or complex64); its
  autograd gives reference gradients of any loss for ``psi``, ``probe`` and ``scan``.
* ``grad_case`` / ``GRAD_CASES``: the geometries of the GPU test with the positions every case must contain.
* ``refine_scenario`` / ``refine``: the end-to-end scenario (positions recovered by Adam on ``scan`` alone).
"""
import numpy as np

from oracle import ptycho_oracle as op


# ---- the formula ------------------------------------------------------------------------------------------------------------
def adj_scan_ref(farplane, scan, psi, probe, precision="double"):
    """``out[t, s] = c Re sum_ij conj(w_ij) probe_ij (dPy_ij, dPx_ij)``, float64 or float32 ``[ptheta, nscan, 2]``."""
    ct, ft = op._ctype(precision)
    psi, probe = np.asarray(psi), np.asarray(probe)
    ptheta, nz, n = psi.shape
    nprb = probe.shape[-1]
    w, c = op._adj_nearplane(farplane, nprb, precision)          # [ptheta, nscan, nprb, nprb], 1 / ndet
    ip, fr, valid = op.split_positions(scan, precision)
    nscan = ip.shape[1]
    out = np.zeros((ptheta, nscan, 2), dtype=ft)
    ar = np.arange(nprb + 1)
    one = ft(1)
    for t in range(ptheta):
        f = psi[t].astype(ct)
        prb = probe[t].astype(ct)
        rows = ip[t, :, 0][:, None] + ar[None, :]
        cols = ip[t, :, 1][:, None] + ar[None, :]
        rok = (rows >= 0) & (rows < nz)
        cok = (cols >= 0) & (cols < n)
        big = f[np.clip(rows, 0, nz - 1)[:, :, None], np.clip(cols, 0, n - 1)[:, None, :]]
        big = np.where(rok[:, :, None] & cok[:, None, :], big, ct(0))        # taps outside the object read 0
        f00, f01, f10, f11 = big[:, :-1, :-1], big[:, :-1, 1:], big[:, 1:, :-1], big[:, 1:, 1:]
        fy = fr[t, :, 0][:, None, None]
        fx = fr[t, :, 1][:, None, None]
        dpy = (f10 - f00) * (one - fx) + (f11 - f01) * fx
        dpx = (f01 - f00) * (one - fy) + (f11 - f10) * fy
        for k, dp in enumerate((dpy, dpx)):
            term = (np.conj(w[t]) * (prb[None] * dp)).real.astype(ft)
            out[t, :, k] = c * term.reshape(nscan, -1).sum(axis=1, dtype=ft)
        out[t, ~valid[t]] = 0
    return out


# ---- fwd in differentiable torch ----------------------------------------------------------------------------------------------
def fwd_torch(psi, scan, probe, ndet):
    """``oracle.fwd`` in torch on the CPU: ``psi [T, nz, n]`` and ``probe [T, nprb, nprb]`` complex128 (or complex64),
    ``scan [T, S, 2]`` real (float64 holding float32 values, or float32; split on the float32 value as the oracle does).
    Same taps, same order of the weight products, zeros outside the object, skipped positions give a zero tile."""
    import torch
    ct = psi.dtype
    rt = torch.float64 if ct == torch.complex128 else torch.float32
    T, nz, n = psi.shape
    nprb = probe.shape[-1]
    ip = torch.trunc(scan.detach().to(torch.float32))
    frac = scan.to(rt) - ip.to(rt)                # exact in float32, so the same fraction in both precisions (the gradient
                                                  # stays in rt: no float32 cast on its way back to scan)
    valid = (ip[..., 0] >= 0) & (ip[..., 1] >= 0)
    ar = torch.arange(nprb + 1)
    rows = ip[..., 0].long()[..., None] + ar
    cols = ip[..., 1].long()[..., None] + ar
    rows = torch.where((rows < 0) | (rows >= nz), torch.full_like(rows, nz), rows)      # row nz / column n: zeros
    cols = torch.where((cols < 0) | (cols >= n), torch.full_like(cols, n), cols)
    padded = torch.zeros((T, nz + 1, n + 1), dtype=ct)
    padded[:, :nz, :n] = psi
    tt = torch.arange(T)[:, None, None, None]
    big = padded[tt, rows[:, :, :, None], cols[:, :, None, :]]                         # [T, S, nprb + 1, nprb + 1]
    fy = frac[..., 0][..., None, None]
    fx = frac[..., 1][..., None, None]
    p = big[..., :-1, :-1] * (1 - fx) * (1 - fy)
    p = p + big[..., :-1, 1:] * fx * (1 - fy)
    p = p + big[..., 1:, :-1] * (1 - fx) * fy
    p = p + big[..., 1:, 1:] * fx * fy
    p = p * valid[..., None, None].to(rt)
    pad = (ndet - nprb) // 2
    near = torch.zeros((T, scan.shape[1], ndet, ndet), dtype=ct)
    near[:, :, pad:pad + nprb, pad:pad + nprb] = (1.0 / ndet) * (probe[:, None] * p)
    return torch.fft.fft2(near)


def torch_grads(loss_of, psi, scan, probe, ndet, precision="double", wrt=("psi", "scan", "probe")):
    """Gradients of the real loss ``loss_of(farplane)`` through ``fwd_torch`` as NumPy arrays (torch's convention for
    complex leaves: ``dL/dRe + i dL/dIm``), in the order of ``wrt``."""
    import torch
    ct, rt = (torch.complex128, torch.float64) if precision == "double" else (torch.complex64, torch.float32)
    leaves = {"psi": torch.tensor(np.asarray(psi), dtype=ct), "scan": torch.tensor(np.asarray(scan, dtype=np.float32), dtype=rt),
              "probe": torch.tensor(np.asarray(probe), dtype=ct)}
    for name in wrt:
        leaves[name].requires_grad_(True)
    loss_of(fwd_torch(leaves["psi"], leaves["scan"], leaves["probe"], ndet)).backward()
    return [leaves[name].grad.numpy() for name in wrt]


# ---- geometries of the GPU test -----------------------------------------------------------------------------------------------
#: ndet, nprb, nscan, ptheta.  ptheta is chosen here: 2 where the case asks for two angles, and otherwise the smallest number
#: of angles with which ptheta * nscan holds the five kinds of position that every case must contain.
GRAD_CASES = [(16, 16, 5, 1), (32, 16, 7, 1), (64, 24, 33, 2), (100, 20, 6, 1), (112, 48, 6, 1), (256, 64, 9, 1),
              (256, 256, 3, 2), (512, 512, 2, 3)]


def crand(rng, shape):
    return (rng.standard_normal(shape) + 1j * rng.standard_normal(shape)).astype(np.complex64)


def grad_case(ndet, nprb, nscan, ptheta, seed=0):
    """Random complex object, probes (another one per angle) and farplane, and positions that contain, in this order from
    the first position of the first angle on: an exact integer, a -0.3 coordinate (valid, negative fraction), a -1.5
    coordinate (skipped), a patch overhanging the bottom and right edges, a position wholly outside the object; the rest
    are random inside the object.  ``special``: the flat indices of the five."""
    rng = np.random.default_rng(1000 * ndet + nprb + seed)
    nz, n = nprb + 11, nprb + 18
    psi = crand(rng, (ptheta, nz, n))
    probe = crand(rng, (ptheta, nprb, nprb))
    farplane = crand(rng, (ptheta, nscan, ndet, ndet))
    lim = np.array([nz - nprb - 1, n - nprb - 1], dtype=np.float64)
    scan = (rng.random((ptheta * nscan, 2)) * lim).astype(np.float32)
    assert ptheta * nscan >= 5
    scan[0] = (3.0, 5.0)
    scan[1] = (-0.3, 2.25)
    scan[2] = (-1.5, 4.0)
    scan[3] = (nz - nprb // 2 - 0.625, n - nprb // 2 - 1 + 0.375)
    scan[4] = (nz + 3.5, n + 7.25)
    return dict(psi=psi, probe=probe, farplane=farplane, scan=scan.reshape(ptheta, nscan, 2), nz=nz, n=n,
                special=dict(integer=0, negative_fraction=1, skipped=2, overhang=3, outside=4))


# ---- the end-to-end scenario --------------------------------------------------------------------------------------------------
REFINE_LR, REFINE_STEPS = 0.05, 80      # chosen on the CPU with fwd_torch in float64 (tests/test_scan_grad_cpu.py)


def refine_scenario(seed=7):
    """Object 64^2 (smooth: a few low-frequency phase waves, 20 % amplitude modulation), gaussian 16^2 probe with a
    quadratic phase, ndet 32, an 8 x 8 raster of step 5.5 with +-0.6 jitter, noise-free data from the float64 oracle, and
    start positions off by uniform +-0.45 px."""
    rng = np.random.default_rng(seed)
    nz = n = 64
    nprb, ndet = 16, 32
    y, x = np.mgrid[:nz, :n] / 64.0
    phase = (0.9 * np.sin(2 * np.pi * (2 * x + y)) + 0.6 * np.cos(2 * np.pi * (3 * y - x) + 0.4)
             + 0.5 * np.sin(2 * np.pi * (4 * x + 3 * y) + 1.1))
    amp = 1.0 + 0.2 * np.cos(2 * np.pi * (2 * y + 0.3)) * np.cos(2 * np.pi * (3 * x - 0.2))
    psi = (amp * np.exp(1j * phase)).astype(np.complex64)[None]
    r = np.arange(nprb) - (nprb - 1) / 2
    r2 = r[:, None] ** 2 + r[None, :] ** 2
    probe = (np.exp(-r2 / (2 * 3.5 ** 2)) * np.exp(1j * 0.06 * r2)).astype(np.complex64)[None]
    k = np.arange(8) * 5.5 + 2.0
    true = np.stack(np.meshgrid(k, k, indexing="ij"), -1).reshape(1, 64, 2) + rng.uniform(-0.6, 0.6, (1, 64, 2))
    true = true.astype(np.float32)
    start = (true + rng.uniform(-0.45, 0.45, true.shape)).astype(np.float32)
    data = np.abs(op.fwd(psi, true, probe, ndet, "double")) ** 2
    return dict(psi=psi, probe=probe, scan_true=true, scan_start=start, data=data, ndet=ndet, nprb=nprb, nz=nz, n=n)


def rms_error(scan, true):
    d = np.asarray(scan, dtype=np.float64) - np.asarray(true, dtype=np.float64)
    return float(np.sqrt((d ** 2).sum(-1).mean()))


def refine(forward, scan, sqrt_data, lr=REFINE_LR, steps=REFINE_STEPS):
    """``torch.optim.Adam`` on ``scan`` alone (a leaf tensor, updated in place) with the loss
    ``sum (|forward(scan)| - sqrt_data)^2``; returns the loss of every step."""
    import torch
    scan.requires_grad_(True)
    opt = torch.optim.Adam([scan], lr=lr)
    losses = []
    for _ in range(steps):
        opt.zero_grad()
        loss = ((torch.abs(forward(scan)) - sqrt_data) ** 2).sum()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    scan.requires_grad_(False)
    return losses
