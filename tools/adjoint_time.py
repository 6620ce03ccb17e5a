#!/usr/bin/env python3
"""Times ``UltrasoundSystem.bfAdjoint`` on one device at a C2-like shape: a 128-element array at 0.3 mm pitch, 128 plane waves, T = K = 2048, a
512 x 512 grid at a quarter wavelength, complex64 synthetic point-target data.  With ``fthresh = -inf`` and ``fthresh = -60``:

* milliseconds of the spectrum step and of ``qdas_adjoint`` separately (device events: warm-up, then the median of ``--reps`` runs), ``Ksel``;
* achieved f32 TFLOP/s under the model ``8 V (N + M) I Ksel`` and its fraction of the 157 TF f32 MFMA rate;
* the same call through a torch composition of the reference's loop (materialised phasor blocks, batched ``torch.matmul``, frequencies blocked under
  1 GiB) -- what a user can do without this kernel --, timed once, and the parity of the two (the float64 oracle is too slow at this size);
* ``bfDAS`` on the same inputs, for orientation.

    python tools/adjoint_time.py [--small] [--reps 3] > profiles/adjoint_time.txt
"""
import argparse
import math
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qups_amd import ChannelData, Scan, Sequence, Transducer, UltrasoundSystem  # noqa: E402
from qups_amd import adjoint as A  # noqa: E402

PEAK_TF = 157.3


def timed(fn, reps, warm=1):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        out = fn()
        b.record()
        torch.cuda.synchronize()
        ms.append(a.elapsed_time(b))
    return float(np.median(ms)), out


def point_target_data(us, T, fs, fc, dev):
    """three scatterers under steered plane waves: a Gaussian pulse at the two-way travel time"""
    Pe = torch.as_tensor(us.rx.positions(), dtype=torch.float64, device=dev)
    nv = torch.as_tensor(us.seq.focus, dtype=torch.float64, device=dev)
    t = torch.arange(T, dtype=torch.float64, device=dev).reshape(T, 1, 1) / fs
    x = torch.zeros((T, Pe.shape[1], nv.shape[1]), dtype=torch.complex64, device=dev)
    for s in ([0.0, 0.0, 20e-3], [-5e-3, 0.0, 12e-3], [6e-3, 0.0, 30e-3]):
        sc = torch.tensor(s, dtype=torch.float64, device=dev)
        d = (torch.linalg.norm(Pe - sc[:, None], dim=0)[None, :, None] + (nv * sc[:, None]).sum(0)[None, None, :]) / us.seq.c0
        x += (torch.exp(-0.5 * ((t - d) / 0.2e-6) ** 2) * torch.exp(2j * math.pi * fc * (t - d))).to(torch.complex64)
    return x


def torch_composition(Xs, freq, Pi, Pr, Pt, cinv, tau_foc, apod_tx, budget=1 << 30):
    """the reference's loop (src/UltrasoundSystem.m:3997-4037) in torch: phasor blocks I x N x Fb, batched matmul, summed over frequency.
    Xs: Ksel x N x V"""
    dev = Xs.device
    tt = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=dev)
    Pi_, Pr_, Pt_ = tt(Pi), tt(Pr), tt(Pt)
    tau_rx = (torch.linalg.norm(Pi_[:, :, None].double() - Pr_[:, None, :].double(), dim=0) * cinv)        # I x N, float64
    tau_tx = (torch.linalg.norm(Pi_[:, :, None].double() - Pt_[:, None, :].double(), dim=0) * cinv)
    foc, apod = torch.as_tensor(tau_foc, dtype=torch.float64, device=dev), tt(apod_tx)
    I, N = tau_rx.shape
    fb = max(1, int(budget // (8 * I * N * 2)))
    ph = lambda cyc: torch.polar(torch.ones_like(cyc, dtype=torch.float32), (2 * math.pi * (cyc - torch.round(cyc))).float())
    b = torch.zeros(I, dtype=torch.complex64, device=dev)
    f = torch.as_tensor(freq, dtype=torch.float64, device=dev)
    for k0 in range(0, len(freq), fb):
        fk = f[k0:k0 + fb].reshape(-1, 1, 1)
        S = apod[None] * ph(-fk * foc[None])                                   # Fb x M x V
        Am = torch.matmul(ph(-fk * tau_tx[None]), S)                           # Fb x I x V
        Am = Am / torch.linalg.norm(Am, dim=2, keepdim=True)
        R = torch.matmul(ph(fk * tau_rx[None]), Xs[k0:k0 + fb])                   # (Fb x I x N) (Fb x N x V)
        b += (R * Am.conj()).sum(dim=(0, 2))
    return b


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="a 64 x 64 grid, 32 elements, 16 plane waves, T = 256 (a quick check of the tool)")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-only", action="store_true", help="skip the torch composition, the end-to-end call and bfDAS (for a run under rocprofv3 --kernel-trace --stats)")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    fs, fc, c0 = 20e6, 5e6, 1540.0
    N, V, T, G = (32, 16, 256, 64) if a.small else (128, 128, 2048, 512)
    lam = c0 / fc
    th = np.deg2rad(np.linspace(-15, 15, V))
    seq = Sequence("PW", np.stack([np.sin(th), 0 * th, np.cos(th)]), c0, V)
    scan = Scan.cartesian((np.arange(G) - G / 2) * lam / 4, 2e-3 + np.arange(G) * lam / 4)
    us = UltrasoundSystem(Transducer.linear(N, 0.3e-3, fc), seq, scan, fs=fs)
    x = point_target_data(us, T, fs, fc, dev)
    chd = ChannelData(x, 0.0, fs)
    I = G * G
    print(f"# adjoint_time: {torch.cuda.get_device_name(0)}; N = M = {N}, V = {V}, T = K = {T}, grid {G} x {G} (I = {I}), complex64, median of {a.reps} after 1 warm-up")
    # geometry and tables staged on the device once: the timed call then holds the kernel, its steering pass and four small device transposes
    dt = lambda a, ty: torch.as_tensor(np.ascontiguousarray(a), device=dev).to(ty)
    Pi = dt(np.asarray(scan.positions(), float).reshape((3, I), order="F"), torch.float32)
    Pr = dt(us.rx.positions(), torch.float32)
    cin = dt([1 / c0], torch.float32)
    tau_foc, apod_tx = dt(seq.delays(us.tx), torch.float64), dt(seq.apodization(us.tx), torch.float32)
    for fthresh in (-math.inf, -60.0):
        ms_spec, X = timed(lambda: A.spectrum(x, 0.0, fs), a.reps)
        ksel = A.select_bins(X, fs, fthresh)
        freq = ksel * (fs / T)
        Xn = X[torch.from_numpy(ksel).to(dev)]                                                  # Ksel x N x V
        Xs = Xn.permute(0, 2, 1).contiguous()                                                   # Ksel x V x N
        ms_k, b = timed(lambda: A.adjoint(Xs, freq, Pi, Pr, Pr, cin, tau_foc, apod_tx), a.reps)
        if a.kernel_only:
            print(f"fthresh {fthresh:6.0f} dB: Ksel {len(ksel):5d}  spectrum {ms_spec:8.2f} ms  qdas_adjoint {ms_k:9.2f} ms")
            continue
        ms_all, b2 = timed(lambda: us.bfAdjoint(chd, fthresh=fthresh), 1, warm=0)
        tf = 8.0 * V * (N + N) * I * len(ksel) / (ms_k * 1e-3) / 1e12
        ms_t, bt = timed(lambda: torch_composition(Xn, freq, Pi.cpu().numpy(), Pr.cpu().numpy(), Pr.cpu().numpy(), 1 / c0, tau_foc.cpu().numpy(),
                                                   apod_tx.cpu().numpy()), 1, warm=0)
        par = float((b - bt).abs().max() / bt.abs().max())
        par2 = float((b2.reshape(-1) - b.reshape(G, G).t().reshape(-1)).abs().max() / b.abs().max())
        print(f"fthresh {fthresh:6.0f} dB: Ksel {len(ksel):5d}  spectrum {ms_spec:8.2f} ms  qdas_adjoint {ms_k:9.2f} ms  ({tf:6.2f} TFLOP/s f32 = {100 * tf / PEAK_TF:4.1f} % of {PEAK_TF} TF)"
              f"  bfAdjoint end to end {ms_all:9.2f} ms  torch composition {ms_t:9.2f} ms ({ms_t / ms_k:5.1f} x)  parity max|b - b_torch| / max|b_torch| {par:.2e}"
              f"  (bfAdjoint against the direct call {par2:.1e})")
        del X, Xn, bt, b2
    # what binds the kernel: the same call with 32 transmits (4 MFMAs per generated phasor) and 64 (8 per phasor); equal times = phasor generation, 1 : 2 = MFMA issue
    k4 = np.arange(0, T // 2, 8)
    for Vs in (32, 64, 128) if V >= 128 else (V,):
        Xv = torch.randn((len(k4), Vs, N), dtype=torch.complex64, device=dev)
        ms_v, _ = timed(lambda: A.adjoint(Xv, k4 * (fs / T), Pi, Pr, Pr, cin, tau_foc[:, :Vs], apod_tx[:, :Vs]), a.reps)
        tfv = 8.0 * Vs * (N + N) * I * len(k4) / (ms_v * 1e-3) / 1e12
        print(f"V = {Vs:3d}, Ksel = {len(k4)}: qdas_adjoint {ms_v:9.2f} ms  ({tfv:6.2f} TFLOP/s)")
    if a.kernel_only:
        return
    ms_das, _ = timed(lambda: us.bfDAS(chd), a.reps)
    print(f"bfDAS on the same inputs: {ms_das:8.2f} ms")


if __name__ == "__main__":
    main()
