#!/usr/bin/env python3
"""Times plane-wave Stolt f-k migration on one device, transmits summed: the fused path (``qdas_migration``, csrc/migration.hip) and ``compose`` (the
same image from ``torch.fft`` and ``qups_amd.wsinterpd`` -- the only way to get it without the kernels), in ONE process, device events, warm-up, then
the median of ``--reps`` runs each, interleaved.

* primary shape: a C2-like call, T = 2048, N = 128, M = 128 plane waves, Nfft = [2048, 128];
* second shape: T = 4096, N = 512, M = 16, Nfft = [4096, 512];
* interpolators cubic and lanczos3;
* per line: milliseconds of both, their ratio, the parity of the two images, and the fraction of the HBM rate the fused path reaches under the byte
  model of DESIGN.md 4.8 (passes A, B, C read and write F K M 8 bytes each, less the columns pass A does not write; pass D moves F K 8 twice).

    python tools/migration_time.py [--small] [--reps 5] > profiles/migration_time.txt
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from qups_amd import migration as MG  # noqa: E402

HBM_TBS = 8.0          # MI355X peak HBM3E rate, TB/s


def timed_pair(fa, fb, reps, warm=2):
    """interleaved: (median ms of fa, of fb, last outputs)"""
    for _ in range(warm):
        fa(); fb()
    ms = ([], [])
    out = [None, None]
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            out[k] = fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b))
    return float(np.median(ms[0])), float(np.median(ms[1])), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="T = 256, N = 32, M = 8 only (a quick check of the tool)")
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    fs, c0, pitch, t0 = 20e6, 1540.0, 0.3e-3, 5e-6
    shapes = [(256, 32, 8)] if a.small else [(2048, 128, 128), (4096, 512, 16)]
    print(f"# migration_time: {torch.cuda.get_device_name(0)}; complex64, transmits summed, Nfft = [T, N], interleaved, median of {a.reps} after 2 warm-ups; "
          f"HBM fraction against {HBM_TBS} TB/s")
    for T, N, M in shapes:
        g = torch.Generator(device=dev).manual_seed(1)
        x = torch.randn((T, N, M), dtype=torch.complex64, device=dev, generator=g)
        th = np.deg2rad(np.linspace(-10, 10, M))
        elem = (np.arange(N) - (N - 1) / 2) * pitch
        tau = -np.sin(th)[None, :] * elem[:, None] / c0
        gam = np.sin(th) / (2 - np.cos(th))
        model = (6.0 * T * N * M + 4.0 * T * N) * 8                      # bytes: A, B, C read + write the block; D reads the sum and writes b
        for interp in ("cubic", "lanczos3"):
            fa = lambda: MG.migrate(x, t0, fs, tau, gam, pitch, c0, None, 0.0, interp, True, False)
            fb = lambda: MG.compose(x, t0, fs, tau, gam, pitch, c0, None, 0.0, interp, True, False)
            ms_f, ms_c, (bf, bc) = timed_pair(fa, fb, a.reps)
            par = float((bf - bc).abs().max() / bc.abs().max())
            tbs = model / (ms_f * 1e-3) / 1e12
            print(f"T {T:5d} N {N:4d} M {M:4d} Nfft [{T}, {N}] {interp:9s}: fused {ms_f:8.3f} ms  compose {ms_c:8.3f} ms  compose / fused {ms_c / ms_f:6.2f} x  "
                  f"model {model / 1e6:7.1f} MB -> {tbs:5.2f} TB/s = {100 * tbs / HBM_TBS:4.1f} % of HBM  parity max|fused - compose| / max|compose| {par:.2e}")


if __name__ == "__main__":
    main()
