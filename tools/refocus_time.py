#!/usr/bin/env python3
"""Times refocus (applying a ready decoder to one frame) on one device: the fused path (``qdas_refocus``, csrc/refocus.hip) against ``compose`` (the same
result from ``torch.fft`` and ``torch.einsum`` -- the only way to get it without the kernels), and the host time of building the decoder.

* totals: ONE process, device events around ``--inner`` back-to-back calls (a timed window of tens of milliseconds, not one call of about 1 ms), warm-up, then
  the median per call of ``--reps`` such windows each, interleaved, with the smallest and the largest window beside it (the spread);
* per pass: a child process per shape that runs the fused path only, under ``timeout -k 10 <s> rocprofv3 --kernel-trace --stats`` (a run of its own: tracing
  slows the host, so the totals are taken with the profiler off); the average duration of each kernel over the child's calls.  A child that ends on a
  signal, an abort or its time limit ends the tool with a non-zero status BEFORE this process opens the device: nothing more is started on a card
  after a fault;
* shapes: C1-like T = 2048, N = 64, V = 32, M = 64 and C2-like T = 2048, N = M = V = 128, one frame, one t0 (no phase passes);
* per shape the byte model -- x read, X written and read, Hi read, Y written and read, y written: 8 T (3 C V + M V + 3 M C) bytes with C = N F
  (``model_bytes``) -- and the f32 flop count of pass 2, 8 T M V N F;
* the decoder: wall time of ``qups_amd.refocus.decoder`` (host numpy, float64) at T = 2048, M = V = 128, once per method.

    python tools/refocus_time.py [--small] [--reps 7] [--inner 20] [--no-passes] [--no-decoder] > profiles/refocus_time.txt
"""
import argparse
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0          # MI355X peak HBM3E rate, TB/s
FS, T0 = 20e6, 1.3e-6


def model_bytes(T, N, V, M, F):
    """x read + X written + X read + Hi read + Y written + Y read + y written, complex64"""
    C = N * F
    return 8 * T * (C * V + 2 * C * V + M * V + 2 * M * C + M * C)


def flops(T, N, V, M, F):
    return 8 * T * M * V * N * F


def setup(shape, torch):
    from qups_amd import refocus as RF
    T, N, V, M, F = shape
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(1)
    x = torch.randn((T, N, V, F), dtype=torch.complex64, device=dev, generator=g)
    rng = np.random.default_rng(2)
    Hi = (rng.standard_normal((M, V, T)) + 1j * rng.standard_normal((M, V, T))) / np.sqrt(V)
    dec = RF.Decoder(Hi)
    dec.on(dev)
    return RF, x, dec


def child(shape, reps):
    import torch
    RF, x, dec = setup(shape, torch)
    for _ in range(reps + 2):
        RF.fused(x, T0, FS, dec)
    torch.cuda.synchronize()


CHILD_LIMIT_S = 300
FAULT_STATUS = (124, 134, 137, 139)                     # time limit (timeout's own codes), abort, kill, segmentation fault


def passes(shape, reps):
    """{kernel: (calls, average us)} of a child run under rocprofv3, or None with the reason.  Exits the tool when the child faulted, aborted or hung."""
    with tempfile.TemporaryDirectory() as d:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "r", "--",
               sys.executable, os.path.abspath(__file__), "--child", ",".join(str(v) for v in shape), "--reps", str(reps)]
        try:
            r = subprocess.run(cmd, capture_output=True, text=True, cwd=d)
        except OSError as e:
            return None, f"rocprofv3 did not run: {e}"
        if r.returncode < 0 or r.returncode in FAULT_STATUS or "illegal memory access" in r.stderr:
            sys.exit(f"refocus_time: the profiled child for {shape} ended with status {r.returncode} (signal, abort or time limit): nothing more is run on "
                     f"this device.\n{r.stderr[-600:]}")
        fs = glob.glob(d + "/**/*kernel_stats.csv", recursive=True)
        if r.returncode or not fs:
            return None, f"rocprofv3 exit {r.returncode}, no kernel_stats.csv: {r.stderr[-300:]}"
        out = {}
        for row in csv.DictReader(open(fs[0])):
            for name in ("fft_twiddles_kernel", "rf_fft", "rf_decode", "rf_ifft"):
                if name in row["Name"]:
                    out[name] = (int(row["Calls"]), float(row["AverageNs"]) / 1e3)
        return out, ""


def timed_pair(torch, fa, fb, reps, inner, warm=2):
    """interleaved windows of ``inner`` calls each: ((median, min, max) ms per call of fa, the same of fb, last outputs)"""
    for _ in range(warm):
        fa(); fb()
    ms = ([], [])
    out = [None, None]
    for _ in range(reps):
        for k, fn in enumerate((fa, fb)):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                out[k] = fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    st = lambda v: (float(np.median(v)), float(np.min(v)), float(np.max(v)))
    return st(ms[0]), st(ms[1]), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="T = 256, N = 8, V = 8, M = 8 only (a quick check of the tool)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
    ap.add_argument("--no-passes", action="store_true")
    ap.add_argument("--no-decoder", action="store_true")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(tuple(int(v) for v in a.child.split(",")), a.reps)
    shapes = [("small", (256, 8, 8, 8, 1))] if a.small else [("C1-like", (2048, 64, 32, 64, 1)), ("C2-like", (2048, 128, 128, 128, 1))]
    per_pass = {}
    if not a.no_passes:                                     # first: this process has not opened the device yet
        for name, shape in shapes:
            per_pass[name] = passes(shape, a.reps)
    import torch
    if not torch.cuda.is_available():
        sys.exit("refocus_time: no HIP device visible -- nothing is measured without one")
    print(f"# refocus_time: {torch.cuda.get_device_name(0)}; complex64, one frame, one t0, a ready decoder; totals: device events around windows of {a.inner} calls, interleaved, "
          f"median per call of {a.reps} windows [smallest .. largest] after 2 warm-ups; passes: rocprofv3 --kernel-trace --stats of a child process, average over its {a.reps + 2} calls; HBM fraction against {HBM_TBS} TB/s")
    for name, shape in shapes:
        T, N, V, M, F = shape
        RF, x, dec = setup(shape, torch)
        (ms_f, lo_f, hi_f), (ms_c, lo_c, hi_c), (yf, yc) = timed_pair(torch, lambda: RF.fused(x, T0, FS, dec), lambda: RF.compose(x, T0, FS, dec), a.reps, a.inner)
        par = float((yf - yc).abs().max() / yc.abs().max())
        mb, gf = model_bytes(*shape), flops(*shape)
        tbs = mb / (ms_f * 1e-3) / 1e12
        print(f"{name:8s} T {T} N {N} V {V} M {M} frames {F}: fused {ms_f:8.3f} ms [{lo_f:.3f} .. {hi_f:.3f}]  compose {ms_c:8.3f} ms [{lo_c:.3f} .. {hi_c:.3f}]  compose / fused {ms_c / ms_f:6.2f} x  "
              f"model {mb / 1e6:7.1f} MB -> {tbs:5.2f} TB/s = {100 * tbs / HBM_TBS:4.1f} % of HBM  pass 2 {gf / 1e9:6.2f} GFLOP (f32) -> {gf / (ms_f * 1e-3) / 1e12:6.2f} TFLOP/s over the whole call  "
              f"parity max|fused - compose| / max|compose| {par:.2e}")
        if name in per_pass:
            rows, why = per_pass[name]
            if rows is None:
                print(f"{name:8s} passes: not measured ({why})")
            else:
                tot = sum(us for _, us in rows.values())
                txt = "  ".join(f"{k} {us:8.1f} us ({n} calls)" for k, (n, us) in rows.items())
                extra = f"  pass 2 alone: {gf / (rows['rf_decode'][1] * 1e-6) / 1e12:6.2f} TFLOP/s" if "rf_decode" in rows else ""
                print(f"{name:8s} passes: {txt}  sum {tot / 1e3:7.3f} ms{extra}")
        del x, dec, yf, yc
        torch.cuda.empty_cache()
    if not a.no_decoder:
        from qups_amd import refocus as RF
        M = V = 8 if a.small else 128
        T = 256 if a.small else 2048
        px = (np.arange(M) - (M - 1) / 2) * 0.3e-3
        fx = np.linspace(-10e-3, 10e-3, V)
        tau = np.sqrt((fx[None, :] - px[:, None]) ** 2 + 30e-3 ** 2) / 1540.0
        for method in RF.METHODS:
            t = time.perf_counter()
            RF.decoder(tau, 1.0, T, FS, method, None, M)
            print(f"decoder  T {T} M {M} V {V} {method:9s}: {time.perf_counter() - t:7.2f} s on the host (numpy float64, {os.cpu_count()} CPUs visible), once per sequence")


if __name__ == "__main__":
    main()
