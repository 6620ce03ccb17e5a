#!/usr/bin/env python3
"""Times the rational-rate polyphase FIR on one device: ``qdas_resample`` as ``resample`` (default Kaiser design) and as the FIR ``filtfilt``, each beside the
composition a user has without it, measured in the same run:

* for ``resample``: zero-stuffing by ``p`` (a torch strided assignment into zeros), ``ChannelData.filter`` (``qdas_convd``, causal) over the ``p``-times
  longer record, then a strided copy by ``q`` from the filter's centre;
* for ``filtfilt``: a torch odd extension by ``3 (K - 1)`` samples, ``ChannelData.filter`` forward, flip, again, flip, trim.

* workloads: the C3 record (``T = 2816``, 256 x 256 traces, float32) at 5/4 and 4/5, the C2 record (``T = 2048``, 128 x 128 traces) at 5/4, 4/5 and 16/25,
  ``filtfilt`` with the 26-tap and the 129-tap Hamming band-pass on C3;
* three figures per workload: the C entry with a prepared descriptor, the ``ChannelData`` method, the composition; the entry's result is compared with the
  composition's (``max |a - b| / max |b|``);
* each workload runs in a child process of its own under ``timeout -k 10 <s>``; a child that ends on a signal, an abort or its time limit ends the tool with
  a non-zero status: nothing more is started on a card after a fault.  This process never opens the device;
* in a child: warm-up, then device events around windows of ``--inner`` back-to-back calls, the paths interleaved, the median per call of ``--reps`` windows
  with the smallest and the largest beside it;
* the byte model: every input sample read once, every output written once.

    python tools/resample_time.py [--small] [--reps 7] [--inner 10] > profiles/resample_time.txt
"""
import argparse
import ctypes as C
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0          # MI355X peak HBM3E rate, TB/s
CHILD_LIMIT_S = 240
FAULT_STATUS = (124, 134, 137, 139)                     # time limit (timeout's own codes), abort, kill, segmentation fault
FC, FS = 5e6, 20e6
# name: (T, N, M, p, q) for resample; (T, N, M, taps) for filtfilt
RESAMPLE = {"c3-5/4": (2816, 256, 256, 5, 4), "c3-4/5": (2816, 256, 256, 4, 5), "c2-5/4": (2048, 128, 128, 5, 4), "c2-4/5": (2048, 128, 128, 4, 5),
            "c2-16/25": (2048, 128, 128, 16, 25)}
FILTFILT = {"c3-ff-k26": (2816, 256, 256, 26), "c3-ff-k129": (2816, 256, 256, 129)}
WORKLOADS = tuple(RESAMPLE) + tuple(FILTFILT)


def timed(torch, fns, reps, inner, warm=3):
    """interleaved windows of ``inner`` calls each: [(median, min, max) ms per call] per function, and the last outputs"""
    for _ in range(warm):
        for fn in fns:
            fn()
    ms = [[] for _ in fns]
    out = [None] * len(fns)
    for _ in range(reps):
        for k, fn in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                out[k] = fn()
            b.record()
            torch.cuda.synchronize()
            ms[k].append(a.elapsed_time(b) / inner)
    return [(float(np.median(v)), float(np.min(v)), float(np.max(v))) for v in ms], out


def fmt(st):
    return f"{st[0]:8.4f} ms [{st[1]:.4f} .. {st[2]:.4f}]"


def child(name, small, reps, inner):
    import torch
    from qups_amd import ChannelData, _lib
    from qups_amd.demod import passband_taps
    from qups_amd.resample import filtfilt_taps, resample_len, resample_taps
    dev = torch.device("cuda:0")
    ff = name in FILTFILT
    if ff:
        T, N, M, Kb = FILTFILT[name]
        p = q = 1
        b = passband_taps((0.5 * FC, 1.5 * FC), FS, Kb - 1)
        h, off, J, edge = filtfilt_taps(b), Kb - 1, T, _lib.RESAMPLE_ODD
    else:
        T, N, M, p, q = RESAMPLE[name]
        h = resample_taps(p, q)
        off, J, edge = (h.size - 1) // 2, resample_len(T, p, q), _lib.RESAMPLE_ZERO
    if small:
        N, M = N // 8, M // 8
    Cn, K = N * M, h.size
    g = torch.Generator(device=dev).manual_seed(1)
    xs = torch.randn((Cn, T), dtype=torch.float32, device=dev, generator=g)                        # C x T: time fastest
    x = xs.t().reshape(T, N, M)                                                                    # the T x N x M view the Python layer takes without a copy
    ht = torch.from_numpy(h.astype(np.float32)).to(dev)
    out = torch.empty((Cn, J), dtype=torch.float32, device=dev)
    d = _lib.ResampleDesc()
    d.T, d.C, d.K, d.J, d.p, d.q, d.off, d.x_ld, d.out_ld = T, Cn, K, J, p, q, off, T, J
    d.in_type, d.edge, d.device = _lib.RESAMPLE_F32, edge, 0
    d.queue = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L = _lib.lib()
    chd = ChannelData(x, 1.3e-6, FS, "TNM")

    def entry():
        _lib.check(L.qdas_resample(C.byref(d), C.c_void_p(xs.data_ptr()), C.c_void_p(ht.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    if ff:
        bt = torch.from_numpy(b.astype(np.float32)).to(dev)
        pad = 3 * (Kb - 1)

        def method():
            return chd.filtfilt(b).data

        def composition():                                                                         # time fastest throughout: C x T rows
            lo = 2 * xs[:, :1] - xs[:, 1:pad + 1].flip(1)
            hi = 2 * xs[:, -1:] - xs[:, -pad - 1:-1].flip(1)
            e = torch.cat([lo, xs, hi], 1).t().reshape(T + 2 * pad, N, M)
            y = ChannelData(e, 0.0, FS, "TNM").filter(bt).data
            y = ChannelData(y.flip(0), 0.0, FS, "TNM").filter(bt).data.flip(0)
            return y[pad:pad + T]
    else:
        def method():
            return chd.resample(FS * p / q).data

        def composition():
            z = torch.zeros((Cn, T * p + off), dtype=torch.float32, device=dev)
            z[:, :T * p:p] = xs
            y = ChannelData(z.t().reshape(T * p + off, N, M), 0.0, FS, "TNM").filter(ht).data
            return y[off::q][:J].contiguous()

    st, outs = timed(torch, [entry, method, composition], reps, inner)
    ye = outs[0].t().reshape(J, N, M)
    par = float((ye - outs[2]).abs().max() / outs[2].abs().max())
    same = bool(torch.equal(ye.contiguous(), outs[1].contiguous()))
    nb_in, nb_out = xs.numel() * 4, out.numel() * 4
    by = nb_in + nb_out
    rate = by / (st[0][0] * 1e-3) / 1e12
    what = f"filtfilt, {Kb} taps (one pass with {K})" if ff else f"resample {p}/{q}, {K} taps ({(K - 1) // p + 1} per output)"
    print(f"{name:11s} T = {T}, {N} x {M} traces, float32, {what}: C entry {fmt(st[0])}  ChannelData method {fmt(st[1])}  "
          f"composition {fmt(st[2])} = {st[2][0] / st[0][0]:5.2f} x the entry  "
          f"bytes {by / 1e6:8.2f} MB (input {nb_in / 1e6:.2f} read once + output {nb_out / 1e6:.2f} written once): entry {1e3 * rate:8.1f} GB/s = "
          f"{100 * rate / HBM_TBS:5.2f} % of the HBM roof  method == entry: {same}  parity max|entry - composition| / max {par:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="an eighth of the traces per side (a quick check of the tool)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--only", default=None, help="comma-separated workloads")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        import torch
        if not torch.cuda.is_available():
            sys.exit("resample_time: no HIP device visible -- nothing is measured without one")
        return child(a.child, a.small, a.reps, a.inner)
    print(f"# resample_time: default Kaiser design (n = 10, beta = 5) for resample, Hamming band-pass 0.5 fc .. 1.5 fc (fc = {FC / 1e6:g} MHz, fs = {FS / 1e6:g} MHz) for "
          f"filtfilt; device events around windows of {a.inner} back-to-back calls, the paths interleaved, median per call of {a.reps} windows [smallest .. largest] "
          f"after 3 warm-ups; each workload in a process of its own (limit {CHILD_LIMIT_S} s); HBM roof {HBM_TBS} TB/s", flush=True)
    for name in (a.only.split(",") if a.only else WORKLOADS):
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--inner", str(a.inner)]
        r = subprocess.run(cmd + (["--small"] if a.small else []), capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode < 0 or r.returncode in FAULT_STATUS or "illegal memory access" in r.stderr:
            sys.exit(f"resample_time: the child for {name} ended with status {r.returncode} (signal, abort or time limit): nothing more is run on this device.\n{r.stderr[-600:]}")
        if r.returncode:
            sys.exit(f"resample_time: the child for {name} failed with status {r.returncode}:\n{r.stderr[-1200:]}")


if __name__ == "__main__":
    main()
