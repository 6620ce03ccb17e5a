#!/usr/bin/env python3
"""Times the fused demodulator on one device: ``qdas_demod`` (downmix, FIR low-pass and decimation in one launch) beside the two compositions the package
offers without it, in the same run:

* ``hilbert(fdown)`` -> ``filter`` -> ``downsample`` (real data only: the one-pass Hilbert kernel mixes down as it goes; analytic amplitude);
* ``downmix`` -> ``filter`` -> ``downsample`` (``ChannelData``'s three methods: a torch multiply, ``qdas_convd`` with the causal window, a strided copy).

* workloads: the C3 record (``T = 2816``, 256 x 256 traces) as int16 and float32 with ``ratio = 4`` and 25 / 129 taps, the C2 record (``T = 2048``,
  128 x 128 traces, float32, 25 taps); ``das-c2`` / ``das-c3``: ``DAS`` of the configuration on the decimated record with ``fmod = fc`` beside ``DAS`` on the
  full analytic record (random data: times only);
* three figures per demodulation workload: the C entry with a prepared descriptor, ``ChannelData.demod`` and each composition; the entry's result is compared
  with ``downmix -> filter -> downsample`` (``max |a - b| / max |b|``);
* each workload runs in a child process of its own under ``timeout -k 10 <s>``; a child that ends on a signal, an abort or its time limit ends the tool with
  a non-zero status: nothing more is started on a card after a fault.  This process never opens the device;
* in a child: warm-up, then device events around windows of ``--inner`` back-to-back calls, the paths interleaved, the median per call of ``--reps`` windows
  with the smallest and the largest beside it;
* the byte model: every input sample read once, ``8 J C`` output bytes written once.

    python tools/demod_time.py [--small] [--reps 7] [--inner 10] > profiles/demod_time.txt
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
FC, FS, RATIO = 5e6, 20e6, 4
# name: (T, N, M, dtype, taps)
DEMOD = {"c3-i16-k25": (2816, 256, 256, "int16", 25), "c3-i16-k129": (2816, 256, 256, "int16", 129), "c3-f32-k25": (2816, 256, 256, "float32", 25),
         "c3-f32-k129": (2816, 256, 256, "float32", 129), "c2-f32-k25": (2048, 128, 128, "float32", 25)}
WORKLOADS = tuple(DEMOD) + ("das-c2", "das-c3")


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


def child_demod(name, small, reps, inner):
    import torch
    from qups_amd import ChannelData, _lib
    from qups_amd.demod import lowpass_taps
    from qups_amd.preproc import hilbert
    dev = torch.device("cuda:0")
    T, N, M, dt, K = DEMOD[name]
    if small:
        N, M = N // 8, M // 8
    Cn, J = N * M, -(-T // RATIO)
    g = torch.Generator(device=dev).manual_seed(1)
    xf = torch.randn((Cn, T), dtype=torch.float32, device=dev, generator=g)
    xs = (xf * 500).to(torch.int16) if dt == "int16" else xf                                       # C x T: time fastest
    x = xs.t().reshape(T, N, M)                                                                    # the T x N x M view the Python layer takes without a copy
    b = lowpass_taps(0.4 * FC, FS, K - 1)
    bt = torch.from_numpy(b.astype(np.float32)).to(dev)
    t0 = 1.3e-6
    cyc0 = torch.tensor([FC * t0 - np.floor(FC * t0)], dtype=torch.float64, device=dev)
    out = torch.empty((Cn, J), dtype=torch.complex64, device=dev)
    d = _lib.DemodDesc()
    d.T, d.C, d.K, d.R, d.x_ld, d.out_ld = T, Cn, K, RATIO, T, J
    d.in_type, d.out_half, d.device = (_lib.DEMOD_I16 if dt == "int16" else _lib.DEMOD_F32), 0, 0
    d.fc_over_fs, d.step = FC / FS, FC * RATIO / FS
    d.cyc0, d.gdiv, d.G = C.c_void_p(cyc0.data_ptr()), 1, 1
    d.queue = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    L = _lib.lib()
    chd = ChannelData(x, t0, FS, "TNM")
    chd_f = ChannelData(x.float() if dt == "int16" else x, t0, FS, "TNM")                          # downmix's torch multiply takes floating data

    def entry():
        _lib.check(L.qdas_demod(C.byref(d), C.c_void_p(xs.data_ptr()), C.c_void_p(bt.data_ptr()), C.c_void_p(out.data_ptr())))
        return out

    def method():
        return chd.demod(FC, RATIO, bt).data

    def via_hilbert():
        y = hilbert(x, None, fdown=FC, t0=t0, fs=FS)
        return ChannelData(y, t0, FS, "TNM").filter(bt).downsample(RATIO).data

    def via_downmix():
        return chd_f.downmix(FC).filter(bt).downsample(RATIO).data

    st, outs = timed(torch, [entry, method, via_hilbert, via_downmix], reps, inner)
    ye = outs[0].t().reshape(J, N, M)
    par = float((ye - outs[3]).abs().max() / outs[3].abs().max())
    same = bool(torch.equal(torch.view_as_real(ye.contiguous()), torch.view_as_real(outs[1].contiguous())))
    nb_in, nb_out = xs.numel() * xs.element_size(), out.numel() * 8
    by = nb_in + nb_out
    rate = by / (st[0][0] * 1e-3) / 1e12
    print(f"{name:12s} T = {T}, {N} x {M} traces, {dt}, ratio {RATIO}, {K} taps: C entry {fmt(st[0])}  ChannelData.demod {fmt(st[1])}  "
          f"hilbert(fdown) -> filter -> downsample {fmt(st[2])} = {st[2][0] / st[0][0]:5.2f} x the entry  "
          f"downmix -> filter -> downsample {fmt(st[3])} = {st[3][0] / st[0][0]:5.2f} x the entry  "
          f"bytes {by / 1e6:8.2f} MB (input {nb_in / 1e6:.2f} read once + output {nb_out / 1e6:.2f} written once): entry {1e3 * rate:8.1f} GB/s = "
          f"{100 * rate / HBM_TBS:5.2f} % of the HBM roof  method == entry: {same}  parity max|entry - downmix composition| / max {par:.2e}")


def child_das(name, small, reps, inner):
    import torch
    from qups_amd import das_spec
    from qups_amd.configs import workload
    dev = torch.device("cuda:0")
    w = workload("small" if small else name[4:])
    T, N, M, fs = w["T"], w["N"], w["M"], w["fs"]
    fc = fs / 4
    J = -(-T // RATIO)
    g = torch.Generator(device=dev).manual_seed(1)
    full = torch.view_as_complex(torch.randn((T, N, M, 2), dtype=torch.float32, device=dev, generator=g))
    deci = torch.view_as_complex(torch.randn((J, N, M, 2), dtype=torch.float32, device=dev, generator=g))
    args = (w["Pi"], w["Pr"], w["Pv"], w["Nv"])
    K = 25

    def das_full():
        return das_spec("DAS", *args, full, w["t0"], fs, w["c0"], *w["opt"], "interp", w["interp"])

    def das_deci():
        return das_spec("DAS", *args, deci, w["t0"] - (K - 1) / 2 / fs, fs / RATIO, w["c0"], *w["opt"], "interp", w["interp"], "modulation", fc)

    st, _ = timed(torch, [das_full, das_deci], reps, max(1, inner // 5), warm=2)
    print(f"{name:12s} {w['label']}: DAS on the full analytic record (T = {T}) {fmt(st[0])}  DAS on the record decimated by {RATIO} (T = {J}, fmod = fc) {fmt(st[1])} "
          f"= {st[1][0] / st[0][0]:5.2f} x the full record's time")


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
            sys.exit("demod_time: no HIP device visible -- nothing is measured without one")
        return (child_das if a.child.startswith("das-") else child_demod)(a.child, a.small, a.reps, a.inner)
    print(f"# demod_time: fc = {FC / 1e6:g} MHz, fs = {FS / 1e6:g} MHz, Hamming low-pass at 0.4 fc; device events around windows of {a.inner} back-to-back calls, the paths "
          f"interleaved, median per call of {a.reps} windows [smallest .. largest] after 3 warm-ups; each workload in a process of its own (limit {CHILD_LIMIT_S} s); "
          f"HBM roof {HBM_TBS} TB/s", flush=True)
    for name in (a.only.split(",") if a.only else WORKLOADS):
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--inner", str(a.inner)]
        r = subprocess.run(cmd + (["--small"] if a.small else []), capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode < 0 or r.returncode in FAULT_STATUS or "illegal memory access" in r.stderr:
            sys.exit(f"demod_time: the child for {name} ended with status {r.returncode} (signal, abort or time limit): nothing more is run on this device.\n{r.stderr[-600:]}")
        if r.returncode:
            sys.exit(f"demod_time: the child for {name} failed with status {r.returncode}:\n{r.stderr[-1200:]}")


if __name__ == "__main__":
    main()
