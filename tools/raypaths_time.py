#!/usr/bin/env python3
"""Times the straight-ray integrals on one device: the fused path (``qdas_raypaths_integrate``: walk and gather in one kernel, no triplets) against the
composition the reference implies -- ``qdas_raypaths_weights`` (the triplets ``w, ix, iz``, ``4 (X + Z + 1)`` per ray), then a torch gather-multiply-sum
over them, in chunks of the reference's ``bsize`` rays (``kern/rayPaths.m:68``).

* workloads (float32, uniform millimetre grids): ``origin-512`` one origin to every pixel of a 512 x 512 map (``globalAverageC``); ``tables-256`` 128 origins
  to every pixel of 256 x 256 (the ``das_lut`` delay-table shape); ``pairs-256`` the 128 x 128 fan between two 128-element apertures on opposite edges of a
  256 x 256 map (the tomography shape).  Both paths get the same explicit rays, origin by origin: the fused path as ``globalAverageC`` launches them
  (``qups_amd.raypaths._fan``: one origin with a point stride of 0, several origins expanded, ``FAN_RAYS`` per launch), the composition ``bsize`` at a time;
* each workload runs in a child process of its own under ``timeout -k 10 <s>``; a child that ends on a signal, an abort or its time limit ends the tool with
  a non-zero status: nothing more is started on a card after a fault.  This process never opens the device;
* in a child: warm-up, then device events around windows of ``--inner`` back-to-back calls, the two paths interleaved, the median per call of ``--reps``
  windows with the smallest and the largest beside it; the results of the two paths are compared (``max |fused - composed| / max |composed|``);
* per line the byte model: fused = the rays read (16 B), ``y`` written (4 B), the map once; composed = the same rays, the triplets written and
  read again (``12 x 4 K`` B per ray each way), 4 map reads per filled slot counted as 4 B each, ``y`` written.

    python tools/raypaths_time.py [--small] [--reps 7] [--inner 10] > profiles/raypaths_time.txt
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0          # MI355X peak HBM3E rate, TB/s
CHILD_LIMIT_S = 240
FAULT_STATUS = (124, 134, 137, 139)                     # time limit (timeout's own codes), abort, kill, segmentation fault
WORKLOADS = ("origin-512", "tables-256", "pairs-256")


def workload(name, small):
    """``(xg, zg, origins 2 x A, ends 2 x J)`` in metres: every origin is paired with every end point"""
    n = {"origin-512": 512, "tables-256": 256, "pairs-256": 256}[name]
    if small:
        n //= 8
    xg = np.linspace(-19.2e-3, 19.2e-3, n)
    zg = np.linspace(0.0, 38.4e-3, n)
    na = 16 if small else 128
    ex = (np.arange(na) - (na - 1) / 2) * 0.3e-3 * (128 / na)
    if name == "origin-512":
        px, pz = np.meshgrid(xg, zg, indexing="ij")
        return xg, zg, np.array([[0.0], [0.0]]), np.stack((px.reshape(-1), pz.reshape(-1)))
    if name == "tables-256":
        px, pz = np.meshgrid(xg, zg, indexing="ij")
        return xg, zg, np.stack((ex, np.zeros(na))), np.stack((px.reshape(-1), pz.reshape(-1)))
    return xg, zg, np.stack((ex, np.zeros(na))), np.stack((ex, np.full(na, zg[-1])))


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


def child(name, small, reps, inner):
    import torch
    if not torch.cuda.is_available():
        sys.exit("raypaths_time: no HIP device visible -- nothing is measured without one")
    from qups_amd import raypaths as RP
    dev, dtype = torch.device("cuda:0"), torch.float32
    xg, zg, org, ends = workload(name, small)
    X, Z, A, J = xg.size, zg.size, org.shape[1], ends.shape[1]
    K = RP.slots(X, Z)
    g = torch.Generator(device=dev).manual_seed(1)
    m = 1 / (1540.0 + 60.0 * torch.rand((Z, X), dtype=dtype, device=dev, generator=g))            # a slowness map, "ZX"
    gx, gz = RP._grid(xg, "x", dtype, dev, True), RP._grid(zg, "z", dtype, dev, True)
    a = torch.from_numpy(org.T.copy()).to(dev, dtype)                                              # A x 2
    b = torch.from_numpy(ends.T.copy()).to(dev, dtype)                                             # J x 2
    m3 = m.unsqueeze(0)
    bsize = RP.default_bsize(X, Z, 1)
    flat = m.reshape(-1)

    if A > 1:
        ae, be = a.repeat_interleave(J, dim=0), b.repeat(A, 1)                                     # the composition's rays (outside the timed window)
    else:
        ae, be = a, b

    def fused():
        y = torch.empty((A, J), dtype=dtype, device=dev)
        RP._fan(y, m3, gx, gz, a, b, dtype, dev, 1, X)
        return y

    def composed():
        y = torch.empty((A * J,), dtype=dtype, device=dev)
        for j0 in range(0, A * J, bsize):
            j1 = min(A * J, j0 + bsize)
            w, ix, iz = RP._weights(gx, gz, ae[j0:j1] if A > 1 else ae, be[j0:j1], j1 - j0, int(A > 1), 1, dtype, dev)
            lin = (iz.to(torch.int64) * X + ix).clamp_(min=0)                                      # (an empty slot has w = 0: any valid index will do)
            y[j0:j1] = (w * flat[lin]).sum(dim=(1, 2))
        return y.view(A, J)

    (ms_f, lo_f, hi_f), (ms_c, lo_c, hi_c), (yf, yc) = timed_pair(torch, fused, composed, reps, inner)
    par = float((yf - yc).abs().max() / yc.abs().max())
    w, ix, _ = RP._weights(gx, gz, a[:1], b, J, 0, 1, dtype, dev)
    filled = float((ix[:, :, 0] >= 0).sum()) / J                                                   # filled slots per ray, first origin
    rays = A * J
    by_f = rays * (16 + 4) + X * Z * 4
    by_c = rays * (16 + 4) + 2 * rays * K * 4 * 12 + rays * filled * 4 * 4
    print(f"{name:11s} grid {X} x {Z}  {A} origin(s) x {J} end points = {rays} rays, K = {K} slots of which {filled:6.1f} filled on average (first origin), composed in chunks of {bsize} rays: "
          f"fused {ms_f:9.3f} ms [{lo_f:.3f} .. {hi_f:.3f}]  composed {ms_c:9.3f} ms [{lo_c:.3f} .. {hi_c:.3f}]  composed / fused {ms_c / ms_f:7.1f} x  "
          f"bytes: fused {by_f / 1e6:9.1f} MB ({by_f / (ms_f * 1e-3) / 1e12:5.3f} TB/s)  composed {by_c / 1e6:10.1f} MB ({by_c / (ms_c * 1e-3) / 1e12:5.3f} TB/s = "
          f"{100 * by_c / (ms_c * 1e-3) / 1e12 / HBM_TBS:4.1f} % of HBM)  {rays * filled / (ms_f * 1e-3) / 1e9:7.2f} G segments/s fused  "
          f"parity max|fused - composed| / max|composed| {par:.2e}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="grids of an eighth of the size, 16 origins (a quick check of the tool)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=10, help="calls per timed window")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.small, a.reps, a.inner)
    print(f"# raypaths_time: float32, one map; device events around windows of {a.inner} calls, fused and composed interleaved, median per call of {a.reps} windows "
          f"[smallest .. largest] after 2 warm-ups; each workload in a process of its own (limit {CHILD_LIMIT_S} s); HBM fraction against {HBM_TBS} TB/s", flush=True)
    for name in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--inner", str(a.inner)]
        r = subprocess.run(cmd + (["--small"] if a.small else []), capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode < 0 or r.returncode in FAULT_STATUS or "illegal memory access" in r.stderr:
            sys.exit(f"raypaths_time: the child for {name} ended with status {r.returncode} (signal, abort or time limit): nothing more is run on this device.\n{r.stderr[-600:]}")
        if r.returncode:
            sys.exit(f"raypaths_time: the child for {name} failed with status {r.returncode}:\n{r.stderr[-1200:]}")


if __name__ == "__main__":
    main()
