#!/usr/bin/env python3
"""Times the transposed straight-ray product on one device: the fused path (``qdas_raypaths_backproject``: a lane per node gathers over the rays, no
triplets, no atomics) against the composition that was the only route before it -- ``qdas_raypaths_weights`` (the triplets ``w, ix, iz``, ``4 (X + Z + 1)``
per ray), then ``index_add_`` of ``w r[j]`` into the map (floating-point atomics), in chunks of the reference's ``bsize`` rays (``kern/rayPaths.m:68``).

* workloads (float32, uniform millimetre grids), those of tools/raypaths_time.py: ``origin-512`` one origin to every pixel of a 512 x 512 map;
  ``tables-256`` 128 origins to every pixel of 256 x 256; ``pairs-256`` the 128 x 128 fan between two 128-element apertures on opposite edges of a 256 x 256
  map (the tomography shape).  Both paths get the same explicit rays, origin by origin, and the same residual vector;
* ``sart-256``: 20 steps of ``qups_amd.ray_sart`` on the ``pairs-256`` rays (one forward and one transposed product per step, the row and column sums once);
  it has no composed counterpart;
* each workload runs in a child process of its own under ``timeout -k 10 <s>``; a child that ends on a signal, an abort or its time limit ends the tool with
  a non-zero status: nothing more is started on a card after a fault.  This process never opens the device;
* in a child: warm-up, then device events around windows of ``--inner`` back-to-back calls, the two paths interleaved, the median per call of ``--reps``
  windows with the smallest and the largest beside it; the results of the two paths are compared (``max |fused - composed| / max |composed|``), and two
  results of either path with each other, bit for bit (the fused path must repeat itself; the composed one need not).

    python tools/raybackproject_time.py [--small] [--reps 5] [--inner 5] > profiles/raybackproject_time.txt
"""
import argparse
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, ROOT)

from raypaths_time import FAULT_STATUS, timed_pair, workload  # noqa: E402

CHILD_LIMIT_S = 240
WORKLOADS = ("origin-512", "tables-256", "pairs-256", "sart-256")
SART_STEPS = 20


def child(name, small, reps, inner):
    import torch
    if not torch.cuda.is_available():
        sys.exit("raybackproject_time: no HIP device visible -- nothing is measured without one")
    from qups_amd import raypaths as RP
    dev, dtype = torch.device("cuda:0"), torch.float32
    xg, zg, org, ends = workload("pairs-256" if name == "sart-256" else name, small)
    X, Z, A, J = xg.size, zg.size, org.shape[1], ends.shape[1]
    K = RP.slots(X, Z)
    rays = A * J
    gx, gz = RP._grid(xg, "x", dtype, dev, True), RP._grid(zg, "z", dtype, dev, True)
    a = torch.from_numpy(org.T.copy()).to(dev, dtype)                                              # A x 2
    b = torch.from_numpy(ends.T.copy()).to(dev, dtype)                                             # J x 2
    ae, be = (a.repeat_interleave(J, dim=0), b.repeat(A, 1)) if A > 1 else (a, b)                  # explicit rays, origin by origin (outside the timed window)
    sa = int(A > 1)
    gen = torch.Generator(device=dev).manual_seed(1)
    tiles = ((X + 7) // 8) * ((Z + 7) // 8)

    if name == "sart-256":
        m = 1 / (1540.0 + 60.0 * torch.rand((Z, X), dtype=dtype, device=dev, generator=gen))       # a slowness map, "ZX"
        t, _ = RP.ray_integrals(m, gx, gz, ae.t(), be.t(), check_grid=False)
        s0 = torch.full((Z, X), 1 / 1540.0, dtype=dtype, device=dev)
        run = lambda: RP.ray_sart(t, gx, gz, ae.t(), be.t(), s0, iters=SART_STEPS, check_grid=False)
        (ms, lo, hi), _, (s1, s2) = timed_pair(torch, run, run, reps, inner)
        res = lambda s: float(torch.linalg.vector_norm(t - RP.ray_integrals(s, gx, gz, ae.t(), be.t(), check_grid=False)[0]))
        print(f"{name:11s} grid {X} x {Z}  {rays} rays, {tiles} tiles, {SART_STEPS} steps of ray_sart: {ms:9.3f} ms [{lo:.3f} .. {hi:.3f}] per call = {ms / SART_STEPS:7.3f} ms per step  "
              f"|t - A s| {res(s0):.3e} -> {res(s1):.3e}  two runs bit-identical: {bool(torch.equal(s1, s2))}")
        return

    r = torch.randn((rays,), dtype=dtype, device=dev, generator=gen)
    bsize = RP.default_bsize(X, Z, 1)

    def fused():
        g = torch.empty((1, Z, X), dtype=dtype, device=dev)
        RP._backproject_into(g, None, r.unsqueeze(0), gx, gz, ae, be, rays, sa, 1, dtype, dev, 1, X)
        return g[0]

    def composed():
        g = torch.zeros((Z * X,), dtype=dtype, device=dev)
        for j0 in range(0, rays, bsize):
            j1 = min(rays, j0 + bsize)
            w, ix, iz = RP._weights(gx, gz, ae[j0:j1] if A > 1 else ae, be[j0:j1], j1 - j0, sa, 1, dtype, dev)
            val = ix >= 0                                                                          # as rayPaths does: the filled slots only -- one synchronisation per
            lin = iz[val].to(torch.int64) * X + ix[val]                                            # chunk (adding the zeros of the empty slots somewhere instead would
            g.index_add_(0, lin, (w * r[j0:j1, None, None])[val])                                  # queue a billion atomics on one address)
        return g.view(Z, X)

    (ms_f, lo_f, hi_f), (ms_c, lo_c, hi_c), (gf, gc) = timed_pair(torch, fused, composed, reps, inner)
    par = float((gf - gc).abs().max() / gc.abs().max())
    same_f, same_c = bool(torch.equal(gf, fused())), bool(torch.equal(gc, composed()))
    by_c = rays * (16 + 4) + 2 * rays * K * 4 * 12
    print(f"{name:11s} grid {X} x {Z}  {A} origin(s) x {J} end points = {rays} rays, {tiles} tiles = waves, composed in chunks of {bsize} rays ({by_c / 1e6:.0f} MB of triplets "
          f"written and read): fused {ms_f:9.3f} ms [{lo_f:.3f} .. {hi_f:.3f}]  composed {ms_c:9.3f} ms [{lo_c:.3f} .. {hi_c:.3f}]  composed / fused {ms_c / ms_f:7.2f} x  "
          f"{rays * tiles / (ms_f * 1e-3) / 1e9:7.2f} G ray-tile tests/s fused  parity max|fused - composed| / max|composed| {par:.2e}  "
          f"two runs bit-identical: fused {same_f}, composed {same_c}")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="grids of an eighth of the size, 16 origins (a quick check of the tool)")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--inner", type=int, default=5, help="calls per timed window")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.small, a.reps, a.inner)
    print(f"# raybackproject_time: float32, one residual vector; device events around windows of {a.inner} calls, fused and composed interleaved, median per call of "
          f"{a.reps} windows [smallest .. largest] after 2 warm-ups; each workload in a process of its own (limit {CHILD_LIMIT_S} s)", flush=True)
    for name in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--inner", str(a.inner)]
        r = subprocess.run(cmd + (["--small"] if a.small else []), capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode < 0 or r.returncode in FAULT_STATUS or "illegal memory access" in r.stderr:
            sys.exit(f"raybackproject_time: the child for {name} ended with status {r.returncode} (signal, abort or time limit): nothing more is run on this device.\n{r.stderr[-600:]}")
        if r.returncode:
            sys.exit(f"raybackproject_time: the child for {name} failed with status {r.returncode}:\n{r.stderr[-1200:]}")


if __name__ == "__main__":
    main()
