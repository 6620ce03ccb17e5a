"""Time the eikonal solver (qdas_eikonal), the table sampler (qdas_eikonal_tables) and bfEikonal end to end.

    python tools/eikonal_time.py [--reps 5] [--out profiles/eikonal_time.txt]

Grids: the reference's own example (src/UltrasoundSystem.m:4146-4164: 481 x 321 nodes of 0.125 mm, layers of 1400 - 1600 m/s, elements on z = 0)
with 16 elements at its 0.5 mm pitch and 128 at 0.3 mm, and a lambda/10 grid (5 MHz, 30.8 um) under a 128 lambda x 128 lambda field of view (1281 x 1281 nodes:
the C2 image's extent) with 128 elements at 0.3 mm pitch.  Per case: wall ms of one solve batch (the call waits for the stream: it ends when the
host has seen a pass that changed nothing), passes taken, nodes solved per second (K C1 C2 / time), and the bytes a pass WOULD move if it visited
every tile (one read and one write of every map, 16 K C1 C2 bytes; most passes visit only the tiles on the front) over the time of a pass, against
the HBM copy rate of 6.0 TB/s.  The sampler alone (device events): one read of the maps and the coordinates, one write of the table, as a fraction of
that rate.  bfEikonal end to end beside bfDAS on the same system (128 elements, 512 x 512 pixels, T = 2048, complex64, cubic).  For context, the
float64 heap solve of ONE source by tests/eikonal_ref.py on the first grid: a Python restatement on one CPU core, NOT the reference's MEX."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from qups_amd import ChannelData, Scan, Sequence, Transducer, UltrasoundSystem  # noqa: E402
from qups_amd import eikonal as E  # noqa: E402

HBM = 6.0e12


def wall(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(ts)


def events(fn, reps):
    fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


def example_map():
    z = 1e-3 * np.linspace(-2, 58, 481)
    c = np.full((481, 321), 1500.0)
    for z0, v in ((15e-3, 1400.0), (25e-3, 1600.0), (35e-3, 1400.0), (45e-3, 1500.0)):
        c[z > z0] = v
    return c, 0.125e-3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    from qups_amd import _lib
    say(f"device: {_lib.device_info()['name']}; HBM copy rate taken as {HBM / 1e12:.1f} TB/s; median of {a.reps} after one warm-up")
    say(f"{'grid':>12} {'K':>4} {'solve ms':>9} {'passes':>6} {'cap':>6} {'ms/pass':>8} {'Mnode/s':>9} {'full-pass TB/s':>14} {'% HBM':>6} | {'sampler ms':>10} {'GB':>6} {'% HBM':>6}")
    cases = []
    c1, dp1 = example_map()
    for K in (16, 128):
        x = (np.arange(K) - (K - 1) / 2) * (0.5e-3 if K == 16 else 0.3e-3)      # (128 elements at the example's 0.5 mm would leave its 40 mm grid)
        src = np.stack([np.full(K, 2e-3 / dp1 + 1.0), (x + 20e-3) / dp1 + 1.0])
        cases.append(("481x321", c1, dp1, src))
    n2, dp2 = 1281, 1540.0 / 5e6 / 10
    i, j = np.meshgrid(np.arange(n2) / (n2 - 1), np.arange(n2) / (n2 - 1), indexing="ij")
    c2 = 1540.0 + 60.0 * np.sin(2 * np.pi * 2 * i) * np.cos(2 * np.pi * 1.5 * j) + np.where(i > 0.5, 40.0, 0.0)
    x = (np.arange(128) - 63.5) * 0.3e-3
    cases.append(("1281x1281", c2, dp2, np.stack([np.ones(128), x / dp2 + (n2 + 1) / 2])))
    for name, c, dp, src in cases:
        C1, C2 = c.shape
        K = src.shape[1]
        ct = torch.from_numpy(c).cuda()
        hold = {}

        def solve():
            hold["T"] = E.eikonal(ct, dp, src)
        ms = wall(solve, a.reps)
        passes = E.last_passes()
        nodes = K * C1 * C2
        full = 16.0 * nodes / (ms / passes * 1e-3)
        # the sampler: every node of the grid as a pixel, offset by a third of a cell (a fractional coordinate everywhere but the last line)
        gi, gj = np.meshgrid(np.arange(C1 - 1) + 1.34, np.arange(C2 - 1) + 1.34, indexing="ij")
        Pi = torch.from_numpy(np.stack([gi.ravel(order="F"), gj.ravel(order="F")])).cuda()
        I = Pi.shape[1]
        out = torch.empty((K, I), dtype=torch.float64, device="cuda")
        T = hold["T"]
        Tm = E._maps_colmajor(T, torch)                      # (the tensor the solver returned is already in this layout: no copy is timed)
        Tv = Tm.permute(2, 1, 0)
        sms = events(lambda: E.eikonal_tables(Tv, Pi, out=out), a.reps)
        sbytes = 8.0 * nodes + 16.0 * I + 8.0 * I * K
        say(f"{name:>12} {K:4d} {ms:9.3f} {passes:6d} {E.pass_cap(C1, C2):6d} {ms / passes:8.4f} {nodes / ms / 1e3:9.1f} {full / 1e12:14.3f} {100 * full / HBM:6.1f} | "
            f"{sms:10.4f} {sbytes / 1e9:6.3f} {100 * sbytes / (sms * 1e-3) / HBM:6.1f}")
        del hold, T, Tm, Tv, out
    # ---- end to end beside bfDAS
    N = 128
    lam = 1540.0 / 5e6
    xdc = Transducer.linear(N, 0.3e-3)
    scan = Scan.cartesian(np.linspace(-64 * lam, 64 * lam, 512), np.linspace(0, 128 * lam, 512))
    cgrd = Scan.cartesian(np.linspace(-64 * lam, 64 * lam, n2), np.linspace(0, 128 * lam, n2))
    us = UltrasoundSystem(xdc, Sequence("FSA", c0=1540.0), scan)
    rng = np.random.default_rng(0)
    xd = torch.from_numpy((rng.standard_normal((2048, N, N)) + 1j * rng.standard_normal((2048, N, N))).astype(np.complex64)).cuda()
    chd = ChannelData(xd, 0.0, 25e6)
    cmap = torch.from_numpy(c2.reshape(cgrd.size)).cuda()
    t_das = wall(lambda: us.bfDAS(chd, interp="cubic"), a.reps)
    t_eik = wall(lambda: us.bfEikonal(chd, cmap, cgrd, interp="cubic"), a.reps)
    t_tab = wall(lambda: us.bfEikonal(None, cmap, cgrd, delay_only=True), a.reps)
    say()
    say(f"end to end, {N} elements FSA, 512 x 512 pixels, T = 2048, complex64, cubic; speed map {n2} x {n2} (lambda/10); wall ms, host work included:")
    say(f"  bfDAS {t_das:9.3f} ms   bfEikonal {t_eik:9.3f} ms   of which the tables (delay_only) {t_tab:9.3f} ms")
    # ---- CPU context
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from tests import eikonal_ref as R
    t0 = time.perf_counter()
    R.fmm(c1, dp1, [[17.0], [161.0]])
    say()
    say(f"context: ONE source on 481 x 321 by the float64 heap solve of tests/eikonal_ref.py (a Python restatement, one core of {os.cpu_count()}; "
        f"not the reference's MEX): {(time.perf_counter() - t0) * 1e3:.0f} ms")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
