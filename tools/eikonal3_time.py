"""Time the 3-D eikonal solver (qdas_eikonal3) and its table sampler (qdas_eikonal3_tables).  Needs an MI355X; there is nothing to fall back to.

    python tools/eikonal3_time.py [--reps 3] [--grids 65,129,161x161x241] [--sources 16,256] [--out profiles/eikonal3_time.txt]

Grids of 65^3, 129^3 and 161 x 161 x 241 nodes under a smooth speed volume (1540 m/s +- 60 with a 40 m/s step half way down dimension 1); the sources are the
elements of a 4 x 4 or 16 x 16 matrix array on the face dimension 1 = 1, spread over the middle half of that face.  Per row: wall ms of one solve batch
(a host clock around the call, which waits for its stream: it ends when the host has seen an empty list), passes taken and their cap, nodes solved per
second (K C1 C2 C3 / time), the LIST SHARE -- tile visits over K x tiles x passes, i.e. the share of (set, tile) pairs on the list in the mean pass; a solver
that launched a workgroup per pair and pass would sit at 1 -- and the sampler alone (device events) at every second node in each dimension, offset by a third of a
cell: 64 taps per pixel and map.  Median of --reps after one warm-up; the spread (min .. max) of the solve is printed beside it."""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from qups_amd import _lib  # noqa: E402
from qups_amd import eikonal as E  # noqa: E402


def speed(shape):
    i, j, l = np.meshgrid(*(np.arange(n) / (n - 1) for n in shape), indexing="ij")
    return 1540.0 + 60.0 * np.sin(2 * np.pi * 2 * i) * np.cos(2 * np.pi * 1.5 * j) * np.cos(2 * np.pi * l) + np.where(i > 0.5, 40.0, 0.0)


def sources(shape, K):
    n = int(round(K ** 0.5))
    assert n * n == K
    a, b = np.meshgrid(np.linspace(0.25 * shape[1], 0.75 * shape[1], n), np.linspace(0.25 * shape[2], 0.75 * shape[2], n), indexing="ij")
    return np.stack([np.ones(K), a.ravel(order="F") + 1.0, b.ravel(order="F") + 1.0])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--grids", default="65,129,161x161x241")
    ap.add_argument("--sources", default="16,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eikonal3_time: no HIP device -- nothing is measured without one")
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)

    dp = 1540.0 / 5e6 / 4                                    # lambda / 4 at 5 MHz
    say(f"device: {_lib.device_info()['name']}; double precision; median of {a.reps} after one warm-up (min .. max of the solve beside it)")
    say(f"{'grid':>12} {'K':>4} {'solve ms':>10} {'min .. max':>19} {'passes':>6} {'cap':>6} {'Mnode/s':>9} {'visits':>10} {'list share':>10} | {'pixels':>9} {'sampler ms':>10} {'Gtap/s':>7}")
    for g in a.grids.split(","):
        shape = tuple(int(v) for v in g.split("x")) if "x" in g else (int(g),) * 3
        ct = torch.from_numpy(speed(shape)).cuda()
        tiles = int(np.prod([-(-n // 8) for n in shape]))
        for K in (int(v) for v in a.sources.split(",")):
            src = sources(shape, K)
            hold = {}

            def solve():
                hold["T"] = None                             # (one batch of maps at a time: 256 maps of 161 x 161 x 241 are 12.8 GB)
                hold["T"] = E.eikonal3(ct, dp, src)
            solve()
            torch.cuda.synchronize()
            ts = []
            for _ in range(a.reps):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                solve()
                torch.cuda.synchronize()
                ts.append((time.perf_counter() - t0) * 1e3)
            ms, passes, visits = statistics.median(ts), E.eikonal3.last_passes, E.eikonal3.last_visits
            nodes = K * int(np.prod(shape))
            T = hold["T"]
            gg = np.meshgrid(*(np.arange(0, n - 1, 2) + 1.34 for n in shape), indexing="ij")
            Pi = torch.from_numpy(np.stack([x.ravel(order="F") for x in gg])).cuda()
            I = Pi.shape[1]
            out = torch.empty((K, I), dtype=torch.float64, device="cuda")
            E.eikonal3_tables(T, Pi, out=out)
            torch.cuda.synchronize()
            es = []
            for _ in range(a.reps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                E.eikonal3_tables(T, Pi, out=out)
                e1.record()
                torch.cuda.synchronize()
                es.append(e0.elapsed_time(e1))
            sms = statistics.median(es)
            assert bool(torch.isfinite(T).all()) and bool(torch.isfinite(out).all())
            say(f"{g:>12} {K:4d} {ms:10.3f} {min(ts):9.3f} ..{max(ts):8.3f} {passes:6d} {E.pass_cap3(*shape):6d} {nodes / ms / 1e3:9.1f} {visits:10d} "
                f"{visits / (K * tiles * passes):10.3f} | {I:9d} {sms:10.4f} {64.0 * I * K / (sms * 1e-3) / 1e9:7.1f}")
            del hold, T, out, Pi
    say()
    say("context, not a threshold: the 2-D solver's table (profiles/eikonal_time.txt) reaches 3.2e9 nodes/s at 1281 x 1281 x 128 sources.")
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
