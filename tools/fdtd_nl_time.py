#!/usr/bin/env python3
"""Time qdas_fdtd_nonlinear (the C entry through ``qups_amd.fdtd.launch`` on prepared tables: device events around the whole step loop) beside the linear
entries in the SAME run, on the shapes of tools/fdtd_loss_time.py (float32, order 8):

  multilayer   801 x 801 nodes, PML 20, 21 plane waves, 1000 steps
  end2end      170 x 200 nodes, PML 20, 32 pulses, 2185 steps

Variants: ``lossless`` (qdas_fdtd), ``stokes`` and ``L3`` (qdas_fdtd_lossy: 0.75 dB/(MHz^y cm), y = 2 and 1.1, fitted over 3 .. 7 MHz), and each of them with
``B/A = 6`` everywhere (``lossless+nl``, ``stokes+nl``, ``L3+nl``: qdas_fdtd_nonlinear), the sources scaled to a source Mach number of 2e-4 for all six (far from
a shock over these paths; the cost per step does not depend on the amplitude, and the linear variants simply carry it).  Per shape and variant: ms per step (the median of interleaved
repeats, every repeat listed: their spread is the run-to-run spread); for a nonlinear variant the time ratio to ITS linear variant of the same run, and
beside it the ratio of the byte models -- per node, step and pulse the lossless passes move 48 B plus 16 B / V for the medium maps, the lossy
density pass adds (2 L + 1) 4 B (4.19), and the nonlinear pass one more 4-byte map read, bq: 52 B against 48 B without absorption.

``--variants lossless,stokes,L3`` times the linear entries alone: with ``QDAS_LIB`` pointing at a library that holds the parent commit's fdtd.hip that is the
A/B run that shows the existing kernels did not move.  A child process per shape under ``timeout``; output -> profiles/fdtd_nl_time.txt."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fdtd_time import SHAPES  # noqa: E402

LINEAR = {"lossless": None, "stokes": (2.0, 0), "L3": (1.1, 3)}
VARIANTS = list(LINEAR) + [v + "+nl" for v in LINEAR]
ALPHA_DB, BAND, BOA, MACH = 0.75, (3e6, 7e6), 6.0, 2e-4


def child(name, reps, variants):
    import numpy as np
    import torch
    from qups_amd import fdtd as F
    from tests import fdtd_ref as R
    sh = SHAPES[name]
    Z, X, P, V, Nt, M = (sh[k] for k in ("Z", "X", "P", "V", "Nt", "M"))
    h = 0.25 * 1540.0 / 7.5e6 if name == "multilayer" else 1e-4
    z, x = np.arange(Z) * h, (np.arange(X) - (X - 1) / 2) * h
    c = R.smooth_map(Z, X, 1400.0, 1680.0, 1)
    rho = R.smooth_map(Z, X, 900.0, 1100.0, 2)
    dt = 0.2 * h / c.max()                                       # (tools/fdtd_loss_time.py's: room for the unrelaxed speed)
    ix = np.linspace(X // 4, 3 * X // 4, M).round().astype(int)
    pos = np.stack([np.zeros(M), x[ix]])
    rng = np.random.default_rng(0)
    n = np.arange(96, dtype=np.float64)[:, None, None]
    dl = rng.uniform(0, 20, (M, V))
    s = np.sin(2 * np.pi * (n - dl[None] - 30) / 24.0) * np.exp(-(((n - dl[None] - 30) / 12.0) ** 2))
    s *= MACH / F.source_mach(s, c, dt, h)
    prep = {}
    for v in variants:
        lin = LINEAR[v.split("+")[0]]
        kw = {} if lin is None else dict(alpha=ALPHA_DB, alpha_power=lin[0], alpha_band=BAND, mechanisms=max(lin[1], 1))
        if v.endswith("+nl"):
            kw["BoA"] = BOA
        prep[v] = F.fdtd(c, rho, z, x, pos, np.stack([np.ones(M), np.zeros(M)]), s, pos, Nt, dt, PML=P, order=8, prec="single", prepare_only=True, **kw)
    Nz, Nx = prep[variants[0]][0]["Nz"], prep[variants[0]][0]["Nx"]

    def kernel_ms(v, nt=None):
        meta, tb, s_dev = prep[v]
        meta = meta if nt is None else dict(meta, Nt=nt)
        st = {k: torch.zeros((V, Nx, meta["ld"]), dtype=torch.float32, device="cuda") for k in F.STATES}
        L = meta["loss"]["L"] if "loss" in meta else 0
        if L:
            st["e"] = torch.zeros((V, L, Nx, meta["ld"]), dtype=torch.float32, device="cuda")
        rec = torch.empty((meta["Nt"], meta["N"], V), dtype=torch.float32, device="cuda")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        F.launch(meta, tb, st, s_dev, rec, 0)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / max(meta["Nt"], 1), rec

    for v in variants:
        kernel_ms(v, 20)                                         # warm-up: code objects, the allocator
    times, recs = {v: [] for v in variants}, {}
    for _ in range(reps):                                        # interleaved
        for v in variants:
            ms, recs[v] = kernel_ms(v)
            times[v].append(ms)
    med = {v: statistics.median(times[v]) for v in variants}
    print(f"{name}: {Z} x {X} nodes + PML {P} = {Nz} x {Nx}, V = {V}, {Nt} steps, fp32, order 8")
    for v in variants:
        base = v.split("+")[0]
        lin = LINEAR[base]
        lin_bytes = 48.0 + 16.0 / V + (0.0 if lin is None else (2 * lin[1] + 1) * 4.0)
        line = f"  {v:12s} {med[v]:8.4f} ms / step   (repeats {', '.join(f'{t:.4f}' for t in times[v])}; spread {100 * (max(times[v]) - min(times[v])) / med[v]:.1f} %)"
        if v.endswith("+nl"):
            if base in med:
                diff = float((recs[v] - recs[base]).abs().max() / recs[base].abs().max())
                line += f"   time ratio to {base} {med[v] / med[base]:.3f}, byte-model ratio {(lin_bytes + 4.0) / lin_bytes:.3f}   |record - linear record| / max {diff:.2e}"
            assert bool(torch.isfinite(recs[v]).all())
        print(line)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated shape names")
    ap.add_argument("--variants", default=",".join(VARIANTS), help="comma-separated: " + ", ".join(VARIANTS))
    ap.add_argument("--child", default="")
    a = ap.parse_args()
    variants = [v for v in a.variants.split(",") if v]
    if any(v not in VARIANTS for v in variants) or not variants:
        ap.error(f"variants are {', '.join(VARIANTS)}")
    if a.child:
        child(a.child, a.reps, variants)
        return 0
    print("qdas_fdtd_nonlinear beside qdas_fdtd and qdas_fdtd_lossy, one MI355X, device events around the whole step loop")
    rc = 0
    for name in SHAPES:
        if a.only and name not in a.only.split(","):
            continue
        sys.stdout.flush()
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps),
                            "--variants", ",".join(variants)], cwd=ROOT)
        if r.returncode:
            print(f"{name}: the child ended with status {r.returncode}")
            rc = r.returncode
            break                                               # nothing more is started on the device after a failure
    return rc


if __name__ == "__main__":
    sys.exit(main())
