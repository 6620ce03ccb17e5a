#!/usr/bin/env python3
"""Time qdas_fdtd_lossy (the C entry through ``qups_amd.fdtd.launch`` on prepared tables: device events around the whole step loop) beside qdas_fdtd in the
SAME run and beside a torch composition of the same arithmetic, on the shapes of tools/fdtd_time.py (float32, order 8):

  multilayer   801 x 801 nodes, PML 20, 21 plane waves, 1000 steps
  end2end      170 x 200 nodes, PML 20, 32 pulses, 2185 steps

Variants: ``lossless`` (qdas_fdtd), ``stokes`` (L = 0), ``L1`` and ``L3`` (relaxation), 0.75 dB/(MHz^y cm) everywhere, y = 2 and 1.1, fitted over 3 .. 7 MHz.
Per shape and variant: ms per step (the median of interleaved repeats, every repeat listed: their spread is the run-to-run spread), the ratio to the lossless
kernel of the same run, and beside it the ratio of the byte models -- per node, step and pulse the lossless passes move 48 B plus 16 B / V
for the medium maps, and the lossy density pass adds (2 L + 1) 4 B: each memory variable read and written, the loss map read.  Then the torch composition of
the lossy step over ``--steps-torch`` steps and the largest difference between the two records.

``--variants lossless`` times qdas_fdtd alone: with ``QDAS_LIB`` pointing at a build of the parent commit that is the A/B run that shows its kernels did not
move.  A child process per shape under ``timeout``; output -> profiles/fdtd_loss_time.txt."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from fdtd_time import COEF, SHAPES  # noqa: E402

VARIANTS = {"lossless": None, "stokes": (2.0, 0), "L1": (1.1, 1), "L3": (1.1, 3)}
ALPHA_DB, BAND = 0.75, (3e6, 7e6)


def torch_scheme(tb, meta, s, V, Nt, torch):
    """tools/fdtd_time.py's composition with the lossy step 4 (``meta["loss"]``: mode, g, E; ``tb["kap"]``)"""
    Nz, Nx = meta["Nz"], meta["Nx"]
    dev = s.device

    def sh(f, k, dim):
        if k == 0:
            return f
        g = torch.roll(f, -k, dim)
        idx = [slice(None)] * 3
        idx[dim] = slice(f.shape[dim] - k, None) if k > 0 else slice(0, -k)
        g[tuple(idx)] = 0
        return g

    def dplus(f, dim):
        d = torch.zeros_like(f)
        for k in range(1, 5):
            d += COEF[k - 1] * (sh(f, k, dim) - sh(f, 1 - k, dim))
        return d

    def dminus(g, dim):
        d = torch.zeros_like(g)
        for k in range(1, 5):
            d += COEF[k - 1] * (sh(g, k - 1, dim) - sh(g, -k, dim))
        return d

    m2 = lambda k: tb[k].reshape(1, Nx, Nz)
    wz_map, wx_map = m2("dtrz") * meta["inv_h"], m2("dtrx") * meta["inv_h"]
    wr = m2("rho") * meta["dt_h"]
    az, azs = tb["az"].reshape(1, 1, Nz), tb["azs"].reshape(1, 1, Nz)
    ax, axs = tb["ax"].reshape(1, Nx, 1), tb["axs"].reshape(1, Nx, 1)
    sj, si = (tb["src_node"] // Nz).long(), (tb["src_node"] % Nz).long()
    nj, ni = (tb["sen_node"] // Nz).long(), (tb["sen_node"] % Nz).long()
    loss = meta["loss"]
    L, kap = int(loss["L"]), m2("kap")
    g, E = [float(v) for v in loss["g"]], [float(v) for v in loss["E"]]
    p, uz, ux, rz, rx = (torch.zeros((V, Nx, Nz), dtype=torch.float32, device=dev) for _ in range(5))
    e = [torch.zeros((V, Nx, Nz), dtype=torch.float32, device=dev) for _ in range(L)]
    rec = torch.empty((Nt, meta["N"], V), dtype=torch.float32, device=dev)
    for n in range(Nt):
        uz = azs * (azs * uz - wz_map * dplus(p, 2))
        ux = axs * (axs * ux - wx_map * dplus(p, 1))
        if n < meta["Ts"]:
            uz[:, sj, si] += (tb["src_wz"][:, None] * s[n]).T
            ux[:, sj, si] += (tb["src_wx"][:, None] * s[n]).T
        ro = rz + rx
        rz = az * (az * rz - wr * dminus(uz, 2))
        rx = ax * (ax * rx - wr * dminus(ux, 1))
        rn = rz + rx
        if L == 0:
            acc = rn - ro
        else:
            acc = torch.zeros_like(rn)
            for l in range(L):
                e[l] = e[l] + E[l] * (rn - e[l])
                acc = acc + g[l] * (rn - e[l])
        p = m2("c2") * (rn + kap * acc)
        rec[n] = p[:, nj, ni].T
    return rec


def child(name, reps, steps_torch, variants):
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
    dt = 0.2 * h / c.max()                                       # (0.2 and not tools/fdtd_time.py's 0.25: room for the unrelaxed speed; the cost per step does not depend on it)
    ix = np.linspace(X // 4, 3 * X // 4, M).round().astype(int)
    pos = np.stack([np.zeros(M), x[ix]])
    rng = np.random.default_rng(0)
    n = np.arange(96, dtype=np.float64)[:, None, None]
    dl = rng.uniform(0, 20, (M, V))
    s = np.sin(2 * np.pi * (n - dl[None] - 30) / 24.0) * np.exp(-(((n - dl[None] - 30) / 12.0) ** 2))
    prep = {}
    for v in variants:
        kw = {} if VARIANTS[v] is None else dict(alpha=ALPHA_DB, alpha_power=VARIANTS[v][0], alpha_band=BAND, mechanisms=max(VARIANTS[v][1], 1))
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

    def torch_ms(v, nsteps):
        meta, tb, s_dev = prep[v]
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        rec = torch_scheme(tb, meta, s_dev, V, nsteps, torch)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / nsteps, rec

    for v in variants:
        kernel_ms(v, 20)                                         # warm-up: code objects, the allocator
    times, recs = {v: [] for v in variants}, {}
    for _ in range(reps):                                        # interleaved
        for v in variants:
            ms, recs[v] = kernel_ms(v)
            times[v].append(ms)
    med = {v: statistics.median(times[v]) for v in variants}
    base_bytes = 48.0 + 16.0 / V
    print(f"{name}: {Z} x {X} nodes + PML {P} = {Nz} x {Nx}, V = {V}, {Nt} steps, fp32, order 8")
    for v in variants:
        L = 0 if VARIANTS[v] is None else VARIANTS[v][1]
        extra = 0.0 if VARIANTS[v] is None else (2 * L + 1) * 4.0
        line = f"  {v:9s} {med[v]:8.4f} ms / step   (repeats {', '.join(f'{t:.4f}' for t in times[v])}; spread {100 * (max(times[v]) - min(times[v])) / med[v]:.1f} %)"
        if "lossless" in med and v != "lossless":
            line += f"   time ratio {med[v] / med['lossless']:.3f}, byte-model ratio {(base_bytes + extra) / base_bytes:.3f}"
        if VARIANTS[v] is not None:
            line += f"   fit_err {prep[v][0]['loss']['fit_err']:.2e}"
        print(line)
    for v in variants:
        if VARIANTS[v] is None or steps_torch <= 0:
            continue
        torch_ms(v, 3)
        t_ms, rec_t = torch_ms(v, steps_torch)
        diff = float((recs[v][:steps_torch] - rec_t).abs().max() / rec_t.abs().max())
        print(f"  torch composition, {v:7s} {t_ms:8.4f} ms / step over {steps_torch} steps   ratio {t_ms / med[v]:.1f} x   largest |record difference| / max {diff:.2e}")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated shape names")
    ap.add_argument("--variants", default=",".join(VARIANTS), help="comma-separated: " + ", ".join(VARIANTS))
    ap.add_argument("--child", default="")
    ap.add_argument("--steps-torch", type=int, default=100, help="steps of the torch composition (its cost per step does not depend on the step); 0: none")
    a = ap.parse_args()
    variants = [v for v in a.variants.split(",") if v]
    if any(v not in VARIANTS for v in variants) or not variants:
        ap.error(f"variants are {', '.join(VARIANTS)}")
    if a.child:
        child(a.child, a.reps, a.steps_torch, variants)
        return 0
    print("qdas_fdtd_lossy beside qdas_fdtd and a torch composition of the same arithmetic, one MI355X, device events around the whole step loop")
    rc = 0
    for name in SHAPES:
        if a.only and name not in a.only.split(","):
            continue
        sys.stdout.flush()
        r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps),
                            "--steps-torch", str(a.steps_torch), "--variants", ",".join(variants)], cwd=ROOT)
        if r.returncode:
            print(f"{name}: the child ended with status {r.returncode}")
            rc = r.returncode
            break                                               # nothing more is started on the device after a failure
    return rc


if __name__ == "__main__":
    sys.exit(main())
