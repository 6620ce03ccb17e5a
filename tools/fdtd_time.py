#!/usr/bin/env python3
"""Time qdas_fdtd (the C entry through ``qups_amd.fdtd.launch`` on prepared tables: device events around the whole step loop) beside a torch composition of
the SAME scheme -- slicing and ``torch.roll``, float32, the same V, exactly the same arithmetic (the derivative sums term by term, both PML updates, the
additive source, p = c^2 (rz + rx), the sensor gather) -- on two shapes:

  multilayer   the grid of the reference's examples/simulation/multilayer_media.m: lambda / 4 at 7.5 MHz, 801 x 801 nodes, PML 20, 21 plane waves, 1000 steps
  end2end      the end-to-end test's shape: 170 x 200 nodes, PML 20, 32 pulses (FSA), 2185 steps

Per shape: ms per step of both paths (the median of interleaved repeats), the bytes per step under the model of csrc/fdtd.hip -- per node, step and pulse
fp32 the velocity pass reads p, uz, ux and writes uz, ux (20 B), the density pass reads uz, ux, rz, rx and writes rz, rx, p (28 B), the four medium maps
add 16 B / V -- the rate that makes and its share of the 8 TB/s HBM roof, the largest difference between the two records, and, on the small shape, the
launch share: the same 2 Nt launches on a grid of ONE tile and one pulse (nothing to compute: the cost of enqueuing and starting two kernels per step)
over the time of the small shape.  A child process per shape under ``timeout``; output -> profiles/fdtd_time.txt."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"multilayer": dict(Z=801, X=801, P=20, V=21, Nt=1000, M=64), "end2end": dict(Z=170, X=200, P=20, V=32, Nt=2185, M=32)}
ROOF = 8.0e12
COEF = (1225.0 / 1024.0, -245.0 / 3072.0, 49.0 / 5120.0, -5.0 / 7168.0)


def torch_scheme(tb, meta, s, V, Nt, torch):
    """the composition: states V x Nx x Nz, z is dim 2; a shift is a roll with the wrapped slice zeroed"""
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
    p, uz, ux, rz, rx = (torch.zeros((V, Nx, Nz), dtype=torch.float32, device=dev) for _ in range(5))
    rec = torch.empty((Nt, meta["N"], V), dtype=torch.float32, device=dev)
    for n in range(Nt):
        uz = azs * (azs * uz - wz_map * dplus(p, 2))
        ux = axs * (axs * ux - wx_map * dplus(p, 1))
        if n < meta["Ts"]:
            uz[:, sj, si] += (tb["src_wz"][:, None] * s[n]).T
            ux[:, sj, si] += (tb["src_wx"][:, None] * s[n]).T
        rz = az * (az * rz - wr * dminus(uz, 2))
        rx = ax * (ax * rx - wr * dminus(ux, 1))
        p = m2("c2") * (rz + rx)
        rec[n] = p[:, nj, ni].T
    return rec


def child(name, reps, steps_torch):
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
    dt = 0.25 * h / c.max()
    ix = np.linspace(X // 4, 3 * X // 4, M).round().astype(int)
    pos = np.stack([np.zeros(M), x[ix]])
    rng = np.random.default_rng(0)
    n = np.arange(96, dtype=np.float64)[:, None, None]
    dl = rng.uniform(0, 20, (M, V))
    s = np.sin(2 * np.pi * (n - dl[None] - 30) / 24.0) * np.exp(-(((n - dl[None] - 30) / 12.0) ** 2))
    meta, tb, s_dev = F.fdtd(c, rho, z, x, pos, np.stack([np.ones(M), np.zeros(M)]), s, pos, Nt, dt, PML=P, order=8, prec="single", prepare_only=True)
    Nz, Nx = meta["Nz"], meta["Nx"]

    def kernel_ms(meta_, tb_, s_, V_):
        st = {k: torch.zeros((V_, meta_["Nx"], meta_["ld"]), dtype=torch.float32, device="cuda") for k in F.STATES}
        rec = torch.empty((meta_["Nt"], meta_["N"], V_), dtype=torch.float32, device="cuda")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        F.launch(meta_, tb_, st, s_, rec, 0)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / max(meta_["Nt"], 1), rec

    def torch_ms(nsteps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        rec = torch_scheme(tb, meta, s_dev, V, nsteps, torch)
        b.record()
        b.synchronize()
        return a.elapsed_time(b) / nsteps, rec

    kernel_ms(dict(meta, Nt=20), tb, s_dev, V)                  # warm-up: code objects, the allocator
    torch_ms(5)
    tk, tt = [], []
    for _ in range(reps):                                       # interleaved
        ms, rec_k = kernel_ms(meta, tb, s_dev, V)
        tk.append(ms)
        ms, rec_t = torch_ms(steps_torch)
        tt.append(ms)
    diff = float((rec_k[:steps_torch] - rec_t).abs().max() / rec_t.abs().max())
    k_ms, t_ms = statistics.median(tk), statistics.median(tt)
    bytes_step = Nz * Nx * (V * 48 + 16)
    rate = bytes_step / (k_ms * 1e-3)
    print(f"{name}: {Z} x {X} nodes + PML {P} = {Nz} x {Nx}, V = {V}, {Nt} steps, fp32, order 8")
    print(f"  qdas_fdtd          {k_ms:8.4f} ms / step   (repeats {', '.join(f'{v:.4f}' for v in tk)}; {k_ms * Nt:.1f} ms the call)")
    print(f"  torch composition  {t_ms:8.4f} ms / step   (repeats {', '.join(f'{v:.4f}' for v in tt)}; over {steps_torch} steps)   ratio {t_ms / k_ms:.1f} x")
    print(f"  bytes / step under the model: {bytes_step / 1e6:.1f} MB -> {rate / 1e12:.2f} TB/s, {100 * rate / ROOF:.1f} % of the 8 TB/s HBM roof")
    print(f"  largest |record difference| / max over the first {steps_torch} steps: {diff:.2e}")
    if name == "end2end":
        # the launches alone: one tile, one pulse, the same number of steps
        c1, r1 = np.full((16, 8), 1500.0), np.full((16, 8), 1000.0)
        z1, x1 = np.arange(16) * h, np.arange(8) * h
        p1 = np.array([[z1[3]], [x1[3]]])
        m1, t1, s1 = F.fdtd(c1, r1, z1, x1, p1, np.array([[1.0], [0.0]]), s[:, :1, :1], p1, Nt, 0.25 * h / 1500.0, PML=0, order=8, prec="single", prepare_only=True)
        kernel_ms(dict(m1, Nt=20), t1, s1, 1)
        tl = statistics.median(kernel_ms(m1, t1, s1, 1)[0] for _ in range(reps))
        print(f"  two launches per step on one tile and one pulse: {tl * 1e3:.2f} us / step -> the launch share of this shape is {100 * tl / k_ms:.0f} %")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated shape names")
    ap.add_argument("--child", default="")
    ap.add_argument("--steps-torch", type=int, default=200, help="steps of the torch composition per repeat (its cost per step does not depend on the step)")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.steps_torch)
        return 0
    print("qdas_fdtd beside a torch composition of the same scheme, one MI355X, device events around the whole step loop")
    rc = 0
    for name in SHAPES:
        if a.only and name not in a.only.split(","):
            continue
        sys.stdout.flush()
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps),
                            "--steps-torch", str(a.steps_torch)], cwd=ROOT)
        if r.returncode:
            print(f"{name}: the child ended with status {r.returncode}")
            rc = r.returncode
            break                                               # nothing more is started on the device after a failure
    return rc


if __name__ == "__main__":
    sys.exit(main())
