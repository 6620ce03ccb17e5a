#!/usr/bin/env python3
"""Time qdas_fdtd3 (the C entry through ``qups_amd.fdtd3.launch`` on prepared tables: device events around the whole step loop) beside a torch composition of
the SAME scheme -- slicing and ``torch.roll``, float32, the same V, exactly the same arithmetic (the derivative sums term by term, the six PML updates, the
additive source, p = c^2 ((rz + rx) + ry), the sensor gather) -- the 3-D twin of tools/fdtd_time.py, on three shapes:

  cube1        128^3 nodes + PML 10 = 148^3, 1 pulse
  cube16       the same with 16 pulses
  end2end      the end-to-end test's shape: 101 x 41 x 41 nodes + PML 10, 16 pulses (FSA, 4 x 4 elements), 1016 steps

Per shape: ms per step of both paths (the median of interleaved repeats), the bytes per step under the model of csrc/fdtd3.hip -- per node, step and pulse
fp32 the velocity pass reads p, uz, ux, uy and writes uz, ux, uy (28 B), the density pass reads the three u and the three r and writes the three r and p
(40 B), the five medium maps add 20 B / V; the z / x halo of a plane and the planes beyond a brick's ends are assumed to hit L2 and are NOT counted -- the rate
that makes and its share of the 8 TB/s HBM roof, the largest difference between the two records, and, on the small shape, the launch share: the same 2 Nt
launches on a grid of ONE brick and one pulse over the time of the small shape.  ``--no-torch`` times the entry alone (brick candidates: QDAS_LIB names the
library).  A child process per shape under ``timeout``; output -> profiles/fdtd3_time.txt."""
import argparse
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"cube1": dict(Z=128, X=128, Y=128, P=10, V=1, Nt=200, M=16), "cube16": dict(Z=128, X=128, Y=128, P=10, V=16, Nt=100, M=16),
          "end2end": dict(Z=101, X=41, Y=41, P=10, V=16, Nt=1016, M=16)}
ROOF = 8.0e12
COEF = (1225.0 / 1024.0, -245.0 / 3072.0, 49.0 / 5120.0, -5.0 / 7168.0)


def torch_scheme(tb, meta, s, V, Nt, torch):
    """the composition: states V x Ny x Nx x Nz, z is dim 3; a shift is a roll with the wrapped slice zeroed"""
    Nz, Nx, Ny = meta["Nz"], meta["Nx"], meta["Ny"]
    dev = s.device

    def sh(f, k, dim):
        if k == 0:
            return f
        g = torch.roll(f, -k, dim)
        idx = [slice(None)] * 4
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

    m3 = lambda k: tb[k].reshape(1, Ny, Nx, Nz)
    DIM = {"z": 3, "x": 2, "y": 1}
    wu = {a: m3("dtr" + a) * meta["inv_h"] for a in DIM}
    wr = m3("rho") * meta["dt_h"]
    shp = {"z": (1, 1, 1, Nz), "x": (1, 1, Nx, 1), "y": (1, Ny, 1, 1)}
    A = {a: tb["a" + a].reshape(shp[a]) for a in DIM}
    As = {a: tb["a" + a + "s"].reshape(shp[a]) for a in DIM}
    split = lambda node: ((node // Nz // Nx).long(), (node // Nz % Nx).long(), (node % Nz).long())
    sk, sj, si = split(tb["src_node"])
    nk, nj, ni = split(tb["sen_node"])
    p = torch.zeros((V, Ny, Nx, Nz), dtype=torch.float32, device=dev)
    u = {a: torch.zeros_like(p) for a in DIM}
    r = {a: torch.zeros_like(p) for a in DIM}
    rec = torch.empty((Nt, meta["N"], V), dtype=torch.float32, device=dev)
    for n in range(Nt):
        for a in DIM:
            u[a] = As[a] * (As[a] * u[a] - wu[a] * dplus(p, DIM[a]))
            if n < meta["Ts"]:
                u[a][:, sk, sj, si] += (tb["src_w" + a][:, None] * s[n]).T
        for a in DIM:
            r[a] = A[a] * (A[a] * r[a] - wr * dminus(u[a], DIM[a]))
        p = m3("c2") * ((r["z"] + r["x"]) + r["y"])
        rec[n] = p[:, nk, nj, ni].T
    return rec


def child(name, reps, steps_torch, no_torch):
    import numpy as np
    import torch
    from qups_amd import fdtd3 as F3
    from tests import fdtd3_ref as R3
    sh = SHAPES[name]
    Z, X, Y, P, V, Nt, M = (sh[k] for k in ("Z", "X", "Y", "P", "V", "Nt", "M"))
    h = 1e-4
    z, x, y = np.arange(Z) * h, (np.arange(X) - (X - 1) / 2) * h, (np.arange(Y) - (Y - 1) / 2) * h
    c = R3.smooth_map(Z, X, Y, 1400.0, 1680.0, 1)
    rho = R3.smooth_map(Z, X, Y, 900.0, 1100.0, 2)
    dt = 0.25 * h / c.max()
    q = int(round(M ** 0.5))
    ix, iy = np.meshgrid(np.linspace(X // 4, 3 * X // 4, q).round().astype(int), np.linspace(Y // 4, 3 * Y // 4, q).round().astype(int), indexing="ij")
    pos = np.stack([x[ix.reshape(-1)], y[iy.reshape(-1)], np.zeros(M)])
    rng = np.random.default_rng(0)
    n = np.arange(96, dtype=np.float64)[:, None, None]
    dl = rng.uniform(0, 20, (M, V))
    s = np.sin(2 * np.pi * (n - dl[None] - 30) / 24.0) * np.exp(-(((n - dl[None] - 30) / 12.0) ** 2))
    nrm = np.stack([np.ones(M), np.zeros(M), np.zeros(M)])
    meta, tb, s_dev = F3.fdtd3(c, rho, z, x, y, pos, nrm, s, pos, Nt, dt, PML=P, order=8, prec="single", prepare_only=True)
    Nz, Nx, Ny = meta["Nz"], meta["Nx"], meta["Ny"]

    def kernel_ms(meta_, tb_, s_, V_):
        st = {k: torch.zeros((V_, meta_["Ny"], meta_["Nx"], meta_["ld"]), dtype=torch.float32, device="cuda") for k in F3.STATES}
        rec = torch.empty((meta_["Nt"], meta_["N"], V_), dtype=torch.float32, device="cuda")
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        F3.launch(meta_, tb_, st, s_, rec, 0)
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
    if not no_torch:
        torch_ms(3)
    tk, tt = [], []
    for _ in range(reps):                                       # interleaved
        ms, rec_k = kernel_ms(meta, tb, s_dev, V)
        tk.append(ms)
        if not no_torch:
            ms, rec_t = torch_ms(steps_torch)
            tt.append(ms)
    k_ms = statistics.median(tk)
    nodes = Nz * Nx * Ny
    bytes_step = nodes * (V * 68 + 20)
    rate = bytes_step / (k_ms * 1e-3)
    print(f"{name}: {Z} x {X} x {Y} nodes + PML {P} = {Nz} x {Nx} x {Ny}, V = {V}, {Nt} steps, fp32, order 8, brick {F3.BRICK[0]} x {F3.BRICK[1]} x {F3.BRICK[2]}"
          f"{' (' + os.path.basename(os.environ['QDAS_LIB']) + ')' if os.environ.get('QDAS_LIB') else ''}")
    print(f"  qdas_fdtd3         {k_ms:8.4f} ms / step   (repeats {', '.join(f'{v:.4f}' for v in tk)}; {k_ms * Nt:.1f} ms the call)")
    if not no_torch:
        t_ms = statistics.median(tt)
        diff = float((rec_k[:steps_torch] - rec_t).abs().max() / rec_t.abs().max())
        print(f"  torch composition  {t_ms:8.4f} ms / step   (repeats {', '.join(f'{v:.4f}' for v in tt)}; over {steps_torch} steps)   ratio {t_ms / k_ms:.1f} x")
        print(f"  largest |record difference| / max over the first {steps_torch} steps: {diff:.2e}")
    print(f"  bytes / step under the model: {bytes_step / 1e6:.1f} MB -> {rate / 1e12:.2f} TB/s, {100 * rate / ROOF:.1f} % of the 8 TB/s HBM roof")
    if name == "end2end":
        # the launches alone: one brick, one pulse, the same number of steps
        c1, r1 = np.full((16, 4, 4), 1500.0), np.full((16, 4, 4), 1000.0)
        z1, x1 = np.arange(16) * h, np.arange(4) * h
        p1 = np.array([[x1[1]], [x1[2]], [z1[3]]])
        m1, t1, s1 = F3.fdtd3(c1, r1, z1, x1, x1, p1, np.array([[1.0], [0.0], [0.0]]), s[:, :1, :1], p1, Nt, 0.25 * h / 1500.0, PML=0, order=8, prec="single",
                              prepare_only=True)
        kernel_ms(dict(m1, Nt=20), t1, s1, 1)
        tl = statistics.median(kernel_ms(m1, t1, s1, 1)[0] for _ in range(reps))
        print(f"  two launches per step on one brick and one pulse: {tl * 1e3:.2f} us / step -> the launch share of this shape is {100 * tl / k_ms:.0f} %")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated shape names")
    ap.add_argument("--child", default="")
    ap.add_argument("--steps-torch", type=int, default=20, help="steps of the torch composition per repeat (its cost per step does not depend on the step)")
    ap.add_argument("--no-torch", action="store_true", help="time the entry alone")
    a = ap.parse_args()
    if a.child:
        child(a.child, a.reps, a.steps_torch, a.no_torch)
        return 0
    if not a.no_torch:
        print("qdas_fdtd3 beside a torch composition of the same scheme, one MI355X, device events around the whole step loop")
    rc = 0
    for name in SHAPES:
        if a.only and name not in a.only.split(","):
            continue
        sys.stdout.flush()
        r = subprocess.run(["timeout", "-k", "10", "240", sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps),
                            "--steps-torch", str(a.steps_torch)] + (["--no-torch"] if a.no_torch else []), cwd=ROOT)
        if r.returncode:
            print(f"{name}: the child ended with status {r.returncode}")
            rc = r.returncode
            break                                               # nothing more is started on the device after a failure
    return rc


if __name__ == "__main__":
    sys.exit(main())
