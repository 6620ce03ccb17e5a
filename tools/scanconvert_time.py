#!/usr/bin/env python3
"""Times the scan conversion on one device: ``qdas_scanconvert`` (one launch: coordinates, cells, ``pre`` and the lerps) beside the composition a user of
torch writes without it -- float64 coordinates of the Cartesian grid, ``torch.searchsorted`` on the source axes, the weights, then per page the envelope /
log compression of the image, four (eight) gathers and the lerps.

* workloads: ``c5-1`` the C5 image (512 x 1024 complex64, the axes of ``qups_amd/configs.py``) onto its ``cartesian_of_polar`` grid with ``pre = "db"``,
  one page; ``c5-32`` the same with 32 pages; ``sph-256`` a spherical volume of 256 x 64 x 64 (complex64, ``pre = "db"``) onto its enclosing grid;
* three figures per workload: the C entry with a prepared descriptor, the Python wrapper ``scan_convert`` / ``scan_convert3`` (device axes,
  ``check_grid=False``: it stages nothing and synchronises nothing) and the composition; for ``c5-1`` also the same C call onto a 1 x 1 grid -- what a launch
  costs by itself, since that call is expected to be launch-bound;
* each workload runs in a child process of its own under ``timeout -k 10 <s>``; a child that ends on a signal, an abort or its time limit ends the tool with
  a non-zero status: nothing more is started on a card after a fault.  This process never opens the device;
* in a child: warm-up, then device events around windows of ``--inner`` back-to-back calls, the paths interleaved, the median per call of ``--reps`` windows
  with the smallest and the largest beside it; the entry's result is compared with the composition's (``max |a - b| / max |b|`` inside, identical masks);
* the byte model: the source read once and the output written once.

    python tools/scanconvert_time.py [--small] [--reps 7] [--inner 20] > profiles/scanconvert_time.txt
"""
import argparse
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_TBS = 8.0          # MI355X peak HBM3E rate, TB/s
CHILD_LIMIT_S = 240
FAULT_STATUS = (124, 134, 137, 139)                     # time limit (timeout's own codes), abort, kill, segmentation fault
WORKLOADS = ("c5-1", "c5-32", "sph-256")
DB_FLOOR = -120.0


def workload(name, small):
    """``(kind, axes in degrees / metres, origin, pages)``"""
    from qups_amd import geometry as G
    if name.startswith("c5"):
        R = 49.57e-3
        nr, na = (64, 128) if small else (512, 1024)
        r, a = np.linspace(R, R + 150e-3, nr), np.linspace(-37, 37, na)
        og = (0.0, 0.0, -R)
        x, y, z = G.cartesian_of_polar(r, a, og)
        return 2, dict(r=r, a=a, x=x, z=z), og, (1 if name == "c5-1" else (4 if small else 32))
    n = (32, 16, 16) if small else (256, 64, 64)
    r, a, e = np.linspace(5e-3, 69e-3, n[0]), np.linspace(-25, 25, n[1]), np.linspace(-25, 25, n[2])
    og = (0.0, 0.0, 0.0)
    x, y, z = G.cartesian_of_spherical(r, a, e, og)
    return 3, dict(r=r, a=a, e=e, x=x, y=y, z=z), og, 1


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


def child(name, small, reps, inner):
    import torch
    if not torch.cuda.is_available():
        sys.exit("scanconvert_time: no HIP device visible -- nothing is measured without one")
    from qups_amd import _lib
    from qups_amd import scanconvert as SC
    dev = torch.device("cuda:0")
    kind, ax, og, P = workload(name, small)
    src_names = ("r", "a", "e")[:kind]
    shape = tuple(ax[k].size for k in src_names)
    g = torch.Generator(device=dev).manual_seed(1)
    b = torch.randn((P,) + tuple(reversed(shape)) + (2,), dtype=torch.float32, device=dev, generator=g)
    b = torch.view_as_complex(b).permute(*reversed(range(kind + 1)))                               # R x A [x E] x P, R fastest: the view DAS returns
    b[1::7, ::5] = 0                                                                               # exact zeros, as outside the support of a DAS image
    deg = {k: torch.from_numpy(ax[k]).to(dev) for k in ax}                                         # as the wrapper takes them
    rad = {k: (deg[k] * math.pi / 180 if k in ("a", "e") else deg[k]) for k in ax}                 # as the C ABI takes them
    out_names = ("z", "x", "y")[:kind]
    oshape = tuple(ax[k].size for k in out_names) + (P,)

    def desc(Z=None, X=None):
        d = _lib.ScanconvertDesc()
        d.R, d.A, d.E = shape[0], shape[1], (shape[2] if kind == 3 else 0)
        d.Z, d.X, d.Y, d.P = (Z or ax["z"].size), (X or ax["x"].size), (ax["y"].size if kind == 3 else 0), P
        d.sr, d.sa, d.se, d.sp = b.stride(0), b.stride(1), (b.stride(2) if kind == 3 else 0), b.stride(kind)
        d.dtype, d.cplx, d.pre, d.device = _lib.QDAS_F32, 1, _lib.SC_PRE_DB, 0
        d.origin[0], d.origin[1], d.origin[2] = og
        d.fill, d.db_floor = math.nan, DB_FLOOR
        for k, t in rad.items():
            setattr(d, k, C.c_void_p(t.data_ptr()))
        d.queue = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
        return d

    L = _lib.lib()
    res = torch.empty(tuple(reversed(oshape)), dtype=torch.float32, device=dev).permute(*reversed(range(kind + 1)))
    d_full, d_one = desc(), desc(1, 1)

    def entry():
        _lib.check(L.qdas_scanconvert(C.byref(d_full), C.c_void_p(b.data_ptr()), C.c_void_p(res.data_ptr())))
        return res

    def launch_only():
        _lib.check(L.qdas_scanconvert(C.byref(d_one), C.c_void_p(b.data_ptr()), C.c_void_p(res.data_ptr())))
        return res

    def wrapper():
        if kind == 2:
            return SC.scan_convert(b, deg["r"], deg["a"], og, deg["x"], deg["z"], pre="db", db_floor=DB_FLOOR, check_grid=False)[0]
        return SC.scan_convert3(b, deg["r"], deg["a"], deg["e"], og, deg["x"], deg["y"], deg["z"], pre="db", db_floor=DB_FLOOR, check_grid=False)[0]

    def cell(gv, p):
        inside = (p >= gv[0]) & (p <= gv[-1])
        k = (torch.searchsorted(gv, p.contiguous(), right=True) - 1).clamp_(0, gv.numel() - 2)
        return inside, k, ((p - gv[k]) / (gv[k + 1] - gv[k])).to(torch.float32)

    def composed():
        dz, dx = (rad["z"] - og[2])[:, None], (rad["x"] - og[0])[None, :]
        if kind == 3:
            dz, dx, dy = dz[:, :, None], dx[:, :, None], (rad["y"] - og[1])[None, None, :]
            rho, alpha, eps = torch.sqrt(dx * dx + dy * dy + dz * dz), torch.atan2(dx, dz).expand(oshape[:3]), torch.atan2(dy, torch.hypot(dz, dx))
            (ir, k, u), (ia, l, v), (ie, m, w) = cell(rad["r"], rho), cell(rad["a"], alpha), cell(rad["e"], eps)
            inside = ir & ia & ie
        else:
            rho, alpha = torch.hypot(dz, dx), torch.atan2(dx, dz)
            (ir, k, u), (ia, l, v) = cell(rad["r"], rho), cell(rad["a"], alpha)
            inside = ir & ia
        pages = []
        for p in range(P):
            img = 20 * torch.log10(b[..., p].abs())
            img = torch.where(img < DB_FLOOR, torch.full_like(img, DB_FLOOR), img)
            if kind == 3:
                sheets = []
                for mm in (m, m + 1):
                    lo = torch.lerp(img[k, l, mm], img[k + 1, l, mm], u)
                    hi = torch.lerp(img[k, l + 1, mm], img[k + 1, l + 1, mm], u)
                    sheets.append(torch.lerp(lo, hi, v))
                o = torch.lerp(sheets[0], sheets[1], w)
            else:
                o = torch.lerp(torch.lerp(img[k, l], img[k + 1, l], u), torch.lerp(img[k, l + 1], img[k + 1, l + 1], u), v)
            pages.append(torch.where(inside, o, torch.full_like(o, math.nan)))
        return torch.stack(pages, dim=-1)

    fns = [entry, wrapper, composed] + ([launch_only] if name == "c5-1" else [])
    st, outs = timed(torch, fns, reps, inner)
    ye, yw, yc = outs[0].clone(), outs[1], outs[2]
    mask_same = bool(torch.equal(torch.isnan(ye), torch.isnan(yc)))
    fin = ~torch.isnan(yc)
    par = float((ye[fin] - yc[fin]).abs().max() / yc[fin].abs().max()) if mask_same else float("nan")
    same_w = bool(torch.equal(torch.nan_to_num(ye, nan=12345.0), torch.nan_to_num(yw, nan=12345.0)))
    nb_src, nb_out = b.numel() * 8, res.numel() * 4
    by = nb_src + nb_out
    rate = lambda ms: by / (ms * 1e-3) / 1e12
    (ms_e, lo_e, hi_e), (ms_w, lo_w, hi_w), (ms_c, lo_c, hi_c) = st[:3]
    line = (f"{name:8s} source {' x '.join(str(s) for s in shape)} complex64 x {P} page(s) -> {' x '.join(str(s) for s in oshape[:-1])} float32 (pre = dB, floor {DB_FLOOR:g}), "
            f"{100 * float(fin.float().mean()):.0f} % inside: C entry {ms_e:8.4f} ms [{lo_e:.4f} .. {hi_e:.4f}]  wrapper {ms_w:8.4f} ms [{lo_w:.4f} .. {hi_w:.4f}]  "
            f"composition {ms_c:9.4f} ms [{lo_c:.4f} .. {hi_c:.4f}]  composition / entry {ms_c / ms_e:6.1f} x  "
            f"bytes {by / 1e6:8.2f} MB (source {nb_src / 1e6:.2f} read once + output {nb_out / 1e6:.2f} written once): entry {1e3 * rate(ms_e):8.1f} GB/s = "
            f"{100 * rate(ms_e) / HBM_TBS:5.2f} % of the HBM roof  masks identical: {mask_same}  wrapper == entry: {same_w}  "
            f"parity max|entry - composition| / max|composition| inside {par:.2e}")
    if name == "c5-1":
        ms_l, lo_l, hi_l = st[3]
        line += f"  the same call onto a 1 x 1 grid (the launch itself) {ms_l:.4f} ms [{lo_l:.4f} .. {hi_l:.4f}] = {100 * ms_l / ms_e:.0f} % of the entry's time"
    print(line)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--small", action="store_true", help="an eighth of the axes (a quick check of the tool)")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--inner", type=int, default=20, help="calls per timed window")
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.small, a.reps, a.inner)
    print(f"# scanconvert_time: complex64 source, pre = dB; device events around windows of {a.inner} back-to-back calls, the paths interleaved, median per call of "
          f"{a.reps} windows [smallest .. largest] after 3 warm-ups; each workload in a process of its own (limit {CHILD_LIMIT_S} s); HBM roof {HBM_TBS} TB/s", flush=True)
    for name in WORKLOADS:
        cmd = ["timeout", "-k", "10", str(CHILD_LIMIT_S), sys.executable, os.path.abspath(__file__), "--child", name, "--reps", str(a.reps), "--inner", str(a.inner)]
        r = subprocess.run(cmd + (["--small"] if a.small else []), capture_output=True, text=True)
        sys.stdout.write(r.stdout)
        sys.stdout.flush()
        if r.returncode < 0 or r.returncode in FAULT_STATUS or "illegal memory access" in r.stderr:
            sys.exit(f"scanconvert_time: the child for {name} ended with status {r.returncode} (signal, abort or time limit): nothing more is run on this device.\n{r.stderr[-600:]}")
        if r.returncode:
            sys.exit(f"scanconvert_time: the child for {name} failed with status {r.returncode}:\n{r.stderr[-1200:]}")


if __name__ == "__main__":
    main()
