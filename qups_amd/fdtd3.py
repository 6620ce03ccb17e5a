"""A 3-D acoustic FDTD channel-data simulator on the device: ``csrc/fdtd3.hip`` behind :func:`fdtd3` (arrays) and ``UltrasoundSystem.fdtdSim`` on a volume
(objects).  The 3-D twin of ``qups_amd/fdtd.py``, whose time step, transmit table, PML factors and size rule, iso-impedance medium and cubic sampling it uses
as they are.

The scheme is that of the 2-D solver with a third axis: linear, lossless, first order on a staggered grid, of order ``2R`` in space (``include/qdas.h`` states
it in full; ``tests/fdtd3_ref.py`` is its numpy restatement).  Maps are ``Z x X x Y``; in memory ``z`` is fastest, then ``x``, then ``y`` -- the order of a
``Scan.cartesian(x, z, y)`` grid.  Everything the kernel reads is prepared here on the host in float64 (the extended medium, the three staggered densities,
the six PML vectors, the source table, the per-brick point lists) and uploaded once; the states, the record and every table are torch tensors, so the C entry
allocates nothing.  There is no CPU fallback: without the library or a device the call raises."""
from __future__ import annotations

import ctypes as C
import math

import numpy as np

from . import _lib
from .das_spec import DasError
from .fdtd import COEFS, _order, _sample_cubic, iso_density, pml_factors, pml_size, time_step, tx_table  # noqa: F401  (one recipe for both solvers)

__all__ = ["fdtd3", "launch", "prepare", "stability_limit", "grid_spacing3", "nearest_nodes3", "brick_lists", "BRICK", "STATES"]

BRICK = (_lib.FDTD3_TZ, _lib.FDTD3_TX, _lib.FDTD3_TY)
STATES = ("p", "uz", "ux", "uy", "rz", "rx", "ry")


def stability_limit(R: int) -> float:
    """``c_max dt / h <= 1 / (sqrt(3) sum|a_k|)``: 0.5774, 0.4949 and 0.4488 for R = 1, 2, 4"""
    return 1.0 / (math.sqrt(3.0) * sum(abs(a) for a in COEFS[int(R)]))


def _check_step(c_max, dt, h, R):
    if c_max * dt / h > stability_limit(R):
        raise DasError(f"fdtd3: c_max dt / h = {c_max * dt / h:.4f} is above the stability limit {stability_limit(R):.4f} of order {2 * R} in 3-D")


def grid_spacing3(z, x, y):
    """``h`` of a uniform cubic grid; unequal or non-uniform spacing (beyond 1e-6 relative) in any of the three axes is refused"""
    ax = [np.asarray(a, np.float64).reshape(-1) for a in (z, x, y)]
    if any(a.size < 2 for a in ax):
        raise DasError("fdtd3: the grid needs at least two nodes in z, in x and in y")
    d = [np.diff(a) for a in ax]
    h = float(d[0].mean())
    if not h > 0 or any(np.abs(v - h).max() > 1e-6 * h for v in d):
        raise DasError(f"fdtd3: the grid spacing must be uniform and equal in z, x and y (dz = {h:g}, dx = {float(d[1].mean()):g}, dy = {float(d[2].mean()):g})")
    return h


def nearest_nodes3(z, x, y, pos):
    """``(iz, ix, iy)`` of the nearest node per position; ``pos`` is ``3 x M`` with rows ``(x, y, z)``, as ``Transducer.positions()`` gives them.  The
    reference's assertion applies when two positions share a node (``:2753-2768``)."""
    z, x, y = (np.asarray(a, np.float64).reshape(-1) for a in (z, x, y))
    pos = np.asarray(pos, np.float64).reshape(3, -1)
    iz = np.abs(pos[2][:, None] - z[None]).argmin(1)
    ix = np.abs(pos[0][:, None] - x[None]).argmin(1)
    iy = np.abs(pos[1][:, None] - y[None]).argmin(1)
    if len(set(zip(iz.tolist(), ix.tolist(), iy.tolist()))) != iz.size:
        raise DasError("Elements are not unique; the Scan spacing or sizing may be too small.")
    return iz.astype(np.int64), ix.astype(np.int64), iy.astype(np.int64)


def brick_lists(Nz, Nx, Ny, nodes):
    """``(start, list)`` int32: the per-brick lists of the points at ``nodes`` (``(k Nx + j) Nz + i``), from the library's host helper"""
    L = _lib.lib()
    nodes = np.ascontiguousarray(nodes, np.int32)
    nb = int(L.qdas_fdtd3_bricks(Nz, Nx, Ny))
    start, lst = np.zeros(nb + 1, np.int32), np.zeros(max(nodes.size, 1), np.int32)
    _lib.check(L.qdas_fdtd3_brick_lists(Nz, Nx, Ny, nodes.size, nodes.ctypes.data if nodes.size else None, start.ctypes.data, lst.ctypes.data))
    return start, lst[:nodes.size]


def prepare(c, rho, h, dt, P):
    """the kernel's host tables in float64 from the interior medium ``c``, ``rho`` (``Z x X x Y``): a dict with ``Nz, Nx, Ny, c, c2, rho, dtrz, dtrx, dtry``
    (``Ny x Nx x Nz``, z fastest: extended by edge replication, the staggered density of an axis the mean of the two neighbours with the last one kept)
    and ``az, azs, ax, axs, ay, ays``"""
    c, rho = np.asarray(c, np.float64), np.asarray(rho, np.float64)
    if c.ndim != 3 or rho.shape != c.shape:
        raise DasError(f"fdtd3: c and rho are Z x X x Y maps of one shape, got {c.shape} and {rho.shape}")
    if not (np.isfinite(c).all() and np.isfinite(rho).all() and (c > 0).all() and (rho > 0).all()):
        raise DasError("fdtd3: c and rho must be finite and positive")
    ce, re = np.pad(c, P, mode="edge"), np.pad(rho, P, mode="edge")
    sgz, sgx, sgy = re.copy(), re.copy(), re.copy()
    sgz[:-1] = 0.5 * (re[:-1] + re[1:])
    sgx[:, :-1] = 0.5 * (re[:, :-1] + re[:, 1:])
    sgy[:, :, :-1] = 0.5 * (re[:, :, :-1] + re[:, :, 1:])
    Nz, Nx, Ny = ce.shape
    c_max = float(c.max())
    az, azs = pml_factors(Nz, P, c_max, h, dt)
    ax, axs = pml_factors(Nx, P, c_max, h, dt)
    ay, ays = pml_factors(Ny, P, c_max, h, dt)
    T = lambda a: np.ascontiguousarray(a.transpose(2, 1, 0))
    return dict(Nz=Nz, Nx=Nx, Ny=Ny, c=T(ce), c2=T(ce * ce), rho=T(re), dtrz=T(dt / sgz), dtrx=T(dt / sgx), dtry=T(dt / sgy), az=az, azs=azs, ax=ax, axs=axs,
                ay=ay, ays=ays)


def _host(a):
    return np.asarray(a.detach().cpu().numpy() if hasattr(a, "detach") else a, np.float64)


def fdtd3(c, rho, z, x, y, src_pos, src_normal, s, sen_pos, Nt, dt, PML=20, order=8, prec="single", bsize=None, device=None, return_state=False, ld=None,
          pstride=None, prepare_only=False, sen_nodes=None):
    """``rec = fdtd3(c, rho, z, x, y, src_pos, src_normal, s, sen_pos, Nt, dt)``: ``Nt`` steps of the scheme on the grid ``z`` x ``x`` x ``y`` (``c``, ``rho``:
    ``Z x X x Y``) with ``PML`` cells added on all six faces.  ``src_pos`` / ``sen_pos``: positions ``3 x M`` rows ``(x, y, z)`` mapped to their nearest nodes;
    ``src_normal``: ``3 x M`` rows ``(nz, nx, ny)``; ``s``: the source table ``T' x M x V`` (host array or tensor).  Returns the record ``Nt x N x V`` (a device
    tensor of ``prec``), and with ``return_state`` also a dict of the seven state arrays ``V x Ny x Nx x Nz`` after the last step.  ``sen_nodes``: the sensors'
    interior nodes ``(iz, ix, iy)`` given directly, in place of ``sen_pos`` (``field``: every node).  ``bsize``: pulses per call, to bound the memory of the
    states: without ``return_state`` ONE set of seven ``bsize x Ny x Nx x ld`` state arrays serves every block (seven states of a 168^3 grid are 133 MB per
    pulse in float32).  ``ld`` / ``pstride``: the row and the plane stride of the state arrays (defaults ``Nz`` and ``Nx ld``).  ``prepare_only``: ``(meta,
    tables, s)`` on the device for :func:`launch`, nothing run.  Queued on torch's current stream."""
    import torch
    if prec not in ("single", "double"):
        raise DasError("fdtd3: prec must be 'single' or 'double'")
    R = _order(order)
    h = grid_spacing3(z, x, y)
    zc, xc, yc = (np.asarray(a, np.float64).reshape(-1) for a in (z, x, y))
    c, rho = _host(c), _host(rho)
    if c.shape != (zc.size, xc.size, yc.size):
        raise DasError(f"fdtd3: c is Z x X x Y = {zc.size} x {xc.size} x {yc.size}, got {c.shape}")
    P = pml_size(PML, zc.size, xc.size, yc.size)
    dt = float(dt)
    if not (dt > 0 and math.isfinite(dt)):
        raise DasError("fdtd3: dt must be positive")
    _check_step(c.max(), dt, h, R)
    tab = prepare(c, rho, h, dt, P)
    Nz, Nx, Ny = tab["Nz"], tab["Nx"], tab["Ny"]
    if Nz * Nx * Ny >= 2 ** 31:
        raise DasError(f"fdtd3: {Nz} x {Nx} x {Ny} nodes reach 2^31")
    s_host = None if isinstance(s, torch.Tensor) else np.asarray(s, np.float64)
    if (s.ndim if s_host is None else s_host.ndim) != 3:
        raise DasError("fdtd3: the source table is T' x M x V")
    Ts, M, V = (int(v) for v in (s.shape if s_host is None else s_host.shape))
    none = (np.zeros(0, np.int64),) * 3
    si = nearest_nodes3(zc, xc, yc, src_pos) if M else none
    if sen_nodes is not None:
        ni = tuple(np.asarray(a, np.int64).reshape(-1) for a in sen_nodes)
        if len(ni) != 3 or len({a.size for a in ni}) != 1 or (ni[0].size and any(a.min() < 0 or a.max() >= n for a, n in zip(ni, c.shape))):
            raise DasError("fdtd3: sen_nodes are (iz, ix, iy) inside the grid")
    else:
        ni = nearest_nodes3(zc, xc, yc, sen_pos) if np.size(sen_pos) else none
    nrm = np.asarray(src_normal, np.float64).reshape(3, -1)
    if si[0].size != M or nrm.shape[1] != M:
        raise DasError(f"fdtd3: {si[0].size} source positions and {nrm.shape[1]} normals for a table of M = {M} sources")
    N, Nt = int(ni[0].size), int(Nt)
    if Nt < 0:
        raise DasError("fdtd3: Nt must not be negative")
    node = lambda q: (((q[2] + P) * Nx + (q[1] + P)) * Nz + (q[0] + P)).astype(np.int32)
    src_node, sen_node = node(si), node(ni)
    csrc = tab["c"].reshape(-1)[src_node] if M else np.zeros(0)
    w = [nrm[a] * 2.0 * csrc * dt / h for a in range(3)]

    if device is None:
        device = s.device if s_host is None and s.is_cuda else torch.device("cuda", torch.cuda.current_device())
    dev = torch.device(device)
    if dev.type != "cuda":
        raise DasError("fdtd3: needs a device (there is no CPU fallback in this package)")
    rdt = torch.float32 if prec == "single" else torch.float64
    up = lambda a, dt_=None: torch.from_numpy(np.ascontiguousarray(a)).to(device=dev, dtype=dt_ or rdt)
    src_start, src_list = brick_lists(Nz, Nx, Ny, src_node)
    sen_start, sen_list = brick_lists(Nz, Nx, Ny, sen_node)
    tb = {k: up(tab[k]) for k in ("c2", "rho", "dtrz", "dtrx", "dtry", "az", "azs", "ax", "axs", "ay", "ays")}
    tb.update(src_wz=up(w[0]), src_wx=up(w[1]), src_wy=up(w[2]))
    tb.update({k: up(v, torch.int32) for k, v in (("src_node", src_node), ("src_start", src_start), ("src_list", src_list), ("sen_node", sen_node),
                                                  ("sen_start", sen_start), ("sen_list", sen_list))})
    s_dev = (s if s_host is None else up(s_host)).to(device=dev, dtype=rdt)
    ld = Nz if ld is None else int(ld)
    if ld < Nz:
        raise DasError(f"fdtd3: ld = {ld} is less than Nz = {Nz}")
    ps = Nx * ld if pstride is None else int(pstride)
    if ps < Nx * ld:
        raise DasError(f"fdtd3: pstride = {ps} is less than Nx ld = {Nx * ld}")
    meta = dict(Nz=Nz, Nx=Nx, Ny=Ny, Nt=Nt, ld=ld, pstride=ps, M=M, Ts=Ts, N=N, dt_h=dt / h, inv_h=1.0 / h, double=prec == "double", order=2 * R)
    if prepare_only:
        return meta, tb, s_dev
    rec = torch.empty((Nt, N, V), dtype=rdt, device=dev)
    bs = V if not bsize else max(1, min(int(bsize), V))
    states = {k: [] for k in STATES}
    pool = None                                                  # the one set of state arrays every block works in, unless the states are wanted
    with torch.cuda.device(dev):
        for v0 in range(0, V, bs) if V else ():
            Vb = min(bs, V - v0)
            if return_state or pool is None:
                pool = {k: torch.empty_strided((Vb, Ny, Nx, ld), (Ny * ps, ps, ld, 1), dtype=rdt, device=dev) for k in STATES}
            st = {k: pool[k][:Vb] for k in STATES}
            for k in STATES:
                st[k].zero_()
            launch(meta, tb, st, s_dev[:, :, v0:v0 + Vb].contiguous(), rec, v0)
            if return_state:
                for k in STATES:
                    states[k].append(st[k][..., :Nz])
    if not return_state:
        return rec
    cat = lambda parts: parts[0] if len(parts) == 1 else torch.cat(parts, 0)
    empty = torch.zeros((0, Ny, Nx, Nz), dtype=rdt, device=dev)
    return rec, {k: (cat(v) if v else empty) for k, v in states.items()}


def launch(meta, tb, st, sb, rec, v0=0, stream=None):
    """one call of ``qdas_fdtd3``: ``meta`` the sizes and scalars, ``tb`` the device tables by the names of ``qdas_fdtd3_args``, ``st`` the seven state tensors
    ``Vb x Ny x Nx x ld`` with the strides ``(Ny pstride, pstride, ld, 1)`` (zero for a start from rest), ``sb`` the source table ``T' x M x Vb`` (contiguous),
    ``rec`` the whole record ``Nt x N x V`` of which the pulses ``v0 .. v0 + Vb - 1`` are written.  ``stream``: a ``torch.cuda.Stream`` (default: the current
    one).  Only enqueues."""
    import torch
    dev = st["p"].device
    Vb = int(st["p"].shape[0])
    d = _lib.Fdtd3Desc()
    d.Nz, d.Nx, d.Ny, d.V, d.Nt = meta["Nz"], meta["Nx"], meta["Ny"], Vb, meta["Nt"]
    d.ld, d.pstride, d.vstride = meta["ld"], meta["pstride"], meta["Ny"] * meta["pstride"]
    for k in STATES:
        want = (d.vstride, d.pstride, d.ld, 1)
        if tuple(st[k].shape) != (Vb, meta["Ny"], meta["Nx"], meta["ld"]) or any(n > 1 and a != b for n, a, b in zip(st[k].shape, st[k].stride(), want)):
            raise DasError(f"fdtd3: state {k} is {tuple(st[k].shape)} with strides {tuple(st[k].stride())}, not Vb x Ny x Nx x ld with (Ny pstride, pstride, ld, 1)")
    d.M, d.Ts, d.N = meta["M"], meta["Ts"], meta["N"]
    d.rec_st, d.rec_sn, d.rec_sv = (int(v) for v in rec.stride())
    d.dt_h, d.inv_h = meta["dt_h"], meta["inv_h"]
    d.dtype, d.order = (0 if meta["double"] else 1), meta["order"]                  # QDAS_F64 | QDAS_F32
    d.device = dev.index if dev.index is not None else torch.cuda.current_device()
    d.flags = int(meta.get("flags", 0))                                           # _lib.FDTD3_ZERO: the entry clears the states itself
    stream = stream or torch.cuda.current_stream(dev)
    d.queue = C.c_void_p(stream.cuda_stream)
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t is not None and t.numel() else None
    a = _lib.Fdtd3Args()
    for k in STATES:
        setattr(a, k, ptr(st[k]))
    for k, t in tb.items():
        setattr(a, k, ptr(t))
    a.s = ptr(sb)
    a.rec = C.c_void_p(rec.data_ptr() + v0 * rec.stride(2) * rec.element_size()) if rec.numel() else None
    _lib.check(_lib.lib().qdas_fdtd3(C.byref(d), C.byref(a)))
    if sb.numel():
        sb.record_stream(stream)
