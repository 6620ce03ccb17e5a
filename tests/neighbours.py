"""Loud-neighbour and isolation checks for batched entries (a helper module, not a conftest; the style of tests/guards.py).

One launch of a batched entry works on many independent MEMBERS (traces, channels, slices, pages, frames, maps).  Three properties that a parity test on
i.i.d. data of one amplitude, normalised by the tensor's maximum, cannot see -- each checked from the host with plain torch:

A. ``check_scale``: exact scale equivariance.  Every entry checked here is linear in its data (or bilinear in data x per-member filter), and a power of two
   commutes with every rounding of ``+ - * fma`` (absent overflow and subnormals).  So the entry runs on ``x`` and on ``x`` with unit ``u`` multiplied by
   ``2^e[u mod 4]``; each output unit of the second run must equal the first run's times ``2^e``, bit for bit.  A sample leaked from a neighbour carries the
   neighbour's exponent and breaks this at any size of leak.  Per-member second operands take the reversed table; the output carries the sum of the exponents.
   (``degree=2``: a member correlated with itself carries twice its exponent.)  The factors are made from their bits (``pow2``), not by ``torch.ldexp``.
B. ``check_parity``: the error of each output unit against a float64 restatement, over THAT UNIT's ``max|ref|``.
C. ``check_poison``: even units, then odd units, are set to NaN (all of the unit) or receive a single +Inf at a position drawn per unit; every unpoisoned output
   unit must keep the bits of the clean run.

A ``Spec`` names, for every input and output, the axes that enumerate members: ``None`` for an input all members share; else one axis per MEMBER DIMENSION (a
tuple; an int stands for one dimension; ``None`` inside a tuple for a dimension the tensor does not have, a filter per column but not per slice).  The member
index of a tensor is the row-major index over the member dimensions it has; ``group`` consecutive members form a UNIT (the one-pass hilbert packs two traces
into one transform: ``group=2``).  With ``guard=(monkeypatch, cpu)`` every ``torch.empty`` of the entry starts as the 0xFF sentinel of tests/guards.py, and an
output scalar that still holds it is reported as never written.

Limits: integers have neither NaN nor Inf -- their largest value stands in; half-precision storage is excluded from A by its callers (subnormal half outputs
are not scale-exact)."""
from __future__ import annotations

import collections
import contextlib

import numpy as np
import torch

from tests import guards as GD

EXP = {torch.float32: (0, 20, -20, 7), torch.complex64: (0, 20, -20, 7),
       torch.float64: (0, 40, -40, 7), torch.complex128: (0, 40, -40, 7),
       torch.int16: (0, 4, 2, 1),                                       # multipliers 1, 16, 4, 2 on |x| <= 2000
       torch.float16: (0, 4, -4, 2), torch.complex32: (0, 4, -4, 2)}    # (B only) N(0, 1/16) data and O(1/4) taps stay inside half's normal range [6e-5, 65504]

SUMMARY = collections.OrderedDict()          # entry -> {"A" | "B" | "C": [cases, members checked]}


class NeighbourError(AssertionError):
    pass


def _count(entry, check, members):
    if entry is not None:
        s = SUMMARY.setdefault(entry, {}).setdefault(check, [0, 0])
        s[0] += 1
        s[1] += int(members)


def _tup(r):
    return tuple(r) if isinstance(r, (tuple, list)) else (r,)


def _real(t):
    """the tensor as real scalars: a complex one gains a trailing axis of 2"""
    return torch.view_as_real(t) if t.is_complex() else t


def bits(t):
    """the bit pattern of every real scalar as integers, in the tensor's shape (NaN compares equal to itself)"""
    r = _real(t).contiguous()
    return r.view(GD._INT[r.element_size()])


def pow2(e, dtype):
    """2^e in a real dtype, made from its bits: ``torch.ldexp`` multiplies by ``pow(2.0, e)``, and a device's ``pow`` owes nobody the last bit"""
    mant, bias, it = {torch.float16: (10, 15, torch.int16), torch.float32: (23, 127, torch.int32), torch.float64: (52, 1023, torch.int64)}[dtype]
    assert bool(((e + bias > 0) & (e + bias < 2 * bias + 1)).all()), "a normal number"
    return ((e.to(torch.int64) + bias) << mant).to(it).view(dtype)


def ldexp(r, e):
    """``r * 2^e`` for a real tensor: exact while nothing overflows or turns subnormal"""
    return r * pow2(e, r.dtype)


class Spec:
    def __init__(self, in_axes, out_axes, group=1, guard=None, seed=0, degree=1):
        self.in_axes = [self._norm(a) for a in in_axes]
        outs = out_axes if isinstance(out_axes, list) else [out_axes]
        self.out_axes = [self._norm(a) for a in outs]
        self.D = max(len(a) for a in self.in_axes + self.out_axes if a is not None)
        assert all(a is None or len(a) == self.D for a in self.in_axes + self.out_axes), "one axis (or None) per member dimension"
        assert all(a is not None for a in self.out_axes), "every output enumerates members"
        self.group, self.guard, self.seed, self.degree = int(group), guard, seed, int(degree)
        assert self.group == 1 or all(a is None or None not in a for a in self.in_axes + self.out_axes), "a group needs every member dimension"

    @staticmethod
    def _norm(a):
        return None if a is None else ((a,) if isinstance(a, int) else tuple(a))

    # -- geometry
    def sizes(self, t, axes):
        """the tensor's size along each member dimension (1 where it has none)"""
        return [1 if a is None else int(t.shape[a]) for a in axes]

    def units(self, sizes, device):
        """unit index of every member, as a grid over the member dimensions"""
        n = int(np.prod(sizes))
        return (torch.arange(n, device=device) // self.group).reshape(sizes)

    @staticmethod
    def layout(grid, axes, ndim):
        """a grid over the member dimensions, shaped to broadcast against a tensor of ``ndim`` axes whose member axes are ``axes``"""
        present = [d for d, a in enumerate(axes) if a is not None]
        assert all(grid.shape[d] == 1 for d in range(grid.ndim) if d not in present), "the tensor lacks a member dimension the grid varies along"
        g = grid.reshape([grid.shape[d] for d in present])
        order = sorted(range(len(present)), key=lambda k: axes[present[k]] % ndim)
        shape = [1] * ndim
        for k in order:
            shape[axes[present[k]] % ndim] = g.shape[k]
        return g.permute(order).reshape(shape)

    def rows(self, t, axes):
        """real scalars as [members, rest] (a copy), and the inverse that puts such a matrix back into the tensor's shape and dtype"""
        r = _real(t)
        nd = t.ndim
        ax = [a % nd for a in axes if a is not None]
        perm = ax + [k for k in range(r.ndim) if k not in ax]
        p = r.permute(perm)
        m = p.reshape(int(np.prod([r.shape[a] for a in ax])) if ax else 1, -1).clone()

        def back(mm):
            q = mm.reshape(p.shape).permute([perm.index(k) for k in range(r.ndim)]).contiguous()
            return torch.view_as_complex(q) if t.is_complex() else q
        return m, back

    def unit_amax(self, t, axes):
        """max |.| over each unit of a tensor (complex: the modulus)"""
        a = t.abs()
        nd = a.ndim
        ax = [x % nd for x in axes if x is not None]
        p = a.permute(ax + [k for k in range(nd) if k not in ax])
        m = p.reshape(int(np.prod([a.shape[x] for x in ax])) if ax else 1, -1).amax(1)
        pad = (-m.numel()) % self.group
        if pad:
            m = torch.cat([m, m.new_zeros(pad)])
        return m.reshape(-1, self.group).amax(1)

    # -- running
    def run(self, fn, inputs):
        ctx = GD.guard_outputs(self.guard[0], cpu=self.guard[1]) if self.guard else contextlib.nullcontext()
        with ctx:
            outs = _tup(fn(*inputs))
        if outs[0].is_cuda:
            torch.cuda.synchronize()
        assert len(outs) == len(self.out_axes), "one member-axis entry per output"
        for k, o in enumerate(outs):
            if o.dtype.is_floating_point or o.is_complex():
                n = int((bits(o) == -1).sum())
                if n:
                    raise NeighbourError(f"output {k}: {n} real scalar(s) never written")
        return outs

    def alive(self, outs, what=""):
        """every unit of a clean run's outputs holds a finite non-zero scalar: an all-NaN or all-zero unit would pass A and C whatever the kernel did"""
        for k, (o, axes) in enumerate(zip(outs, self.out_axes)):
            r = _real(o)
            v = torch.where(torch.isfinite(r), r, torch.zeros_like(r)).abs()
            v = v.amax(-1) if o.is_complex() else v
            dead = self.unit_amax(v, axes) == 0
            if bool(dead.any()):
                raise NeighbourError(f"{what}: output {k}: unit {int(dead.nonzero()[0])} of the clean run holds no finite non-zero value")
        return outs

    def _member_inputs(self, inputs):
        assert len(inputs) == len(self.in_axes)
        return [k for k, a in enumerate(self.in_axes) if a is not None]

    def exponents(self, inputs):
        """per member input: the exponent grid over the member dimensions (first member input: the table; later ones: the table reversed)"""
        out = {}
        for j, k in enumerate(self._member_inputs(inputs)):
            t = inputs[k]
            tab = EXP[t.dtype] if j == 0 else tuple(reversed(EXP[t.dtype]))
            u = self.units(self.sizes(t, self.in_axes[k]), t.device)
            out[k] = torch.tensor(tab, device=t.device)[u % 4]
        return out

    def scaled(self, inputs):
        """(the inputs with every unit multiplied by its power of two, the exponent grid of the outputs)"""
        ex = self.exponents(inputs)
        res, total = list(inputs), 0
        for k, e in ex.items():
            t = inputs[k]
            el = self.layout(e, self.in_axes[k], t.ndim)
            if t.dtype.is_floating_point or t.is_complex():
                r = ldexp(_real(t), el.unsqueeze(-1) if t.is_complex() else el)
                res[k] = torch.view_as_complex(r.contiguous()) if t.is_complex() else r
                if t.dtype in (torch.float16, torch.complex32):
                    assert bool(torch.isfinite(r).all())
            else:
                res[k] = t * (torch.ones_like(el) << el).to(t.dtype)
                assert bool((res[k].to(torch.int64) == t.to(torch.int64) * (1 << el.to(torch.int64))).all()), "integer overflow"
            total = total + e * self.degree                                # (degree 2: a member correlated with itself)
        return res, total

    # -- A
    def check_scale(self, fn, inputs, entry=None, what="", same=False):
        """A.  ``same``: the output is homogeneous of degree 0 in each member (a normalised correlation) and must not change at all."""
        clean = self.alive(self.run(fn, inputs), what)
        xs, e = self.scaled(inputs)
        got = self.run(fn, xs)
        members = 0
        for k, (a, b, axes) in enumerate(zip(clean, got, self.out_axes)):
            if a.shape != b.shape or a.dtype != b.dtype:
                raise NeighbourError(f"{what}: output {k} changed shape or type under scaling")
            el = self.layout(e if not same else torch.zeros_like(e), axes, a.ndim)
            ra, rb = _real(a), _real(b)
            want = ldexp(ra, el.unsqueeze(-1) if a.is_complex() else el)
            want = torch.where(torch.isnan(ra), ra, want)                     # (a NaN keeps its bits: pixels outside a mask)
            bad = bits(want) != bits(rb)
            bad = bad.any(-1) if a.is_complex() else bad
            if bool(bad.any()):
                first = tuple(int(v) for v in bad.nonzero()[0])
                raise NeighbourError(f"{what}: output {k} is not the clean output times its unit's power of two: {int(bad.sum())} element(s), first at {first} "
                                     f"(got {b[first].item()!r}, want {ra[first].tolist()!r} x 2^{int(el.expand(a.shape)[first])})")
            members += int(np.prod(self.sizes(a, axes)))
        _count(entry, "A", members)
        return clean, got

    # -- B
    def check_parity(self, outs, refs, bound, entry=None, what=""):
        """B.  ``refs``: float64 (complex128) arrays or tensors in the outputs' shapes.  Returns the largest per-unit error over the unit's own ``max|ref|``."""
        worst, members = 0.0, 0
        for k, (o, r, axes) in enumerate(zip(_tup(outs), _tup(refs), self.out_axes)):
            r = torch.as_tensor(np.ascontiguousarray(r) if isinstance(r, np.ndarray) else r)
            o = o.detach().cpu()
            o = torch.view_as_complex(torch.view_as_real(o).double()) if o.is_complex() else o.double()
            if tuple(o.shape) != tuple(r.shape):
                raise NeighbourError(f"{what}: output {k} has shape {tuple(o.shape)}, the reference {tuple(r.shape)}")
            err, den = self.unit_amax(o - r, axes), self.unit_amax(r, axes)
            if bool((err[den == 0] != 0).any()):
                raise NeighbourError(f"{what}: output {k}: a unit whose reference is zero is not zero")
            ratio = torch.where(den > 0, err / den.clamp_min(1e-300), torch.zeros_like(err))
            ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
            if bool((ratio > bound).any()):
                u = int(ratio.argmax())
                raise NeighbourError(f"{what}: output {k} unit {u}: error {float(err[u]):.3e} over the unit's max|ref| {float(den[u]):.3e} = {float(ratio[u]):.3e} > {bound:g}")
            worst = max(worst, float(ratio.max()))
            members += int(np.prod(self.sizes(o, axes)))
        _count(entry, "B", members)
        return worst

    # -- C
    def poisoned(self, inputs, parity, fill):
        """(the inputs with the units of that parity poisoned, the bool grid of the poisoned output members)"""
        rng = np.random.default_rng([self.seed, parity, fill == "nan"])
        res, hit = list(inputs), False
        for k in self._member_inputs(inputs):
            t = inputs[k]
            sizes = self.sizes(t, self.in_axes[k])
            sel = self.units(sizes, t.device) % 2 == parity
            hit = sel | hit
            m, back = self.rows(t, self.in_axes[k])
            isint = not (t.dtype.is_floating_point or t.is_complex())
            if fill == "nan":
                m[sel.reshape(-1)] = torch.iinfo(t.dtype).max if isint else float("nan")
            else:
                rest, n = m.shape[1], m.shape[0]
                for u in range(parity, -(-n // self.group), 2):
                    lo, hi = u * self.group, min((u + 1) * self.group, n)
                    r = int(rng.integers(0, (hi - lo) * rest))
                    m[lo + r // rest, r % rest] = torch.iinfo(t.dtype).max if isint else float("inf")
            res[k] = back(m)
        return res, hit

    def check_poison(self, fn, inputs, entry=None, what="", clean=None):
        """C.  Returns the runs as ``[(parity, fill, poisoned inputs, outputs, poisoned-member grid)]`` for checks of the caller's own."""
        clean = self.alive(self.run(fn, inputs), what) if clean is None else clean
        runs, members = [], 0
        for parity in (0, 1):
            for fill in ("nan", "inf"):
                xs, hit = self.poisoned(inputs, parity, fill)
                got = self.run(fn, xs)
                for k, (a, b, axes) in enumerate(zip(clean, got, self.out_axes)):
                    if a.shape != b.shape or a.dtype != b.dtype:
                        raise NeighbourError(f"{what}: output {k} changed shape or type under poison")
                    keep = ~self.layout(hit, axes, a.ndim)
                    bad = bits(a) != bits(b)
                    bad = (bad.any(-1) if a.is_complex() else bad) & keep
                    if bool(bad.any()):
                        first = tuple(int(v) for v in bad.nonzero()[0])
                        raise NeighbourError(f"{what}: output {k}: {int(bad.sum())} element(s) of unpoisoned units changed ({fill} in the "
                                             f"{'even' if parity == 0 else 'odd'} units), first at {first}: {a[first].item()!r} -> {b[first].item()!r}")
                    members += int(keep.sum())
                runs.append((parity, fill, xs, got, hit))
        _count(entry, "C", members)
        return runs
