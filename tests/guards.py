"""Host-checked memory guards for the device wrappers (a helper module, not a conftest).

Three properties a parity test cannot see, each checked from the host with plain torch:

* ``guarded_empty`` / ``guard_outputs`` / ``Guard.check``: every output a wrapper takes from ``torch.empty`` (``empty_like``,
  ``empty_strided``) lies between two 64 KiB bands of byte 0xFF and starts out as 0xFF itself.  After the call the bands must be
  untouched (nothing was stored outside the output) and no real scalar of the returned output may still be all-0xFF (every element
  was written by THIS call, not left over from the block's previous owner).  0xFF.. is a NaN in every float width whose payload no
  arithmetic produces (hardware NaNs are 0x7FC0.. / 0xFFC0.., ``np.nan`` is 0x7FF8..).
* ``haloed`` / ``haloed_view``: an input copied into the middle of a larger buffer whose surroundings are 0, NaN or Inf.  A result
  that depends on the fill has used a value outside its input.

Limits: the bands are 64 KiB wide (a wilder store is not seen); an INTEGER output that legitimately holds -1 (all bits set) reads as
"never written" -- no wrapper returns integers today; the library's own arenas and plan scratch are not torch tensors
(tests/test_gpu_scratch.py poisons them through QDAS_SCRATCH_POISON instead); an out-of-bounds READ whose value is discarded (masked by select) is invisible -- by design, that is legal."""
from __future__ import annotations

import contextlib
import math

import torch

G = 64 * 1024                    # guard width [bytes]: a multiple of 512, so the interior is aligned like a fresh torch allocation
FILL = 0xFF
_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
_REAL = {torch.complex32: torch.float16, torch.complex64: torch.float32, torch.complex128: torch.float64}

_empty, _empty_like, _empty_strided = torch.empty, torch.empty_like, torch.empty_strided


class GuardError(AssertionError):
    pass


class _Buf:
    def __init__(self, raw, nbytes, inner, what):
        self.raw, self.nbytes, self.inner, self.what = raw, nbytes, inner, what

    def band_damage(self):
        """byte offset, relative to the interior, of the first damaged guard byte; None when both bands are intact"""
        lo = (self.raw[:G] != FILL).nonzero()
        if lo.numel():
            return int(lo[0]) - G
        hi = (self.raw[G + self.nbytes:] != FILL).nonzero()
        if hi.numel():
            return self.nbytes + int(hi[0])
        return None

    def unwritten(self):
        """(count, first index) of the real scalars of the interior that are still all-0xFF"""
        t = self.inner
        if t.dtype in _REAL:                                  # each real component on its own: a half-written complex element counts
            es = t.element_size() // 2
            r = t.reshape(-1).view(_REAL[t.dtype]) if t.is_contiguous() else torch.view_as_real(t)
        else:
            es, r = t.element_size(), t
        bad = r.view(_INT[es]) == -1
        n = int(bad.sum())
        return n, (tuple(int(v) for v in bad.nonzero()[0]) if n else None)


class Guard:
    """The registry of one guarded region: every buffer handed out, with its raw allocation."""

    def __init__(self):
        self.bufs = []

    # -- allocation
    def empty_strided(self, shape, stride, dtype, device="cpu", what="empty"):
        shape, stride = tuple(int(s) for s in shape), tuple(int(s) for s in stride)
        es = _empty((), dtype=dtype, device="meta").element_size()
        n = 0 if math.prod(shape) == 0 else (1 + sum((s - 1) * st for s, st in zip(shape, stride))) * es
        raw = torch.full((n + 2 * G,), FILL, dtype=torch.uint8, device=device)
        inner = raw[G:G + n].view(dtype).as_strided(shape, stride)
        self.bufs.append(_Buf(raw, n, inner, f"{what}{shape} {dtype}"))
        return inner

    def empty(self, shape, dtype, device="cpu", what="empty"):
        shape = tuple(int(s) for s in shape)
        stride, run = [], 1
        for s in reversed(shape):
            stride.append(run)
            run *= max(s, 1)
        return self.empty_strided(shape, tuple(reversed(stride)), dtype, device, what)

    @property
    def nbytes(self):
        return sum(b.nbytes for b in self.bufs)

    # -- the check
    def check(self, *results, all_written=False):
        """Synchronise, then: (a) both bands of EVERY buffer are intact; (b) no real scalar is still 0xFF in the buffers whose storage one
        of ``results`` aliases (a workspace a wrapper does not return may stay partly unwritten) -- in every buffer with ``all_written``.
        Returns the number of buffers (b) was applied to."""
        if any(b.raw.is_cuda for b in self.bufs):
            torch.cuda.synchronize()
        flat = []
        for r in results:
            flat += list(r) if isinstance(r, (tuple, list)) else [r]
        ptrs = {r.untyped_storage().data_ptr() for r in flat if isinstance(r, torch.Tensor)}
        errs, applied = [], 0
        for k, b in enumerate(self.bufs):
            off = b.band_damage()
            if off is not None:
                errs.append(f"buffer {k} ({b.what}, {b.nbytes} bytes): guard band damaged, first byte at offset {off} relative to the interior")
            if all_written or b.raw.untyped_storage().data_ptr() in ptrs:
                applied += 1
                n, first = b.unwritten()
                if n:
                    errs.append(f"buffer {k} ({b.what}): {n} real scalar(s) never written, first at index {first}")
        if errs:
            raise GuardError("; ".join(errs))
        return applied


_DEFAULT = Guard()


def guarded_empty(shape, dtype, device="cpu", guard=None):
    """``torch.empty(shape, dtype, device)`` whose bytes are 0xFF, between two bands of ``G`` bytes of 0xFF; registered with ``guard``
    (default: the module's registry, see :func:`check`)."""
    return (guard or _DEFAULT).empty(shape, dtype, device)


def check(*results, all_written=False):
    """:meth:`Guard.check` of the module's registry, which is emptied."""
    try:
        return _DEFAULT.check(*results, all_written=all_written)
    finally:
        _DEFAULT.bufs.clear()


@contextlib.contextmanager
def guard_outputs(monkeypatch, cpu=False):
    """Within the block ``torch.empty``, ``torch.empty_like`` and ``torch.empty_strided`` hand out guarded device tensors (CPU requests pass
    through unless ``cpu``: the self-tests).  Yields the :class:`Guard`; call its ``check`` inside or after the block."""
    g = Guard()

    def wanted(proto_device):
        return proto_device.type == "cuda" or (cpu and proto_device.type == "cpu")

    def plain(kw):
        return not (kw.get("out") is not None or kw.get("pin_memory") or kw.get("requires_grad")
                    or kw.get("layout", torch.strided) is not torch.strided)

    def empty(*args, **kw):
        dev = torch.device(kw["device"]) if kw.get("device") is not None else torch.device("cpu")
        if not wanted(dev) or not plain(kw):
            return _empty(*args, **kw)
        p = _empty(*args, **{**kw, "device": "meta"})
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return g.empty_strided(p.shape, p.stride(), p.dtype, dev, "empty")

    def empty_like(t, **kw):
        dev = torch.device(kw["device"]) if kw.get("device") is not None else t.device
        if not wanted(dev) or not plain(kw):
            return _empty_like(t, **kw)
        p = _empty_like(t, **{**kw, "device": "meta"})
        return g.empty_strided(p.shape, p.stride(), p.dtype, dev, "empty_like")

    def empty_strided(size, stride, **kw):
        dev = torch.device(kw["device"]) if kw.get("device") is not None else torch.device("cpu")
        if not wanted(dev) or not plain(kw):
            return _empty_strided(size, stride, **kw)
        if dev.type == "cuda" and dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return g.empty_strided(size, stride, kw.get("dtype") or torch.get_default_dtype(), dev, "empty_strided")

    with monkeypatch.context() as m:
        m.setattr(torch, "empty", empty)
        m.setattr(torch, "empty_like", empty_like)
        m.setattr(torch, "empty_strided", empty_strided)
        yield g


# ---------------------------------------------------------------------------------------------------------------- inputs
def _fill_value(fill, dtype):
    v = {"0": 0.0, "nan": float("nan"), "inf": float("inf")}[str(fill)] if not isinstance(fill, float) else fill
    if dtype.is_complex:
        return complex(v, v)
    if not dtype.is_floating_point:
        if v != v or v in (float("inf"), -float("inf")):     # integers have no NaN / Inf: the largest value stands in
            return torch.iinfo(dtype).max
        return int(v)
    return v


def _full(n, value, dtype, device):
    if dtype == torch.complex32:                             # (no fill kernel for complex32: fill the halves)
        return torch.view_as_complex(torch.full((n, 2), value.real, dtype=torch.float16, device=device))
    return torch.full((n,), value, dtype=dtype, device=device)


def haloed(t, fill):
    """A contiguous copy of ``t`` in the interior of a larger buffer whose surroundings (``G`` bytes each side) hold ``fill`` (0, "nan" or
    "inf"; both components of a complex element; integers take their largest value for "nan" / "inf").  Aligned like a fresh allocation."""
    t = t.contiguous()
    pad = G // t.element_size()
    big = _full(t.numel() + 2 * pad, _fill_value(fill, t.dtype), t.dtype, t.device)
    inner = big[pad:pad + t.numel()].view(t.shape)
    inner.copy_(t)
    return inner


def haloed_view(t, fill):
    """``t`` with its OWN strides (a non-contiguous view stays one: ``big[::2, 1:N+1]``) inside a buffer in which every element ``t`` does not
    address -- the skipped elements of the view as well as ``G`` bytes each side -- holds ``fill``."""
    if t.numel() == 0:
        return t
    pad = G // t.element_size()
    span = 1 + sum((s - 1) * st for s, st in zip(t.shape, t.stride()))
    big = _full(span + 2 * pad, _fill_value(fill, t.dtype), t.dtype, t.device)
    inner = big.as_strided(tuple(t.shape), tuple(t.stride()), pad)
    inner.copy_(t)
    return inner
