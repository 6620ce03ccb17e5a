"""tests/guards.py catches what it claims to catch.  The "kernels" here are plain torch functions on the CPU: nothing on a GPU is ever asked
to misbehave."""
import numpy as np
import pytest
import torch

from tests import guards as GD

DTYPES = [torch.complex32, torch.complex64, torch.complex128, torch.float16, torch.float32, torch.float64, torch.int16]


def _good(src):
    """a well-behaved wrapper: takes its output from torch.empty and writes all of it"""
    y = torch.empty(src.shape, dtype=src.dtype, device=src.device)
    y.copy_(src)
    return y


def _src(dtype, n=37):
    if dtype.is_complex:
        return torch.view_as_complex(torch.arange(2.0 * n).reshape(n, 2).to(GD._REAL[dtype]))
    return torch.arange(n).to(dtype)


@pytest.mark.parametrize("dtype", DTYPES, ids=str)
def test_guarded_empty_is_aligned_sentinel_filled_and_passes_when_fully_written(dtype):
    y = GD.guarded_empty((5, 7), dtype)
    assert y.shape == (5, 7) and y.dtype == dtype and y.is_contiguous()
    raw = GD._DEFAULT.bufs[-1].raw
    assert (y.data_ptr() - raw.data_ptr()) == GD.G and GD.G % 512 == 0
    assert raw.numel() == 35 * y.element_size() + 2 * GD.G and bool((raw == 0xFF).all())
    with pytest.raises(GD.GuardError, match=r"35|70"):                 # nothing written yet: every scalar is reported
        GD._DEFAULT.check(y)
    y.copy_(_src(dtype, 35).reshape(5, 7))
    assert GD.check(y) == 1


def test_sentinel_is_a_nan_no_arithmetic_makes():
    for dt, it in ((torch.float16, torch.int16), (torch.float32, torch.int32), (torch.float64, torch.int64)):
        y = GD.guarded_empty((3,), dt)
        assert bool(torch.isnan(y).all())
        hw = (torch.zeros(3, dtype=dt) / 0).view(it)                    # the NaN arithmetic produces
        assert not bool((hw == -1).any()) and not bool((torch.full((3,), np.nan, dtype=dt).view(it) == -1).any())
    GD.check()


@pytest.mark.parametrize("dtype", [torch.float32, torch.complex64, torch.complex32, torch.int16], ids=str)
def test_fake_kernel_that_skips_the_last_element_is_reported(dtype, monkeypatch):
    src = _src(dtype)
    with GD.guard_outputs(monkeypatch, cpu=True) as g:
        y = torch.empty(src.shape, dtype=dtype)
        y[:-1] = src[:-1]
        with pytest.raises(GD.GuardError, match=r"never written, first at index \(7[23],\)|never written, first at index \(36,\)"):
            g.check(y)


def test_fake_kernel_that_writes_only_the_real_parts_is_reported(monkeypatch):
    src = _src(torch.complex64)
    with GD.guard_outputs(monkeypatch, cpu=True) as g:
        y = torch.empty_like(src)
        torch.view_as_real(y)[:, 0] = src.real
        with pytest.raises(GD.GuardError, match=r"37 real scalar\(s\) never written, first at index \(1,\)"):
            g.check(y)


def test_fake_kernel_that_writes_one_element_before_the_interior_is_reported(monkeypatch):
    src = _src(torch.float32)
    with GD.guard_outputs(monkeypatch, cpu=True) as g:
        y = _good(src)
        y.as_strided((1,), (1,), y.storage_offset() - 1).fill_(1.0)
        with pytest.raises(GD.GuardError, match=r"guard band damaged, first byte at offset -4 "):
            g.check(y)


def test_fake_kernel_that_writes_one_element_after_the_interior_is_reported(monkeypatch):
    src = _src(torch.complex128)
    with GD.guard_outputs(monkeypatch, cpu=True) as g:
        y = _good(src)
        y.as_strided((1,), (1,), y.storage_offset() + 37).fill_(1.0)
        with pytest.raises(GD.GuardError, match=rf"guard band damaged, first byte at offset {37 * 16} "):
            g.check(y)


def test_a_damaged_band_of_an_unreturned_workspace_is_reported_and_its_unwritten_part_is_not(monkeypatch):
    src = _src(torch.float32)
    with GD.guard_outputs(monkeypatch, cpu=True) as g:
        work = torch.empty(100, dtype=torch.float32)              # partly used scratch: legal
        work[:10] = 0
        y = _good(src)
        assert g.check(y) == 1 and len(g.bufs) == 2
        assert g.check(y.reshape(37, 1).t()) == 1                 # a view of the output aliases its buffer
        with pytest.raises(GD.GuardError, match="90 real"):
            g.check(y, all_written=True)
        work.as_strided((1,), (1,), work.storage_offset() + 100).fill_(0.0)
        with pytest.raises(GD.GuardError, match="buffer 0 .*offset 400 "):
            g.check(y)


def test_patch_covers_the_three_allocators_passes_cpu_through_by_default_and_is_undone(monkeypatch):
    before = (torch.empty, torch.empty_like, torch.empty_strided)
    with GD.guard_outputs(monkeypatch) as g:
        a = torch.empty((3, 4), dtype=torch.float32)              # a CPU request: not guarded
        b = torch.empty(3, 4, device="cpu")
        assert len(g.bufs) == 0 and a.shape == b.shape == (3, 4)
    with GD.guard_outputs(monkeypatch, cpu=True) as g:
        a = torch.empty((3, 4), dtype=torch.float64)
        b = torch.empty(3, 4)
        c = torch.empty_like(a.t())
        d = torch.empty_strided((3, 1, 4), (1, 12, 3), dtype=torch.complex64)
        assert len(g.bufs) == 4 and b.dtype == torch.float32 and c.stride() == a.t().stride() and d.stride() == (1, 12, 3)
        assert g.nbytes == 96 + 48 + 96 + 96
        for t in (a, b, c, d):
            t.zero_()
        assert g.check(a, b, c, d) == 4
    assert (torch.empty, torch.empty_like, torch.empty_strided) == before


@pytest.mark.parametrize("fill", [0, "nan", "inf"])
def test_haloed_surroundings_and_a_fake_kernel_that_multiplies_a_halo_sample_by_zero(fill):
    x = torch.arange(1.0, 9.0)

    def by_select(v):                                             # reads one element past the end, discards it
        w = v.as_strided((9,), (1,), v.storage_offset())
        return torch.where(torch.arange(9) < 8, w, torch.zeros(())).sum()

    def by_multiply(v):                                           # ... multiplies it by zero instead
        w = v.as_strided((9,), (1,), v.storage_offset())
        return (w * (torch.arange(9) < 8)).sum()

    h = GD.haloed(x, fill)
    assert torch.equal(h, x) and h.is_contiguous() and h.storage_offset() * 4 == GD.G
    out = h.as_strided((2,), (h.numel() + 1,), h.storage_offset() - 1)
    want = {0: 0.0, "nan": np.nan, "inf": np.inf}[fill]
    assert np.array_equal(out.numpy(), np.array([want, want], np.float32), equal_nan=True)
    assert by_select(h) == 36.0
    if fill == 0:
        assert by_multiply(h) == 36.0                             # finite surroundings hide the defect ...
    else:
        assert torch.isnan(by_multiply(h))                        # ... NaN and Inf report it


def test_haloed_complex_and_integer_fills():
    c = GD.haloed(_src(torch.complex32, 5), "inf")
    raw = torch.view_as_real(c.as_strided((1,), (1,), c.storage_offset() - 1))
    assert bool(torch.isinf(raw).all())
    i = GD.haloed(torch.arange(5, dtype=torch.int16), "nan")
    assert int(i.as_strided((1,), (1,), i.storage_offset() + 5)) == 32767 and torch.equal(i, torch.arange(5, dtype=torch.int16))


def test_haloed_view_fills_the_skipped_elements_too():
    N = 4
    big = torch.zeros((6, N + 3))
    big[::2, 1:N + 1] = torch.arange(1.0, 13.0).reshape(3, 4)
    v = big[::2, 1:N + 1]
    h = GD.haloed_view(v, "nan")
    assert h.stride() == v.stride() and not h.is_contiguous() and torch.equal(h, v)
    span = h.as_strided((2 * (N + 3) * 2 + N,), (1,), h.storage_offset())
    assert int(torch.isnan(span).sum()) == span.numel() - 12      # everything the view does not address
    before = h.as_strided((4,), (1,), h.storage_offset() - 4)
    assert bool(torch.isnan(before).all())
