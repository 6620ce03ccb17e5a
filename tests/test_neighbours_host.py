"""tests/neighbours.py catches what it claims to catch.  The "kernels" here are plain torch functions in float32 on the CPU: nothing on a GPU is ever asked to
misbehave.  The last test walks the rows of tests/test_gpu_neighbours.py on the CPU, through their float64 restatements alone, and checks that the scaled inputs
keep every output far inside float32's normal range -- the premise of the bit-exact check A."""
import numpy as np
import pytest
import torch

from tests import neighbours as NB
from tests.test_preproc import hilbert_ref

T, K, L = 48, 7, 5
BOUND = 2e-5                                   # tests/test_preproc.py:49, tests/test_convd.py:110


def _x(seed=0, shape=(T, K)):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal(shape).astype(np.float32))


def _taps(seed=1, shape=(L,)):
    return torch.from_numpy(np.random.default_rng(seed).uniform(0.5, 1.5, shape).astype(np.float32))


def fir(x, h, leak=0.0, const=0.0):
    """causal FIR along dim 0, one column per member; taps shared (L) or per member (L x K); float32 multiply-then-add in tap order"""
    y = torch.zeros_like(x)
    for j in range(h.shape[0]):
        hj = h[j] if h.ndim == 1 else h[j].unsqueeze(0)
        y[j:] = y[j:] + hj * x[:x.shape[0] - j]
    if leak:                                    # the window of the member's last output reaches one sample into the next member
        y[-1, :-1] = y[-1, :-1] + leak * x[0, 1:]
    return y + const if const else y


def fir_ref(x, h, *_):
    x, h = x.double(), h.double()
    y = torch.zeros_like(x)
    for j in range(h.shape[0]):
        y[j:] += (h[j] if h.ndim == 1 else h[j].unsqueeze(0)) * x[:x.shape[0] - j]
    return y


def fft_filter(x, H):
    """per-member filter in the frequency domain, complex64 transforms along dim 0"""
    return torch.fft.ifft(torch.fft.fft(x.to(torch.complex64), dim=0) * H.unsqueeze(1), dim=0)


def packed_hilbert(x):
    """the float32 restatement of the one-pass kernel's packing: columns 2j and 2j+1 share one complex64 transform z = x1 + i x2"""
    N, Kc = x.shape
    xp = torch.cat([x, x.new_zeros(N, Kc % 2)], 1)
    x1, x2 = xp[:, 0::2], xp[:, 1::2]
    w = torch.zeros(N)
    w[0] = 1
    w[1:N // 2] = 2
    w[N // 2] = 1 + N % 2
    Y = torch.fft.ifft(torch.fft.fft(torch.complex(x1, x2), dim=0) * w.unsqueeze(1), dim=0)
    y = torch.empty((N, xp.shape[1]), dtype=torch.complex64)
    y[:, 0::2] = torch.complex(x1, Y.imag - x2)
    y[:, 1::2] = torch.complex(x2, x1 - Y.real)
    return y[:, :Kc]


def _abc(spec, fn, inputs, ref, bound=BOUND):
    """A, then B on the scaled inputs, then C"""
    spec.check_scale(fn, inputs)
    xs, _ = spec.scaled(inputs)
    worst = spec.check_parity(spec.run(fn, xs), ref(*xs), bound)
    spec.check_poison(fn, inputs)
    return worst


# ---------------------------------------------------------------------------------------------------------------- honest kernels pass
@pytest.mark.parametrize("per_member", [False, True])
def test_an_honest_fir_passes_a_b_and_c(per_member):
    spec = NB.Spec([1, 1 if per_member else None], 1)
    h = _taps(shape=(L, K) if per_member else (L,))
    assert _abc(spec, fir, [_x(), h], fir_ref) <= 1e-6


def test_an_honest_fft_filter_passes_a_b_and_c():
    H = torch.from_numpy(np.exp(-np.arange(T) / 9.0).astype(np.float32))
    spec = NB.Spec([1, None], 1)
    ref = lambda x, H: torch.from_numpy(np.fft.ifft(np.fft.fft(x.double().numpy(), axis=0) * H.double().numpy()[:, None], axis=0))
    assert _abc(spec, fft_filter, [_x(), H], ref) <= 1e-5


def test_members_over_two_axes_and_a_filter_per_column_only():
    """x (T, 4, 3) with members over axes 1 and 2, taps (L, 4, 1): the output carries the sum of both exponents"""
    x, h = _x(shape=(T, 4, 3)), _taps(shape=(L, 4, 1))

    def fn(x, h):
        y = torch.zeros_like(x)
        for j in range(L):
            y[j:] = y[j:] + h[j].unsqueeze(0) * x[:T - j]
        return y
    spec = NB.Spec([(1, 2), (1, None)], (1, 2))
    xs, e = spec.scaled([x, h])
    assert tuple(e.shape) == (4, 3) and len(set(e.reshape(-1).tolist())) > 4
    assert torch.equal(xs[0][:, 1, 2], x[:, 1, 2] * 2.0 ** NB.EXP[torch.float32][5 % 4]) and torch.equal(xs[1][:, 1, 0], h[:, 1, 0] * 2.0 ** -20)   # (the table reversed)
    spec.check_scale(fn, [x, h])
    spec.check_poison(fn, [x, h])


def test_powers_of_two_are_made_from_bits():
    """(``torch.ldexp`` multiplies by ``pow(2.0, e)``; on an MI355X that product was off in the last bit and every float32 row failed A)"""
    for dt, lo, hi in ((torch.float16, -14, 15), (torch.float32, -126, 127), (torch.float64, -1022, 1023)):
        e = torch.arange(lo, hi + 1)
        assert torch.equal(NB.pow2(e, dt).double(), torch.tensor(2.0, dtype=torch.float64) ** e)
    x = _x()
    assert torch.equal(NB.ldexp(x, torch.tensor(-20)), x / 2.0 ** 20)
    with pytest.raises(AssertionError):
        NB.pow2(torch.tensor([128]), torch.float32)


def test_int16_units_are_multiplied_by_1_16_4_2():
    x = torch.from_numpy(np.random.default_rng(0).integers(-2000, 2001, (T, 6)).astype(np.int16))
    spec = NB.Spec([1], 1)
    xs, e = spec.scaled([x])
    assert xs[0].dtype == torch.int16 and e.tolist() == [0, 4, 2, 1, 0, 4] and torch.equal(xs[0][:, 1], x[:, 1] * 16)
    spec.check_scale(lambda v: v.float() * 0.3, [x])
    spec.check_poison(lambda v: v.float() * 0.3, [x])


# ---------------------------------------------------------------------------------------------------------------- the defects are reported
def test_a_fir_that_reads_one_sample_of_the_next_member_is_rejected_by_a_b_and_c():
    """a leak of 1e-6 of the neighbour: invisible at equal amplitudes under the suites' 2e-5 of the global maximum, reported by each of the three checks"""
    x, h = _x(), _taps()
    leaky = lambda x, h: fir(x, h, leak=1e-6)
    spec = NB.Spec([1, None], 1)
    y, ref = leaky(x, h), fir_ref(x, h)
    assert float((y - ref).abs().max() / ref.abs().max()) <= BOUND                     # what the parity tests see: nothing
    with pytest.raises(NB.NeighbourError, match=rf"not the clean output times its unit's power of two: \d+ element\(s\), first at \({T - 1}, 0\)"):
        spec.check_scale(leaky, [x, h])
    xs, _ = spec.scaled([x, h])
    with pytest.raises(NB.NeighbourError, match=r"over the unit's max\|ref\|"):
        spec.check_parity(leaky(*xs), fir_ref(*xs), BOUND)
    with pytest.raises(NB.NeighbourError, match=rf"unpoisoned units changed \(nan in the even units\), first at \({T - 1}, 1\)"):       # (member 1 reads member 2)
        spec.check_poison(leaky, [x, h])


def test_the_pair_packed_hilbert_is_rejected_trace_by_trace_and_accepted_pair_by_pair():
    x = _x(shape=(256, 5))                                                               # odd: the last trace is single
    ref = lambda v: torch.from_numpy(hilbert_ref(v.double().numpy()))
    one, two = NB.Spec([1], 1), NB.Spec([1], 1, group=2)
    with pytest.raises(NB.NeighbourError, match="power of two"):
        one.check_scale(packed_hilbert, [x])
    xs, _ = one.scaled([x])
    with pytest.raises(NB.NeighbourError, match=r"max\|ref\|"):
        one.check_parity(packed_hilbert(*xs), ref(*xs), BOUND)
    with pytest.raises(NB.NeighbourError, match="unpoisoned units changed"):
        one.check_poison(packed_hilbert, [x])
    assert _abc(two, packed_hilbert, [x], ref) <= BOUND
    xs, e = two.scaled([x])
    assert e.tolist() == [0, 0, 20, 20, -20]


def test_an_exact_kernel_that_adds_a_constant_is_rejected_by_a():
    with pytest.raises(NB.NeighbourError, match="power of two"):
        NB.Spec([1, None], 1).check_scale(lambda x, h: fir(x, h, const=1.0), [_x(), _taps()])


def test_an_output_unit_left_unwritten_is_rejected(monkeypatch):
    def lazy(x, h):
        y = torch.empty(x.shape, dtype=x.dtype)
        y[:, :-1] = fir(x, h)[:, :-1]
        return y
    with pytest.raises(NB.NeighbourError, match=rf"{T} real scalar\(s\) never written"):
        NB.Spec([1, None], 1, guard=(monkeypatch, True)).check_scale(lazy, [_x(), _taps()])
    NB.Spec([1, None], 1, guard=(monkeypatch, True)).check_scale(lambda x, h: fir(x, h) + torch.empty(x.shape).zero_(), [_x(), _taps()])


def test_a_stale_unit_without_the_sentinel_is_still_seen_when_its_exponent_is_not_zero():
    """without ``guard`` an unwritten unit holds whatever the allocator hands back; the worst case is the clean run's own result"""
    keep = {}

    def stale(x, h):
        y = fir(x, h)
        if "y" in keep:
            y[:, 1] = keep["y"][:, 1]
        keep.setdefault("y", y.clone())
        return y
    with pytest.raises(NB.NeighbourError, match=r"first at \(0, 1\)"):
        NB.Spec([1, None], 1).check_scale(stale, [_x(), _taps()])


# ---------------------------------------------------------------------------------------------------------------- the GPU rows' inputs
from tests import test_gpu_neighbours as G  # noqa: E402  (the table only: nothing in it touches a device before a row is called)

RANGE = {"f32": (2.0 ** -100, 2.0 ** 100), "f64": (2.0 ** -200, 2.0 ** 200),
         "f16": (0.0, 65504.0)}                 # (half rows take B and C only: a subnormal output is legal there, an overflow is not)


@pytest.mark.parametrize("row", G.ROWS, ids=lambda r: r.name)
def test_gpu_rows_keep_every_output_inside_the_normal_range(row):
    """the smallest non-zero |ref| of the clean and of the scaled run is >= 2^-100 and the largest <= 2^100 (float64 rows: 2^-200 and 2^200), computed from the
    row's float64 restatement on the CPU; and the table's own shapes are consistent: the restatement has the shape the row's output axes index"""
    inputs = row.inputs()
    spec = row.spec()
    lo, hi = RANGE[row.prec]
    xs, e = spec.scaled(inputs)
    for ins in (inputs, xs):
        refs = NB._tup(row.ref(*ins))
        assert len(refs) == len(spec.out_axes)
        for ref, axes in zip(refs, spec.out_axes):
            a = torch.as_tensor(ref).abs()
            assert [a.shape[x] for x in axes if x is not None] == [s for s, x in zip(e.shape, axes) if x is not None], (row.name, tuple(a.shape), tuple(e.shape))
            a = a[(a > 0) & ~torch.isnan(a)]
            assert a.numel() and float(a.min()) >= lo and float(a.max()) <= hi, (row.name, float(a.min()), float(a.max()))


def test_the_table_names_every_entry_of_the_issue():
    assert {r.entry for r in G.ROWS} >= {"hilbert fixed list", "hilbert run-time list", "hilbert 512-thread lists", "hilbert hipFFT passes", "convd time-contiguous",
                                         "convd strided", "convd half", "convd FFT path", "sosfilt", "shift_sum", "pwznxcorr", "refocus", "migrate", "scan_convert",
                                         "scan_convert3", "ray_integrals", "ray_backproject", "demod", "resample", "filtfilt"}


def test_a_clean_unit_without_a_finite_non_zero_value_is_rejected():
    """an all-NaN or all-zero unit would pass A and C whatever the kernel did (NaN keeps its bits for the pixels outside a scan converter's mask)"""
    def hollow(fill):
        def fn(x, h):
            y = fir(x, h)
            y[:, 2] = fill
            return y
        return fn
    spec = NB.Spec([1, None], 1)
    for fill in (float("nan"), 0.0):
        with pytest.raises(NB.NeighbourError, match="unit 2 of the clean run holds no finite non-zero value"):
            spec.check_scale(hollow(fill), [_x(), _taps()])
        with pytest.raises(NB.NeighbourError, match="unit 2 of the clean run holds no finite non-zero value"):
            spec.check_poison(hollow(fill), [_x(), _taps()])

    def masked(x, h):                                                   # NaN at SOME elements of every unit: legal
        y = fir(x, h)
        y[:3] = float("nan")
        return y
    spec.check_scale(masked, [_x(), _taps()])
