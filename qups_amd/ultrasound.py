"""The caller's side of the path: a Python mirror of ``UltrasoundSystem.DAS`` / ``bfDAS`` / ``bfDASLUT``.

Only what those three methods need is modelled: small value classes carrying the
arrays the reference's definition classes emit -- element positions / normals, the pixel grid, the sequence type
and foci, the channel data with its time axis -- and the argument marshalling of
``UltrasoundSystem.DAS`` (reference ``src/UltrasoundSystem.m:3297-3371``), ``bfDAS`` (``:4429-4473``) and
``bfDASLUT`` (``:4476-4673``).  Simulators, other beamformers, interop, plotting etc. are out of scope.
"""
from __future__ import annotations

import math
from dataclasses import dataclass, field

import numpy as np

from . import geometry as G
from .das_spec import DasError, das_spec
from .interpd import sample2sep, wsinterpd


@dataclass
class Transducer:
    """Element positions ``3 x N`` and normals ``3 x N`` (what ``positions()`` / ``orientations()`` return)."""
    pos: np.ndarray
    normals: np.ndarray
    fc: float = 5e6
    offset: np.ndarray = field(default_factory=lambda: np.zeros(3))
    kind: str = "Transducer"            # the reference's class of the array: 'TransducerArray' (linear), 'TransducerConvex', 'TransducerMatrix', or the generic base
    pitch: float | None = None          # element spacing of a linear array

    @property
    def numel(self):
        return self.pos.shape[1]

    def positions(self):
        return self.pos

    @staticmethod
    def linear(numel, pitch, fc=5e6, offset=(0.0, 0.0, 0.0)):          # reference src/TransducerArray.m:95-109
        p, n = G.linear_array(numel, pitch, offset)
        return Transducer(p, n, fc, np.asarray(offset, float), "TransducerArray", float(pitch))

    @staticmethod
    def matrix(numd, pitch, fc=5e6, offset=(0.0, 0.0, 0.0)):           # reference src/TransducerMatrix.m:130-147
        p, n = G.matrix_array(numd, pitch, offset)
        return Transducer(p, n, fc, np.asarray(offset, float), "TransducerMatrix")

    @staticmethod
    def convex(numel, radius, angular_pitch_deg, fc=3.7e6, offset=(0.0, 0.0, 0.0)):   # reference src/TransducerConvex.m:85-102
        p, n = G.convex_array(numel, radius, angular_pitch_deg, offset)
        return Transducer(p, n, fc, np.asarray(offset, float), "TransducerConvex")


@dataclass
class Sequence:
    """``type`` in ``{'FSA','PW','FC','VS','DV'}`` (reference ``src/Sequence.m:62``); ``focus`` is ``3 x M``: foci for
    FC/VS/DV, unit normal vectors for PW (reference ``src/UltrasoundSystem.m:3346``)."""
    type: str = "FSA"
    focus: np.ndarray | None = None
    c0: float = 1540.0
    numPulse: int | None = None

    def delays(self, tx: "Transducer"):
        """``tau = delays(seq, tx)``: ``N x S`` transmit delays (reference ``src/Sequence.m:888-931``): FC ``+|focus - p|/c0``,
        DV the negative, VS signed by whether every element lies in front of the focus, PW ``-(n . p)/c0``, FSA zeros."""
        p = np.asarray(tx.positions(), float)
        N = p.shape[1]
        if self.type == "FSA":
            return np.zeros((N, N))
        f = np.asarray(self.focus, float)
        if self.type == "PW":
            return -(f[:, None, :] * p[:, :, None]).sum(0) / self.c0
        v = f[:, None, :] - p[:, :, None]
        tau = np.sqrt((v ** 2).sum(0)) / self.c0
        if self.type == "FC":
            return tau
        if self.type == "DV":
            return -tau
        if self.type == "VS":
            return tau * np.where(np.all(f[2][None, :] > p[2][:, None], axis=0), 1.0, -1.0)[None, :]
        raise DasError(f"Unknown sequence type {self.type!r}.")

    def t0Offset(self):
        """``t0 = t0Offset(seq)``: the time offset from the foci to the transducer origin, one value per transmit (reference ``src/Sequence.m:1042-1050``):
        ``-|focus| / c0`` for FC and VS, ``+|focus| / c0`` for DV, 0 for FSA and PW"""
        if self.type in ("FSA", "PW"):
            return np.zeros(1)
        r = np.sqrt((np.asarray(self.focus, float) ** 2).sum(0)) / self.c0
        if self.type in ("FC", "VS"):
            return -r
        if self.type == "DV":
            return r
        raise DasError(f"Unknown sequence type {self.type!r}.")

    def apodization(self, tx: "Transducer"):
        """``N x S`` transmit apodization (reference ``src/Sequence.m:953-975``): identity for FSA, ones otherwise"""
        N = tx.numel
        if self.type == "FSA":
            return np.eye(N)
        S = self.numPulse or (np.asarray(self.focus).shape[1] if self.focus is not None else N)
        return np.ones((N, S))


@dataclass
class Scan:
    """Pixel grid: ``positions()`` is ``3 x I1 x I2 x I3`` (reference ``src/Scan.m:194``)."""
    pos: np.ndarray
    # the axes the positions were made from, when a constructor below made them: {"kind": "cartesian" | "polar" | "spherical", ...}; None for positions alone
    axes: dict | None = field(default=None, compare=False, repr=False)

    @property
    def size(self):
        return tuple(self.pos.shape[1:4])

    def positions(self):
        return self.pos

    @staticmethod
    def cartesian(x, z, y=(0.0,)):                   # order 'ZXY' (reference src/ScanCartesian.m:11,126-143)
        ax = dict(kind="cartesian", **{k: np.asarray(v, float).reshape(-1) for k, v in (("x", x), ("y", y), ("z", z))})
        return Scan(G.scan_cartesian(x, z, y), ax)

    @staticmethod
    def polar(r, a_deg, origin=(0.0, 0.0, 0.0)):     # order 'RAY' (reference src/ScanPolar.m:11,99-115)
        ax = dict(kind="polar", r=np.asarray(r, float).reshape(-1), a=np.asarray(a_deg, float).reshape(-1), origin=np.asarray(origin, float).reshape(3))
        return Scan(G.scan_polar(r, a_deg, origin), ax)

    @staticmethod
    def spherical(r, a_deg, e_deg, origin=(0.0, 0.0, 0.0)):     # order 'RAE' (reference src/ScanSpherical.m:11,77-93)
        ax = dict(kind="spherical", r=np.asarray(r, float).reshape(-1), a=np.asarray(a_deg, float).reshape(-1), e=np.asarray(e_deg, float).reshape(-1),
                  origin=np.asarray(origin, float).reshape(3))
        return Scan(G.scan_spherical(r, a_deg, e_deg, origin), ax)

    def scanConvert(self, b, scanC: "Scan | None" = None, **kw):
        """``(b_cart, scanC) = scanConvert(scan, b)`` / ``scanConvert(scan, b, scanC)`` (reference ``src/ScanPolar.m:143-201``,
        ``src/ScanSpherical.m:121-188``): the image ``b`` on this polar (spherical) scan -- ``R x A x ...`` (``R x A x E x ...``), what ``DAS`` returns -- on
        the Cartesian scan ``scanC``, by default the one that encloses this scan (``ScanCartesian(scan)``).  Keywords (``pre``, ``db_floor``, ``fill``,
        ``check_grid``) go to :func:`qups_amd.scanconvert.scan_convert` / ``scan_convert3``.  Works on scans made by :meth:`polar` / :meth:`spherical`
        (and a ``scanC`` made by :meth:`cartesian`): positions alone do not tell the data's order."""
        from . import scanconvert as SC
        ax = self.axes
        if ax is None or ax.get("kind") not in ("polar", "spherical"):
            raise DasError("Data must be in order 'RAY'.")          # (the reference's refusal, src/ScanPolar.m:193: such a scan does not say how b is ordered)
        given = {}
        if scanC is not None:
            if scanC.axes is None or scanC.axes.get("kind") != "cartesian":
                raise DasError("scanC must be a Cartesian scan made by Scan.cartesian (order 'ZXY').")
            given = dict(x=scanC.axes["x"], z=scanC.axes["z"])
        if ax["kind"] == "polar":
            bc, (x, y, z) = SC.scan_convert(b, ax["r"], ax["a"], ax["origin"], **given, **kw)
        else:
            if scanC is not None:
                given["y"] = scanC.axes["y"]
            bc, (x, y, z) = SC.scan_convert3(b, ax["r"], ax["a"], ax["e"], ax["origin"], **given, **kw)
        return bc, (scanC if scanC is not None else Scan.cartesian(x, z, y))


@dataclass
class ChannelData:
    """``data`` is ``T x N x M x F...`` in ``order='TNM'`` (any permutation of the three letters is accepted and put in order by
    :meth:`rectifyDims`); ``t0`` scalar or one value per transmit (``1 x 1 x M``); ``fs`` scalar (reference ``src/ChannelData.m``)."""
    data: object
    t0: object = 0.0
    fs: float = 1.0
    order: str = "TNM"

    # -- the pieces of ChannelData the DAS path calls
    def _torch_data(self):
        import torch
        return self.data if hasattr(self.data, "is_cuda") else torch.from_numpy(np.asarray(self.data))

    @property
    def T(self):
        return int(self.data.shape[self.order.index("T")])

    def rectifyDims(self):
        """``T x N x M x ...`` order (reference ``src/ChannelData.m:1895-1913``): permutes ``data`` (and a non-scalar ``t0``)"""
        if self.order[:3] == "TNM":
            return self
        d = self._torch_data()
        lead = [self.order.index(c) for c in "TNM"]
        perm = lead + [k for k in range(max(d.ndim, 3)) if k not in lead]
        d = d.reshape(tuple(d.shape) + (1,) * (len(perm) - d.ndim)).permute(*perm)
        t0 = self.t0
        if np.ndim(t0) > 0 and np.size(t0) > 1:
            t0a = np.asarray(t0)
            t0a = t0a.reshape(t0a.shape + (1,) * (len(perm) - t0a.ndim)).transpose(perm)
            t0 = t0a
        return ChannelData(d, t0, self.fs, "TNM")

    def zeropad(self, B=0, A=0):
        """``B`` zeros in front (``t0`` moves back by ``B/fs``), ``A`` behind, along time (reference ``src/ChannelData.m:1153-1183``)"""
        import torch
        if A < 0 or B < 0:
            raise DasError("Data append or prepend size must be positive.")
        if A == 0 and B == 0:
            return self
        d = self._torch_data()
        ax = self.order.index("T")
        z = lambda n: torch.zeros(tuple(d.shape[:ax]) + (n,) + tuple(d.shape[ax + 1:]), dtype=d.dtype, device=d.device)
        return ChannelData(torch.cat([z(B), d, z(A)], ax), np.asarray(self.t0, float) - B / self.fs if np.ndim(self.t0) else float(self.t0) - B / self.fs,
                           self.fs, self.order)

    def filter(self, b, dim=None, a=None, sos=None, gain=1.0):
        """Filter the data along time -- what ``filter(chd, D)`` does with a ``digitalFilter`` ``D`` (reference ``src/ChannelData.m:857-888``: ``filter(D, x)``
        along the time dimension, then ``t0 -= L / fs`` with ``L = filtord(D) / 2`` for an FIR and ``L = filtord(D)`` for an IIR filter, ``:876-879``).
        FIR (``b`` alone): the causal convolution ``y[t] = sum_k b[k] x[t - k]`` on the device (``qdas_convd`` with the ``'causal'`` window).
        IIR: second-order sections ``sos`` (``n x 6``, MATLAB's ``D.Coefficients``) with ``gain``, or a transfer function ``(b, a)`` -- converted to sections
        (``scipy.signal.tf2sos``: MATLAB's own ``filter(b, a, x)`` runs the direct form; the two agree to rounding) -- on the device (``qdas_iir``)."""
        import torch
        ax = self.order.index("T") if dim is None else int(dim) - 1
        d = self._torch_data()
        if sos is not None or a is not None:
            from .convd import sosfilt
            if sos is None:
                from scipy.signal import tf2sos
                bb, aa = np.atleast_1d(np.asarray(b, float)), np.atleast_1d(np.asarray(a, float))
                order = max(len(bb), len(aa)) - 1
                sos = tf2sos(bb, aa) if order > 0 else np.array([[bb[0], 0, 0, aa[0], 0, 0]], float)
            else:
                sos = np.asarray(sos, float).reshape(-1, 6)
                deg = lambda c: 2 if c[2] != 0 else (1 if c[1] != 0 else 0)
                order = int(max(sum(deg(r[0:3]) for r in sos), sum(deg(r[3:6]) for r in sos)))      # filtord of the cascade: the degree of its transfer function
            if d.dtype in (torch.float16, torch.complex32):
                d = d.to(torch.complex64 if d.is_complex() else torch.float32)
            y = sosfilt(d, sos, ax + 1, gain)
            t0 = self.t0
            if ax == self.order.index("T"):
                t0 = np.asarray(t0, float) - order / self.fs if np.ndim(t0) else float(t0) - order / self.fs
            return ChannelData(y, t0, self.fs, self.order)
        from .convd import convd
        bt = b if hasattr(b, "is_cuda") else torch.from_numpy(np.asarray(b))
        bt = bt.reshape(-1)
        if not (bt.is_floating_point() or bt.is_complex()):
            bt = bt.to(torch.float64)
        if d.dtype in (torch.float32, torch.complex64, torch.float16, torch.complex32) and bt.dtype in (torch.float64, torch.complex128):
            bt = bt.to(torch.complex64 if bt.is_complex() else torch.float32)      # (coefficients follow the data's precision, as MATLAB's filter does for single data)
        y = convd(d, bt.reshape((1,) * ax + (-1,) + (1,) * (d.ndim - ax - 1)), ax + 1, "causal")
        t0 = self.t0
        if ax == self.order.index("T"):
            L = (bt.numel() - 1) / 2.0                           # filtord / 2
            t0 = np.asarray(t0, float) - L / self.fs if np.ndim(t0) else float(t0) - L / self.fs
        return ChannelData(y, t0, self.fs, self.order)

    def hilbert(self, N=None):
        """analytic signal along time (reference ``src/ChannelData.m:935-966``: ``hilbert(chd, N)``, zero-padded / truncated to ``N`` points)
        on the device: real fp32 / int16 traces go through the one-pass kernel of ``qdas_pre_*`` (``qups_amd/csrc/pre.hip``)"""
        from .preproc import hilbert
        d = self._torch_data()
        ax = self.order.index("T")
        if d.is_complex():
            raise DasError("hilbert expects real data")
        y = hilbert(d.movedim(ax, 0), N)
        return ChannelData(y.movedim(0, ax), self.t0, self.fs, self.order)

    def downmix(self, fc: float):
        """``chd.data .* exp(-2i*pi*fc*time)`` (reference ``src/ChannelData.m:757-766``); for real traces the Hilbert transform and the mixing are
        ONE pass over the data (``hilbert`` with ``fdown``), complex data are multiplied on the device"""
        import torch
        d = self._torch_data()
        ax = self.order.index("T")
        t0 = np.asarray(self.t0, float)
        if not d.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("qups_amd: no HIP device visible -- downmix has no CPU fallback")
            d = d.cuda()
        n = torch.arange(d.shape[ax], device=d.device, dtype=torch.float64).reshape((1,) * ax + (-1,) + (1,) * (d.ndim - ax - 1))
        if t0.size == 1:
            t0t = float(t0.reshape(-1)[0])
        else:                                                        # one start time per transmit: an array that broadcasts against the data
            if t0.ndim > d.ndim or any(a not in (1, b) for a, b in zip(t0.shape, d.shape)):
                raise DasError("downmix: t0 must be a scalar or broadcast against the data")
            t0t = torch.from_numpy(t0.reshape(t0.shape + (1,) * (d.ndim - t0.ndim))).to(d.device)
        cyc = fc * (t0t + n / self.fs)
        ph = (-2.0 * np.pi) * (cyc - torch.floor(cyc))
        cdt = torch.complex128 if d.dtype in (torch.float64, torch.complex128) else torch.complex64
        return ChannelData(d.to(cdt) * torch.polar(torch.ones_like(ph), ph).to(cdt), self.t0, self.fs, self.order)

    def downsample(self, ratio: int):
        """every ``ratio``-th sample along time (reference ``src/ChannelData.m:1042-1058``: ``subD(chd, 1:ratio:chd.T, chd.tdim)``); ``fs`` follows"""
        ratio = int(ratio)
        if ratio < 1:
            raise DasError("ratio must be a positive integer")
        d = self._torch_data()
        ax = self.order.index("T")
        idx = [slice(None)] * d.ndim
        idx[ax] = slice(0, None, ratio)
        return ChannelData(d[tuple(idx)].contiguous(), self.t0, self.fs / ratio, self.order)

    def demod(self, fc: float, ratio: int, b, out_half=False):
        """``downmix(fc)`` -> ``filter(b)`` -> ``downsample(ratio)`` in ONE pass over the record (``qdas_demod``, ``qups_amd/csrc/demod.hip``): the
        reference's recipe for baseband imaging (the example in the help text of ``downmix``, ``src/ChannelData.m:757-807``), to be followed by
        ``DAS(us, chd, fmod=fc)``.  ``b``: real FIR taps (:meth:`getLowpassFilter`).  The result has ``t0 - (K - 1) / 2 / fs`` (a per-transmit ``t0``
        keeps its shape) and ``fs / ratio``; any ``order`` is accepted and kept.  For real data the result carries half the analytic amplitude, exactly as
        the composition does (``2 * b`` restores it).  ``out_half``: complex32 data, what ``DAS(..., prec='halfT')`` takes."""
        import torch
        from .demod import demod
        d = self._torch_data()
        ax = self.order.index("T")
        if not d.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("qups_amd: no HIP device visible -- demod has no CPU fallback")
            d = d.cuda()
        t0 = np.asarray(self.t0, float)
        t0m = t0
        if t0.size > 1:
            if t0.ndim > d.ndim or any(a not in (1, b_) for a, b_ in zip(t0.shape, d.shape)) or (t0.ndim > ax and t0.shape[ax] != 1):
                raise DasError("demod: t0 must be a scalar or broadcast against the data (and not vary along time)")
            t0m = np.moveaxis(t0.reshape(t0.shape + (1,) * (d.ndim - t0.ndim)), ax, 0)
        K = int(b.numel()) if hasattr(b, "numel") else int(np.size(b))
        y = demod(d.movedim(ax, 0), fc, self.fs, t0m, b, ratio, out_half=out_half)
        L = (K - 1) / 2.0
        return ChannelData(y.movedim(0, ax), t0 - L / self.fs if np.ndim(self.t0) else float(self.t0) - L / self.fs, self.fs / int(ratio), self.order)

    def _device_data(self, what):
        import torch
        d = self._torch_data()
        if not d.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError(f"qups_amd: no HIP device visible -- {what} has no CPU fallback")
            d = d.cuda()
        return d

    def resample(self, fs: float, n: int = 10, beta: float = 5.0, p=None, q=None):
        """The data at the sampling frequency ``fs`` (reference ``src/ChannelData.m:1059-1094``) by a rational-rate polyphase FIR on the device
        (``qdas_resample``, ``qups_amd/csrc/resample.hip``): MATLAB's uniform ``resample(x, p, q, n, beta)`` with its default Kaiser-windowed design.
        ``p / q = Fraction(fs / self.fs).limit_denominator(4096)``; when that does not reproduce ``fs`` to 1e-9 relative the call raises and asks for explicit
        ``p, q``.  ``t0`` is unchanged and the new ``fs`` is ``self.fs p / q``; any ``order`` is accepted and kept.
        TWO DEVIATIONS from the reference: it computes in double and casts back, this computes in the data's precision; and it calls MATLAB's non-uniform
        syntax ``resample(x, t, fs)``, whose linear pre-interpolation and 1 % rate tolerance are not reproduced."""
        from fractions import Fraction
        from .resample import resample
        if (p is None) != (q is None):
            raise DasError("resample: give both p and q, or neither")
        if p is None:
            if not (fs > 0 and np.isfinite(fs)):
                raise DasError("resample: fs must be positive")
            fr = Fraction(float(fs) / float(self.fs)).limit_denominator(4096)
            p, q = fr.numerator, fr.denominator
            if p < 1 or abs(self.fs * p / q - fs) > 1e-9 * abs(fs):
                raise DasError(f"resample: fs / self.fs = {float(fs) / float(self.fs)!r} is no ratio p / q with q <= 4096 (the nearest, {p} / {q}, misses fs by more "
                               "than 1e-9): pass p and q explicitly")
        fr = Fraction(int(p), int(q))
        d = self._device_data("resample")
        ax = self.order.index("T")
        y = resample(d.movedim(ax, 0), fr.numerator, fr.denominator, n, beta)
        return ChannelData(y.movedim(0, ax), self.t0, self.fs * fr.numerator / fr.denominator, self.order)

    def filtfilt(self, b, dim=None, a=None, sos=None):
        """Zero-phase filtering along time with the real FIR taps ``b`` (reference ``src/ChannelData.m:890-909``: ``filtfilt(D, x)``; ``t0`` is unchanged) in
        ONE pass on the device (``qups_amd.resample.filtfilt``).  An IIR filter (``a`` or ``sos``) is not built and raises.  Any ``order`` is accepted and
        kept.  DEVIATION: the reference computes in double and casts back; this computes in the data's precision."""
        from .resample import filtfilt
        if a is not None or sos is not None:
            raise DasError("filtfilt: an IIR filter (a, sos) is not built -- only FIR taps b")
        ax = self.order.index("T") if dim is None else int(dim) - 1
        d = self._device_data("filtfilt")
        y = filtfilt(b, d.movedim(ax, 0))
        return ChannelData(y.movedim(0, ax), self.t0, self.fs, self.order)

    def fftfilt(self, b, dim=None):
        """``fftfilt(D, x)`` along time for the FIR taps ``b`` (reference ``src/ChannelData.m:910-934``), ``t0 -= (K - 1) / 2 / fs`` (``:931-933``).  For an FIR
        filter the result equals :meth:`filter`'s, so this routes there: ``qdas_convd`` already picks its FFT path for long filters."""
        return self.filter(b, dim)

    def getLowpassFilter(self, cutoff: float, N: int = 25):
        """``N + 1`` real taps of a low-pass FIR filter with cutoff ``cutoff`` [Hz] at this data's ``fs`` (reference ``src/ChannelData.m:833-856``:
        ``designfilt('lowpassfir', 'FilterOrder', N, 'CutoffFrequency', cutoff, 'DesignMethod', 'window')``) from ``scipy.signal.firwin`` with its
        Hamming window -- the window design ``designfilt`` documents.  There is no MATLAB to pin the taps against: the tests hold them to the closed
        form (Hamming-windowed sinc, unit gain at DC, symmetric taps)."""
        from .demod import lowpass_taps
        return lowpass_taps(cutoff, self.fs, N)

    def getPassbandFilter(self, bw, N: int = 25):
        """``N + 1`` real taps of a band-pass FIR filter between ``bw[0]`` and ``bw[-1]`` [Hz] (reference ``src/ChannelData.m:808-832``:
        ``designfilt('bandpassfir', ..., 'DesignMethod', 'window')``) from ``scipy.signal.firwin`` (Hamming window).  As for :meth:`getLowpassFilter` the
        tests hold the taps to the closed form: the difference of two windowed sincs, unit gain at the band centre, symmetric taps."""
        from .demod import passband_taps
        bw = np.asarray(bw, float).reshape(-1)
        return passband_taps((bw[0], bw[-1]), self.fs, N)

    def sample(self, tau, interp="linear", w=1, sdim=None, fmod=0.0, **kw):
        """``y = sample(chd, tau, interp, w, sdim, fmod)`` (reference ``src/ChannelData.m:1230-1336``): ``tau`` holds TIMES and
        broadcasts against ``T x N x M x F...`` in every dimension but the first; sample indices ``(tau - t0) * fs`` (``:1317``),
        upmix ``exp(2i pi fmod/fs * ntau)`` (``:1320``), then ``wsinterpd(data, ntau, 1, w, sdim, interp, 0, omega)`` (``:1327``)."""
        import torch
        chd = self.rectifyDims()
        as_t = lambda a: a if hasattr(a, "is_cuda") else torch.from_numpy(np.asarray(a, dtype=np.float64))
        tt = as_t(tau).to(torch.float64)
        t0 = as_t(np.asarray(chd.t0, dtype=np.float64)).to(tt.device)
        ntau = (tt - t0) * chd.fs
        return wsinterpd(chd.data, ntau, 1, w, sdim, interp, 0.0, 2j * np.pi * fmod / chd.fs, **kw)

    def rectifyt0(self, interp="cubic"):
        """one start time for all transmits (reference ``src/ChannelData.m:1205-1228``): traces are resampled onto the earliest
        ``t0``; the time axis grows by ``ceil(max(t0 - min t0) * fs)`` samples at zeropad and again in the sampling grid, as in
        the reference (``:1220-1222``)."""
        if np.size(self.t0) == 1:
            return self
        chd = self.rectifyDims()
        t0 = np.asarray(chd.t0, float)
        t0_ = float(t0.min())
        npad = int(np.ceil((t0 - t0_).max() * chd.fs))
        chd = chd.zeropad(0, npad)
        nd = max(chd._torch_data().ndim, t0.ndim)
        tau = t0_ + np.arange(chd.T + npad).reshape((-1,) + (1,) * (nd - 1)) / chd.fs
        return ChannelData(chd.sample(tau, interp), t0_, chd.fs, "TNM")


def _cat_tx(parts):
    import torch
    return parts[0] if len(parts) == 1 else torch.cat(parts, dim=4)


class UltrasoundSystem:
    def __init__(self, xdc: Transducer, seq: Sequence, scan: Scan, fs=None, rx: Transducer | None = None):
        self.tx, self.rx, self.seq, self.scan, self.fs = xdc, rx or xdc, seq, scan, fs
        self.xdc = xdc

    # ------------------------------------------------------------------------------------
    def _tx_geometry(self):
        """(Pv, Nv, options) by sequence type (reference src/UltrasoundSystem.m:3340-3352)"""
        t = self.seq.type
        if t == "FSA":
            return G.sequence_args("FSA", tx_pos=self.tx.positions(), tx_normals=self.tx.normals)
        if t == "PW":
            return G.sequence_args("PW", focus=self.seq.focus)
        if t in ("FC", "VS", "DV"):
            return G.sequence_args(t, focus=self.seq.focus, tx_offset=self.tx.offset)
        raise DasError(f"Unknown sequence type {t!r}.")

    # ---- receive-apodization generators (reference src/UltrasoundSystem.m:5165-5267, 5303-5429)
    def apAcceptanceAngle(self, theta=45.0):
        """materialised ``I1 x I2 x I3 x N x 1`` mask, reference ``:5303-5374``"""
        from . import apodization as A
        return A.ap_acceptance_angle(self.scan.positions(), self.rx.positions(), self.rx.normals, theta)

    def apCosineAngle(self, theta=45.0):
        """reference ``:5377-5429``"""
        from . import apodization as A
        return A.ap_cosine_angle(self.scan.positions(), self.rx.positions(), self.rx.normals, theta)

    def apApertureGrowth(self, f=1.5, Dmax=np.inf):
        """reference ``:5165-5267``"""
        from . import apodization as A
        return A.ap_aperture_growth(self.scan.positions(), self.rx.positions(), self.rx.normals, f, Dmax)

    def rx_apod(self, kind, **kw):
        """the same rules, GENERATED inside the beamforming kernel: ``us.DAS(chd, rx_apod=us.rx_apod('acceptance', theta=30))``"""
        from . import apodization as A
        return A.rx_apod_spec(kind, normals=self.rx.normals, **kw)

    @staticmethod
    def _chd_array(chd):
        """``(list of ChannelData, concatenation dimension | None)`` of an ND-array of ChannelData (reference ``src/UltrasoundSystem.m:3301-3305``,
        ``:4670-4672``): a single object, a numpy object array with at most one non-singleton dimension, or a list / tuple -- MATLAB's
        ``[chd1, chd2, ...]``, a 1 x K row.  The dimension is 0-based here (MATLAB's ``chddim - 1``): the images are concatenated along it."""
        if isinstance(chd, ChannelData):
            return [chd], None
        if isinstance(chd, (list, tuple)):
            arr = np.empty((1, len(chd)), dtype=object)
            for k, c in enumerate(chd):
                arr[0, k] = c
        else:
            arr = np.asarray(chd, dtype=object)
            if arr.ndim < 2:
                arr = arr.reshape(1, -1)                       # (MATLAB has no 1-D arrays: a vector is a row)
        items = list(arr.reshape(-1, order="F"))
        if not items or not all(isinstance(c, ChannelData) for c in items):
            raise DasError("chd must be a ChannelData or an array of ChannelData")
        dims = [d for d, n in enumerate(arr.shape) if n > 1]
        if len(dims) > 1:
            raise DasError("ChannelData array can only contain up to one non-scalar dimension.")     # (:3304)
        return items, (dims[0] if dims else None)

    def DAS(self, chd: ChannelData, *apods, c0=None, fmod=0.0, prec="single", device=-1, apod=1, interp="cubic",
            keep_tx=False, keep_rx=False, return_plan=False, kernel=0, rx_apod=None):
        """``b = DAS(us, chd, A1, ..., 'c0', c0, 'fmod', fc, 'interp', method, 'prec', type, 'keep_tx', tf, 'keep_rx', tf)``

        reference ``src/UltrasoundSystem.m:3172-3372``.  Output ``I1 x I2 x I3 x F... x [N] x [M]`` (``:3361``).  ``chd`` may be an array of
        ChannelData with one non-scalar dimension (``:3301-3305``): each is beamformed on its own (``:3325``) and the images are
        concatenated along that dimension (``:3368``); with ``return_plan`` the plan of the first element comes back (the reference's
        loop runs from the last element to the first and keeps the last call's kernel handle).
        """
        if prec not in ("single", "double", "halfT"):
            raise DasError("prec must be one of {'double', 'single', 'halfT'}")
        chds, chddim = self._chd_array(chd)
        if len(chds) > 1 or chddim is not None:
            import torch
            kw = dict(c0=c0, fmod=fmod, prec=prec, device=device, apod=apod, interp=interp, keep_tx=keep_tx, keep_rx=keep_rx, kernel=kernel, rx_apod=rx_apod)
            D = max([c.data.ndim for c in chds] + [0 if chddim is None else chddim + 1])        # max dimension of data (:3305)
            outs, plan = [], None
            for k, c in enumerate(chds):
                o = self.DAS(c, *apods, return_plan=(return_plan and k == 0), **kw)
                if return_plan and k == 0:
                    o, plan = o
                outs.append(o)
            nd = max(max(o.ndim for o in outs), (chddim or 0) + 1, D)
            outs = [o.reshape(tuple(o.shape) + (1,) * (nd - o.ndim)) for o in outs]
            b = outs[0] if chddim is None else torch.cat(outs, dim=chddim)
            return (b, plan) if return_plan else b
        chd = chds[0]
        c0 = self.seq.c0 if c0 is None else c0
        apods = list(apods) + ([] if (np.isscalar(apod) and apod == 1) else [apod])
        fun = {(True, True): "DAS", (True, False): "SYN", (False, True): "MUL", (False, False): "BF"}[(not keep_tx, not keep_rx)]   # :3318-3322
        if np.size(chd.t0) > 1 and np.asarray(chd.t0).reshape(-1).size != self._num_tx(chd):
            chd = chd.rectifyt0()                              # t0 varies outside the transmit dimension   (:3330)
        if chd.order[0] != "T" or chd.order[:3] not in ("TNM", "TMN"):
            chd = chd.rectifyDims()                            # time is not the first dimension             (:3333)
        Pv, Nv, opt = self._tx_geometry()
        ext = ["device", device, "input-precision", prec, "transpose", chd.order == "TMN", "interp", interp, "modulation", fmod]   # :3336-3338
        for a in apods:
            ext += ["apod", a]
        if rx_apod is not None:
            ext += ["rx-apod", rx_apod]
        out = das_spec(fun, self.scan.positions(), self.rx.positions(), Pv, Nv, chd.data, chd.t0, chd.fs, c0, *ext, *opt,
                       return_plan=return_plan, kernel=kernel)
        b, plan = out if return_plan else (out, None)
        nd = b.ndim
        b = b.permute(0, 1, 2, *range(5, nd), 3, 4)          # I1 x I2 x I3 x F... x [N] x [M]   (:3361)
        return (b, plan) if return_plan else b

    def greens(self, scat_pos, scat_amp, waveform, wv_t0, wv_fs, fs=None, R0=None, interp="cubic", focus=True):
        """``chd = greens(us, scat)`` (reference ``src/UltrasoundSystem.m:463-882``): full-synthetic-aperture channel data of point
        scatterers from the simulator kernel, then -- like the reference's last step (``:877``) -- ``focusTx`` synthesises this
        system's transmit sequence from it.  The transmit-receive waveform is an input (samples, start time, sampling frequency)."""
        import torch
        from .greens import greens as _greens
        fs = fs or self.fs
        y, t0 = _greens(self.rx.positions(), self.tx.positions(), scat_pos, scat_amp, self.seq.c0, waveform, wv_t0, wv_fs, fs,
                        R0=R0, interp=interp)
        chd = ChannelData(y.contiguous(), t0, fs, "TNM")
        return self.focusTx(chd, self.seq, interp=interp) if focus else chd

    def fdtdSim(self, c, rho=None, cgrd: Scan | None = None, *, waveform, wv_t0, wv_fs, rx_impulse=None, rx_t0=0.0, c0=None, rho0=None, T=None, PML=20,
                CFL_max=0.25, order=8, isosub=False, field=False, bsize=None, prec="single", ElemMapMethod="nearest", plan_only=False,
                alpha=None, alpha_power=1.01, alpha_band=None, mechanisms=3, BoA=None):
        """``chd = fdtdSim(us, c, rho, cgrd)``: channel data that travelled through the medium ``c``, ``rho`` (``Z x X`` on the Cartesian scan ``cgrd``, by
        default this system's scan), from a 2-D acoustic FDTD solver on the device (``qups_amd/fdtd.py`` -> ``qdas_fdtd``).  It follows the wrapper contract of
        the reference's ``kspaceFirstOrder`` (``src/UltrasoundSystem.m:2458-3170``) -- the time step from ``CFL_max`` as an integer fraction of ``1 / us.fs``
        (``:2714-2729``), the transmit table from the sequence's delays and apodization (``:2735-2741``), elements on their nearest nodes (``:2753-2768``),
        additive velocity sources along the element normals (``:2874-2878``), ``T`` defaulting to one round trip across the grid (``:2890``), ``t0``
        (``:2904``), ``isosub`` (``:2706-2712``), ``field`` (``:2471-2482``) -- but the method is FDTD of order ``order`` in space, NOT k-space pseudospectral:
        absolute amplitude and dispersion are this discretisation's and are not matched to k-Wave.

        The transmit waveform is an input (samples, start time, sampling frequency), as in :meth:`greens`; ``rx_impulse`` (samples at ``wv_fs`` starting at
        ``rx_t0``) is applied afterwards with ``convd`` in ``'full'`` shape (``:3069-3070``).  ``rho = None``: ``rho0`` everywhere, ``rho0 = c0 / 1.5`` (the
        reference's default medium, ``:2638``).  ``PML``: a size, or a range ``[lo, hi]``.  ``bsize``: pulses per solver call.  The record is ``T x N x V`` at
        ``fs_ = ratio us.fs``, as the reference returns it: the caller downsamples.  ``field=True``: the pressure of the whole interior grid per step,
        ``T x (Z X) x V`` (sensors = all nodes, ``Z`` slowest, no receive impulse), refused above 2 GiB.  ``plan_only``: the wrapper arithmetic alone, a dict
        (no device needed).  A ``cgrd`` with three non-singleton dimensions goes to the 3-D solver (``qups_amd/fdtd3.py`` -> ``qdas_fdtd3``): ``c``, ``rho`` of
        ``cgrd.size``, ``field`` as ``T x (Z X Y) x V``.

        ABSORPTION (2-D).  ``alpha``: a scalar or a map on ``cgrd`` in dB/(MHz^y cm), k-Wave's ``alpha_coeff`` -- ``1e4 Medium.alpha0``, the conversion of
        the reference's ``Medium.getMediumKWave`` (``src/Medium.m:443``) -- with ``alpha_power = y`` (``Medium.alpha_power``, default 1.01).  ``1 <= y < 2``:
        ``mechanisms <= 4`` relaxation mechanisms fitted to ``w^y`` over ``alpha_band`` (default ``(0.5 fc, 1.5 fc)`` of the transducer): a relaxation FDTD
        of the Fullwave kind, NOT k-Wave's fractional Laplacian; ``y = 2``: k-Wave's ``alpha_mode = 'stokes'``.  The time step respects the unrelaxed speed
        (``fdtd.loss_time_step``), and ``plan["loss"]["fit_err"]`` is the fit's largest relative deviation from the power law inside the band.
        ``alpha=None``: lossless, as before.  ``y`` outside ``[1, 2]`` or a negative ``alpha``: ``ValueError``; a volume with ``alpha``:
        ``NotImplementedError``.

        NONLINEARITY (2-D).  ``BoA``: a scalar or a map on ``cgrd`` of B/A (``Medium.BoA``, handed to k-Wave as ``BonA``, ``src/Medium.m:442-447``): k-Wave's
        nonlinear first-order equations (``qdas_fdtd_nonlinear``), ``beta = 1 + B/2A`` for a plane wave; it combines with ``alpha``.  THE WAVEFORM IS IN m/s
        then -- the particle velocity at the elements' faces -- and its size matters; ``plan["nl"]`` reports ``beta_max`` and ``mach``, the source Mach number
        ``max|s| (2 c_max dt / h) / c_min`` of the transmit table.  The time step is the linear one.  There is no shock capturing: without absorption a wave
        that reaches the shock distance (``sigma = 1``) rings at the grid scale.  ``BoA=None`` or all NaN: linear, as before (the reference drops the field
        only when every value is NaN); ``BoA = 0`` is still nonlinear (``beta = 1``); a partly NaN map, a negative or an infinite value: ``ValueError``; a
        volume with ``BoA``: ``NotImplementedError``.  Not built: absorption and nonlinearity in 3-D, shock capturing, a per-node ``alpha_power``, ``'linear'`` and ``karray-*`` element mapping,
        sensor directivity."""
        from . import fdtd as F
        if ElemMapMethod != "nearest":
            if ElemMapMethod in ("linear", "karray-direct", "karray-depend"):
                raise NotImplementedError(f"fdtdSim: ElemMapMethod '{ElemMapMethod}' is not built; only 'nearest' is")
            raise DasError(f"fdtdSim: unknown ElemMapMethod {ElemMapMethod!r}")
        if prec not in ("single", "double"):
            raise DasError("fdtdSim: prec must be 'single' or 'double'")
        cgrd = cgrd or self.scan
        if cgrd.axes is None or cgrd.axes.get("kind") != "cartesian":
            raise DasError("fdtdSim: cgrd must be a Cartesian scan made by Scan.cartesian (order 'ZXY').")
        if sum(int(v) > 1 for v in tuple(cgrd.size)) == 3:           # three non-singleton dimensions -> the 3-D solver (reference :2929-2948), as in bfEikonal
            if alpha is not None:
                raise NotImplementedError("fdtdSim: absorption is built for the 2-D solver only; a volume takes alpha=None")
            if BoA is not None:
                raise NotImplementedError("fdtdSim: nonlinearity is built for the 2-D solver only; a volume takes BoA=None")
            return self._fdtdSim3(c, rho, cgrd, waveform=waveform, wv_t0=wv_t0, wv_fs=wv_fs, rx_impulse=rx_impulse, rx_t0=rx_t0, c0=c0, rho0=rho0, T=T, PML=PML,
                                  CFL_max=CFL_max, order=order, isosub=isosub, field=field, bsize=bsize, prec=prec, plan_only=plan_only)
        z, x = cgrd.axes["z"], cgrd.axes["x"]
        h = F.grid_spacing(z, x, cgrd.axes["y"])
        Z, X = z.size, x.size
        c0 = float(self.seq.c0 if c0 is None else c0)
        rho0 = float(c0 / 1.5 if rho0 is None else rho0)
        c = np.asarray(c.detach().cpu().numpy() if hasattr(c, "detach") else c, np.float64).reshape(Z, X) if np.size(c) == Z * X else None
        if c is None:
            raise DasError(f"fdtdSim: c must have the grid's size Z x X = {Z} x {X}")
        if rho is None:
            rho = np.full((Z, X), rho0)
        rho = np.asarray(rho.detach().cpu().numpy() if hasattr(rho, "detach") else rho, np.float64)
        if rho.size != Z * X:
            raise DasError(f"fdtdSim: rho must have the grid's size Z x X = {Z} x {X}")
        rho = rho.reshape(Z, X)
        if self.fs is None:
            raise DasError("fdtdSim: the system needs a sampling frequency fs")
        loss = None
        if alpha is None:
            ratio, fs_, dt = F.time_step(self.fs, c.max(), h, CFL_max, order)
        else:
            if alpha_band is None:
                alpha_band = (0.5 * float(self.xdc.fc), 1.5 * float(self.xdc.fc))
            ratio, fs_, dt, loss = F.loss_time_step(self.fs, c, alpha, alpha_power, alpha_band, h, CFL_max, order, mechanisms)
        s, txn0, txne = F.tx_table(waveform, wv_t0, wv_fs, self.seq.delays(self.tx), self.seq.apodization(self.tx), fs_)
        if T is None:
            T = 2.0 * math.hypot(z[-1] - z[0], x[-1] - x[0]) / c0
        Nt = 1 + int(math.floor((float(T) + (txne - txn0) / fs_) * fs_ + 1e-9))
        P = F.pml_size(PML, Z, X)
        rx_t0 = float(rx_t0) if (rx_impulse is not None and not field) else 0.0
        plan = dict(h=h, ratio=ratio, fs_=fs_, dt=dt, txn0=txn0, txne=txne, Nt=Nt, t0=txn0 / fs_ + rx_t0, P=P, Nz=Z + 2 * P, Nx=X + 2 * P, T=float(T),
                    rho=rho, rho_iso=F.iso_density(c, c0, rho0) if isosub else None)
        lkw = {}
        if loss is not None:
            plan["loss"] = loss
            lkw = dict(alpha=alpha, alpha_power=alpha_power, alpha_band=alpha_band, mechanisms=mechanisms)
        nl = F.nl_model(rho, BoA)
        if nl is not None:
            plan["nl"] = dict(beta_max=nl["beta_max"], mach=F.source_mach(s, c, dt, h), bq=nl["bq"])
            lkw["BoA"] = BoA
        nrm = np.stack([self.tx.normals[2], self.tx.normals[0]])
        V = s.shape[2]
        if field:
            sen, sen_nodes = np.zeros((2, 0)), tuple(np.indices((Z, X)).reshape(2, -1))      # every node, Z slowest: no search
            if Nt * Z * X * V * (4 if prec == "single" else 8) > 2 ** 31:
                raise DasError(f"fdtdSim: field=True would return {Nt} x {Z * X} x {V} values, above 2 GiB; shorten T or coarsen the grid")
        else:
            sen, sen_nodes = self.rx.positions(), None
        siz, six = F.nearest_nodes(z, x, self.tx.positions())           # (raises the reference's assertion before any device work)
        plan.update(src_nodes=(siz, six), sen_nodes=F.nearest_nodes(z, x, sen) if not field else None)
        if plan_only:
            return plan
        run = lambda r: F.fdtd(c, r, z, x, self.tx.positions(), nrm, s, sen, Nt, dt, PML=P, order=order, prec=prec, bsize=bsize, sen_nodes=sen_nodes, **lkw)
        y = run(rho)
        if isosub:
            y = y - run(plan["rho_iso"])
        if rx_impulse is not None and not field:
            import torch
            from .convd import convd
            w = np.asarray(rx_impulse, np.float64).reshape(-1)
            nr = int(math.floor((w.size - 1) / wv_fs * fs_ + 1e-9)) + 1
            taps = F._sample_cubic(w, np.arange(nr) / fs_ * wv_fs)
            y = convd(y, torch.from_numpy(taps).to(device=y.device, dtype=y.dtype).reshape(-1, 1, 1), 1, "full")
        return ChannelData(y, plan["t0"], fs_, "TNM")

    def _fdtdSim3(self, c, rho, cgrd, *, waveform, wv_t0, wv_fs, rx_impulse, rx_t0, c0, rho0, T, PML, CFL_max, order, isosub, field, bsize, prec, plan_only):
        """:meth:`fdtdSim` on a volume: ``c``, ``rho`` of ``cgrd.size = Z x X x Y``, through ``qups_amd/fdtd3.py`` -> ``qdas_fdtd3``.  The same wrapper contract
        with three axes: the normals from all three rows of ``tx.normals`` (``ux``, ``uy``, ``uz``, ``:2874-2878``), ``T`` defaulting to
        ``2 |(dx, dy, dz)| / c0`` (``:2890``), ``field=True`` as ``T x (Z X Y) x V`` with the nodes in C order of ``(Z, X, Y)``."""
        from . import fdtd as F
        from . import fdtd3 as F3
        z, x, y = cgrd.axes["z"], cgrd.axes["x"], cgrd.axes["y"]
        h = F3.grid_spacing3(z, x, y)
        Z, X, Y = z.size, x.size, y.size
        c0 = float(self.seq.c0 if c0 is None else c0)
        rho0 = float(c0 / 1.5 if rho0 is None else rho0)
        c = F3._host(c)
        if c.size != Z * X * Y:
            raise DasError(f"fdtdSim: c must have the grid's size Z x X x Y = {Z} x {X} x {Y}")
        c = c.reshape(Z, X, Y)
        rho = np.full((Z, X, Y), rho0) if rho is None else F3._host(rho)
        if rho.size != Z * X * Y:
            raise DasError(f"fdtdSim: rho must have the grid's size Z x X x Y = {Z} x {X} x {Y}")
        rho = rho.reshape(Z, X, Y)
        if self.fs is None:
            raise DasError("fdtdSim: the system needs a sampling frequency fs")
        ratio, fs_, dt = F.time_step(self.fs, c.max(), h, CFL_max, order)
        F3._check_step(c.max(), dt, h, int(order) // 2)
        s, txn0, txne = F.tx_table(waveform, wv_t0, wv_fs, self.seq.delays(self.tx), self.seq.apodization(self.tx), fs_)
        if T is None:
            T = 2.0 * math.sqrt((x[-1] - x[0]) ** 2 + (y[-1] - y[0]) ** 2 + (z[-1] - z[0]) ** 2) / c0
        Nt = 1 + int(math.floor((float(T) + (txne - txn0) / fs_) * fs_ + 1e-9))
        P = F.pml_size(PML, Z, X, Y)
        rx_t0 = float(rx_t0) if (rx_impulse is not None and not field) else 0.0
        plan = dict(h=h, ratio=ratio, fs_=fs_, dt=dt, txn0=txn0, txne=txne, Nt=Nt, t0=txn0 / fs_ + rx_t0, P=P, Nz=Z + 2 * P, Nx=X + 2 * P, Ny=Y + 2 * P,
                    T=float(T), rho=rho, rho_iso=F.iso_density(c, c0, rho0) if isosub else None)
        nrm = np.stack([self.tx.normals[2], self.tx.normals[0], self.tx.normals[1]])
        V = s.shape[2]
        if field:
            sen, sen_nodes = np.zeros((3, 0)), tuple(np.indices((Z, X, Y)).reshape(3, -1))   # every node, C order of (Z, X, Y): no search
            if Nt * Z * X * Y * V * (4 if prec == "single" else 8) > 2 ** 31:
                raise DasError(f"fdtdSim: field=True would return {Nt} x {Z * X * Y} x {V} values, above 2 GiB; shorten T or coarsen the grid")
        else:
            sen, sen_nodes = self.rx.positions(), None
        src_nodes = F3.nearest_nodes3(z, x, y, self.tx.positions())       # (raises the reference's assertion before any device work)
        plan.update(src_nodes=src_nodes, sen_nodes=F3.nearest_nodes3(z, x, y, sen) if not field else None)
        if plan_only:
            return plan
        run = lambda r: F3.fdtd3(c, r, z, x, y, self.tx.positions(), nrm, s, sen, Nt, dt, PML=P, order=order, prec=prec, bsize=bsize, sen_nodes=sen_nodes)
        yd = run(rho)
        if isosub:
            yd = yd - run(plan["rho_iso"])
        if rx_impulse is not None and not field:
            import torch
            from .convd import convd
            w = np.asarray(rx_impulse, np.float64).reshape(-1)
            nr = int(math.floor((w.size - 1) / wv_fs * fs_ + 1e-9)) + 1
            taps = F._sample_cubic(w, np.arange(nr) / fs_ * wv_fs)
            yd = convd(yd, torch.from_numpy(taps).to(device=yd.device, dtype=yd.dtype).reshape(-1, 1, 1), 1, "full")
        return ChannelData(yd, plan["t0"], fs_, "TNM")

    def _num_tx(self, chd):
        return int(chd.data.shape[chd.order.index("M")])

    def focusTx(self, chd: ChannelData, seq: Sequence | None = None, interp="cubic", buffer=0):
        """``chd = focusTx(us, chd, seq)`` (reference ``src/UltrasoundSystem.m:3374-3503``): synthesise the transmits of ``seq`` from
        full-synthetic-aperture data by delaying and summing over the transmit elements,
        ``z[t', n, m'] = sum_m apd[m, m'] * x(time[t'] - tau[m, m'], n, m)`` with ``tau = -seq.delays(tx)`` shifted so that all delays
        are non-negative (``:3457-3470``; the reference samples with ``sample2sep`` at ``:3498``)."""
        import torch
        from .interpd import das_lut
        seq = seq or self.seq
        chd = chd.rectifyDims()
        tau = -np.asarray(seq.delays(self.tx), float)            # M x M'
        apd = np.broadcast_to(np.asarray(seq.apodization(self.tx), float), tau.shape)
        if seq.type == "FSA" and not np.count_nonzero(tau) and np.array_equal(apd, np.eye(self.tx.numel)):
            return chd                                             # already FSA (:3461)
        i = apd != 0
        nmin = int(np.floor(np.nanmin(tau[i]) * chd.fs))
        nmax = int(np.ceil(np.nanmax(tau[i]) * chd.fs))
        t0 = float(np.asarray(chd.t0).reshape(-1)[0]) + nmin / chd.fs
        tau = tau - nmin / chd.fs
        pad = (nmax - nmin) + int(buffer)
        d = chd._torch_data()
        if d.dtype in (torch.float32, torch.float64, torch.complex64, torch.complex128):
            # the positions are the record's own time grid plus ONE offset per (element, synthesised transmit): the shift-and-sum kernel
            # (qdas_shift_sum: per-pair tap offset and weights, LDS-staged windows, zero weights skipped; round 3).  The zeros the reference appends
            # (chd = zeropad(chd, 0, nmax - nmin + buffer), :3479) are not stored: `tpad` makes the kernel read them as in-range zeros (round 6)
            from .interpd import shift_sum
            dev = d.device if d.is_cuda else torch.device("cuda")
            z = shift_sum(d.to(dev), -tau * chd.fs, apd, interp, tpad=pad)
            return ChannelData(z, t0, chd.fs, "TNM")
        chd = ChannelData(chd.data, t0, chd.fs, "TNM").zeropad(0, pad)
        d = chd._torch_data()
        T2, N, M = d.shape[:3]
        dev = d.device if d.is_cuda else torch.device("cuda")
        Mp = tau.shape[1]
        # other data types: ONE launch of the general single-delay kernel over the index space (t', n, m, m', frames...): the sample index depends
        # on (t', m, m'), the data on (n, m, frames), the weight on (m, m'); the transmit elements m are summed
        ntau = torch.arange(T2, dtype=torch.float64, device=dev).reshape(T2, 1, 1, 1) - torch.from_numpy(tau * chd.fs).to(dev).reshape(1, 1, M, Mp)
        xd = d.to(dev).reshape((T2, N, M, 1) + tuple(d.shape[3:]))
        z = wsinterpd(xd, ntau, 1, apd.reshape(1, 1, M, Mp), [3], interp, 0.0)        # T' x N x 1 x M' x F...
        z = z.reshape((T2, N, Mp) + tuple(d.shape[3:]))
        return ChannelData(z, t0, chd.fs, "TNM")

    def refocus(self, chd: ChannelData, seq: Sequence | None = None, gamma=None, method="tikhonov"):
        """``[chd, Hi] = refocus(us, chd, seq, 'gamma', gamma, 'method', method)`` (reference ``src/UltrasoundSystem.m:3505-3768``): the inverse of
        ``focusTx`` -- data recorded with the ``V`` pulses of ``seq`` (default ``us.seq``) back to the full-synthetic-aperture data of the ``M`` transmit
        elements, by a per-frequency decoding matrix.  ``method``: ``'tikhonov'`` (default; ``gamma`` defaults to ``10 (chd.N / 10)^2`` and is scaled by the
        largest singular value per frequency), ``'adjoint'`` (enough for plane waves and orthogonal codes) or ``'pinv'`` (not recommended).  Returns the
        ``ChannelData`` (``T x N x M x frames...`` complex, ``t0 = min(chd.t0)``) and ``Hi`` (``M x V x T`` complex128, host).  The formulas are in
        ``qups_amd/refocus.py``; the decoder of the last ``(delays, apodization, T, fs, method, gamma)`` is kept, so a stream of frames builds it once.

        Zero-pad first.  A focused sequence has t = 0 at each focus, FSA data at each transmitting element, so the recovered echoes move in time while
        the time axis stays as it is; and since the decoding works on the record's spectrum, whatever moves past either end of the record wraps around
        to the other.  The record must therefore already span the times the FSA echoes will occupy: if they reach 40 us and ``chd`` ends at 20 us,
        ``chd.zeropad(0, ceil(fs * 20e-6))`` before the call."""
        import torch
        from . import refocus as RF
        if not isinstance(chd, ChannelData):
            raise DasError("refocus: chd must be one ChannelData")
        if method not in RF.METHODS:
            raise DasError(f"refocus: method must be one of {RF.METHODS}, got {method!r}")
        seq = seq or self.seq
        chd = chd.rectifyDims()
        x = chd._torch_data()
        if x.ndim < 3:
            x = x.reshape(tuple(x.shape) + (1,) * (3 - x.ndim))
        T, N, V = (int(v) for v in x.shape[:3])
        tau = np.asarray(seq.delays(self.tx), float)               # M x V
        apd = np.broadcast_to(np.asarray(seq.apodization(self.tx), float), tau.shape)
        if tau.shape[1] != V:
            raise DasError(f"Number of transmits ({V}) must match the sequence's delays ({tau.shape[0]} x {tau.shape[1]}).")
        gamma = RF.default_gamma(N) if gamma is None else float(gamma)
        if not gamma >= 0:
            raise DasError("refocus: gamma must be non-negative")
        if not x.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("qups_amd: no HIP device visible -- refocus has no CPU fallback")
            x = x.cuda()
        key = (tau.shape, tau.tobytes(), apd.tobytes(), T, float(chd.fs), method, gamma if method == "tikhonov" else None)
        kept = getattr(self, "_refocus_decoder", None)
        if kept is None or kept[0] != key:
            # the Decoder this replaces may still be read by a call queued on another stream: every use of its device copy has recorded the
            # stream that reads it (Decoder.on), so the allocator holds the block back until those calls have passed
            kept = (key, RF.Decoder(RF.decoder(tau, apd, T, chd.fs, method, gamma)))
            self._refocus_decoder = kept
        y, t0, Hi = RF.refocus(x, np.asarray(chd.t0, float).reshape(-1), chd.fs, decoder=kept[1])
        return ChannelData(y, t0, chd.fs, "TNM"), Hi

    # ------------------------------------------------------------------------------------
    def delay_tables(self, c0=None, device=None):
        """``tau_rx (I1 x I2 x I3 x N)``, ``tau_tx (I1 x I2 x I3 x M)`` as ``bfDAS`` computes them
        (reference ``src/UltrasoundSystem.m:4429-4463``): ``dr/c0`` and ``dv/c0`` with the per-type sign rule.  numpy arrays, or --
        with ``device`` -- float64 torch tensors computed there (the tables of a 1024 x 1024 image over 256 elements are 2 x 2 GB)."""
        c0 = self.seq.c0 if c0 is None else c0
        Pi, Pr = self.scan.positions(), self.rx.positions()
        Pv, Nv, _ = self._tx_geometry()
        M = max(Pv.shape[1], Nv.shape[1])
        Pv = np.broadcast_to(Pv, (3, M)) if Pv.shape[1] == 1 else Pv
        Nv = np.broadcast_to(Nv, (3, M)) if Nv.shape[1] == 1 else Nv
        if device is not None:
            import torch
            tt = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=device)
            Pi_t, Pr_t, Pv_t, Nv_t = tt(Pi), tt(Pr), tt(Pv), tt(Nv)
            e = lambda P: P[:, None, None, None, :]
            ct = tt(np.asarray(c0, float))
            ct = ct.reshape(tuple(ct.shape) + (1,) * (4 - ct.ndim)) if ct.ndim else ct
            # blocks of elements whose 3 x I x block temporary stays below ~256 MB: a handful of launches instead of one per element
            I = int(np.prod(Pi_t.shape[1:]))
            nb = max(1, (1 << 25) // max(3 * I, 1))
            ex = lambda P, a, b: P[:, None, None, None, a:b]
            tau_rx = torch.cat([torch.linalg.norm(Pi_t[..., None] - ex(Pr_t, a, min(a + nb, Pr_t.shape[1])), dim=0)
                                for a in range(0, Pr_t.shape[1], nb)], -1) / ct
            cols = []
            for a in range(0, M, nb):
                rv = Pi_t[..., None] - ex(Pv_t, a, min(a + nb, M))
                if self.seq.type in ("DV", "FSA"):
                    cols.append(torch.linalg.norm(rv, dim=0))
                elif self.seq.type in ("VS", "FC"):
                    cols.append(torch.linalg.norm(rv, dim=0) * torch.sign((rv * ex(Nv_t, a, min(a + nb, M))).sum(0)))
                else:
                    cols.append((rv * ex(Nv_t, a, min(a + nb, M))).sum(0))
            return tau_rx, torch.cat(cols, -1) / ct
        dr = np.linalg.norm(Pi[..., None] - Pr[:, None, None, None, :], axis=0)
        rv = Pi[..., None] - Pv[:, None, None, None, :]
        t = self.seq.type
        if t in ("DV", "FSA"):
            dv = np.linalg.norm(rv, axis=0)
        elif t in ("VS", "FC"):
            dv = np.linalg.norm(rv, axis=0) * np.sign((rv * Nv[:, None, None, None, :]).sum(0))
        else:
            dv = (rv * Nv[:, None, None, None, :]).sum(0)
        c = np.asarray(c0, float)
        c = c.reshape(c.shape + (1,) * (4 - c.ndim)) if c.ndim else c
        return dr / c, dv / c

    def bfDAS(self, chd: ChannelData, *apods, c0=None, apod=1, fmod=0.0, interp="cubic", keep_tx=False, keep_rx=False,
              prec=None, bsize=None):
        """``b = bfDAS(us, chd, ...)`` (reference ``src/UltrasoundSystem.m:4334-4474``): delay tables + ``bfDASLUT``."""
        import torch
        first = self._chd_array(chd)[0][0]                 # (an array of ChannelData: the tables serve every element, :4429-4463)
        dev = (first.data.device if hasattr(first.data, "is_cuda") and first.data.is_cuda else "cuda") if torch.cuda.is_available() else None
        tau_rx, tau_tx = self.delay_tables(c0, device=dev)
        return self.bfDASLUT(chd, tau_rx, tau_tx, *apods, apod=apod, fmod=fmod, interp=interp, keep_tx=keep_tx, keep_rx=keep_rx, prec=prec, bsize=bsize)

    def bfEikonal(self, chd, c, cgrd=None, *apods, fmod=0.0, interp="cubic", apod=1, keep_rx=False, keep_tx=False, bsize=None,
                  delay_only=False, prec=None, return_delays=False):
        """``[b, tau_rx, tau_tx] = bfEikonal(us, chd, med, cgrd, ...)`` (reference ``src/UltrasoundSystem.m:4204-4331``): delay-and-sum with
        travel times through the sound-speed map ``c``, an array of ``cgrd.size`` (a scalar: homogeneous; there is no ``Medium`` class here).
        ``cgrd`` defaults to ``us.scan`` and must be a Cartesian scan with equal steps in its non-singleton dimensions: two of them (``msfm2d``), or
        three -- a volume, solved by ``qups_amd.eikonal.eikonal3`` (``msfm3d``; with a matrix array that is aberration-corrected volumetric imaging).

        One travel-time map per element is solved on the device (``qups_amd.eikonal``; the reference: one ``msfm`` call per element, ``:4295-4308``)
        from the element's position floored to a grid node, sampled at the pixels of ``us.scan`` by cubic convolution (NaN outside ``cgrd``; such
        pixels add nothing to the image), and handed to :meth:`bfDASLUT` without leaving the device.  The transmit tables are the receive tables
        when ``us.tx is us.rx`` or the positions are equal (``:4300``).  Returns ``b``.  The reference's ``[b, tau_rx, tau_tx] = ...`` is asked for with
        ``return_delays=True`` (Python has no ``nargout``); ``delay_only=True`` implies it and skips the image (``b`` is then empty, ``:4324``):
        ``(b, tau_rx, tau_tx)`` with ``tau_rx`` ``I1 x I2 x I3 x N`` and ``tau_tx`` ``I1 x I2 x I3 x 1 x M``."""
        import torch
        from . import eikonal as E
        cgrd = self.scan if cgrd is None else cgrd
        chds = []
        if not delay_only:
            chds, _ = self._chd_array(chd)
            if not all(int(x.data.shape[x.order.index("M")]) == self.tx.numel for x in chds):       # (:4244-4245)
                raise DasError("Number of transmits must match number of transmitter elements.")
            if not all(int(x.data.shape[x.order.index("N")]) == self.rx.numel for x in chds):
                raise DasError("Number of receives must match number of receiver elements.")
        volume = sum(int(v) > 1 for v in tuple(cgrd.size)) == 3                                     # (:4251, :4261-4267: three non-singleton dimensions -> msfm3d)
        og, dp, dims, axes, csz = E.scan_grid3(cgrd) if volume else E.scan_grid(cgrd)
        tables = E.travel_time_tables3 if volume else E.travel_time_tables
        if np.ndim(c) == 0:
            cmap = np.full(csz, float(c))
        else:
            if not hasattr(c, "shape"):
                c = np.asarray(c, dtype=np.float64)
            if tuple(int(v) for v in c.shape) != tuple(cgrd.size):
                raise DasError(f"bfEikonal: the sound speed must be a scalar or an array of the grid's size {tuple(cgrd.size)}")
            cmap = c.reshape(csz)
        Prc = E.grid_coordinates(self.rx.positions(), og, dp, axes)                                 # (:4283-4284)
        reuse = E.same_aperture(self)
        Pvc = Prc if reuse else E.grid_coordinates(self.tx.positions(), og, dp, axes)
        Isz = self.scan.size
        Pi = np.asarray(self.scan.positions(), float).reshape(3, -1, order="F")                     # pixels in memory order: I1 fastest
        Pic = E.grid_coordinates(Pi, og, dp, axes)
        first = chds[0] if chds else None
        dev = first.data.device if first is not None and hasattr(first.data, "is_cuda") and first.data.is_cuda else None
        if dev is None and hasattr(c, "is_cuda") and c.is_cuda:
            dev = c.device
        tau_rx = tables(cmap, dp, Prc, Pic, Isz, device=dev)
        tau_tx = tau_rx if reuse else tables(cmap, dp, Pvc, Pic, Isz, device=dev)
        if delay_only:
            b = torch.zeros(tuple(Isz) + (self.rx.numel if keep_rx else 1, self.tx.numel if keep_tx else 1, 0), device=tau_rx.device)   # (:4324)
            return b, tau_rx, tau_tx.unsqueeze(3)
        b = self.bfDASLUT(chd, tau_rx, tau_tx, *apods, apod=apod, fmod=fmod, interp=interp, keep_tx=keep_tx, keep_rx=keep_rx, prec=prec, bsize=bsize)
        return (b, tau_rx, tau_tx.unsqueeze(3)) if return_delays else b

    def bfAdjoint(self, chd: ChannelData, *apods, c0=None, fmod=0.0, fthresh=-np.inf, apod=1, Nfft=None, keep_tx=False, keep_rx=False,
                  bsize=None, verbose=False, return_delays=False, return_bins=False):
        """``b = bfAdjoint(us, chd, A1, ..., 'c0', c0, 'fmod', fc, 'fthresh', thresh, 'Nfft', K, 'keep_tx', tf, 'keep_rx', tf)`` (reference
        ``src/UltrasoundSystem.m:3770-4050``): the inner product of the normalised transmitted wave with the received data, in the frequency domain.
        Output ``I1 x I2 x I3 x F... x [N] x [V]``.

        The spectrum, the frequency selection (``fthresh``: bins where no trace is within ``fthresh`` dB of its own maximum are dropped; bins at or
        above ``fs / 2`` always) and the routing of the apodization arrays run in torch on the data's device; the reference's loop over frequency
        blocks is one ``qdas_adjoint`` call per frame (``qups_amd.adjoint``, f32 matrix cores).  ``c0``: a scalar or ``I1 x I2 x I3``.

        ``Nfft``: the frequencies are ``f_k = k fs / Nfft`` throughout.  (The reference builds its phase ramps on the data's own frequency axis, of
        length ``T``, and takes the step from ``Nfft``: it only runs for ``Nfft == T``.)  ``Nfft >= T`` zero-pads; ``Nfft < T`` raises.
        Only complex64 data is supported (the reference itself warns that half precision is insufficient; there is no fp64 path).
        ``bsize`` and ``verbose`` are accepted for signature compatibility: no phasor block is ever stored, so there is nothing to bound.
        ``return_delays=True`` returns ``(b, tau_rx, tau_tx, tau_foc)`` as the reference's extra outputs: ``tau_rx`` ``I1 x I2 x I3 x N``, ``tau_tx``
        ``I1 x I2 x I3 x 1 x M`` (element to pixel), ``tau_foc = delays(seq, tx) + t0Offset`` (``M x V``).
        ``return_bins=True`` appends the ascending 0-based list of the frequency bins that were evaluated to whatever is returned."""
        import torch
        from . import adjoint as A
        if not isinstance(chd, ChannelData):
            raise DasError("bfAdjoint: chd must be one ChannelData")
        chd = chd.rectifyDims()
        x = chd._torch_data()
        if x.dtype != torch.complex64:
            raise DasError(f"bfAdjoint: complex64 data only, got {str(x.dtype).replace('torch.', '')} (half precision is insufficient for "
                           "frequency-domain beamforming; there is no double precision path; real data: hilbert first)")
        if x.ndim < 3:
            x = x.reshape(tuple(x.shape) + (1,) * (3 - x.ndim))
        T, N, V = (int(v) for v in x.shape[:3])
        M = self.tx.numel
        if Nfft is not None and int(Nfft) < T:
            raise DasError(f"bfAdjoint: Nfft ({int(Nfft)}) must be at least the number of samples ({T})")
        if N != self.rx.numel:
            raise DasError("Number of receives must match number of receiver elements.")
        del_tx = np.asarray(self.seq.delays(self.tx), float)
        if del_tx.shape != (M, V):
            raise DasError(f"Number of transmits ({V}) must match the sequence's delays ({del_tx.shape[0]} x {del_tx.shape[1]}).")
        apod_tx = np.broadcast_to(np.asarray(self.seq.apodization(self.tx), float), (M, V))
        t0off = np.broadcast_to(np.asarray(self.seq.t0Offset(), float).reshape(-1), (V,))
        t0 = np.asarray(chd.t0, float).reshape(-1)
        if t0.size not in (1, V):
            raise DasError("bfAdjoint: t0 must be a scalar or one value per transmit")
        tau_foc = del_tx + t0off[None, :]
        Isz = tuple(self.scan.size)
        I = int(np.prod(Isz))
        c0 = self.seq.c0 if c0 is None else c0
        cv = np.asarray(c0.cpu() if hasattr(c0, "cpu") else c0, float)
        if cv.size != 1 and tuple(cv.shape) + (1,) * (3 - cv.ndim) != Isz:
            raise DasError(f"bfAdjoint: c0 must be a scalar or an array of the scan's size {Isz}")
        cinv = 1.0 / cv.reshape(-1, order="F")
        a_n, a_m, a_mn = A.classify_apods(([] if (np.isscalar(apod) and apod == 1) else [apod]) + list(apods), Isz, N, V)
        if not x.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("qups_amd: no HIP device visible -- the adjoint beamformer has no CPU fallback")
            x = x.cuda()
        dev = x.device
        Fsz = tuple(int(v) for v in x.shape[3:])
        xf = x.reshape(T, N, V, -1)
        amn = None if a_mn is None else torch.from_numpy(np.array(a_mn)).to(dev, torch.float32).reshape(1, N, V)
        # one spectrum per frame (K x N x V each): a frame's numbers do not depend on its neighbours
        Xf = [A.spectrum(xf[..., f].contiguous(), t0, chd.fs, fmod, Nfft, t0off) for f in range(xf.shape[3])]
        K = T if Nfft is None else int(Nfft)
        ksel = A.select_bins(torch.stack(Xf, 3), chd.fs, fthresh) if Xf else np.zeros(0, np.int64)   # (one list for all frames, on the un-apodized spectrum, :3935-3938)
        if amn is not None:
            Xf = [X * amn for X in Xf]                         # a_mn is applied to the data (:4022)
        freq = ksel.astype(np.float64) * (chd.fs / K)
        kidx = torch.from_numpy(ksel).to(dev)
        Pi = np.asarray(self.scan.positions(), float).reshape((3, I), order="F")                   # pixels in memory order: I1 fastest
        Pr, Pt = np.asarray(self.rx.positions(), float), np.asarray(self.tx.positions(), float)
        flat = lambda a, n: None if a is None else np.asarray(a, float).reshape((I, n), order="F")
        an, am = flat(a_n, N), flat(a_m, V)
        Nn, Vv = (N if keep_rx else 1), (V if keep_tx else 1)
        frames = []
        for X in Xf:                                                           # one call per frame; the pixel index is column-major (I1 fastest)
            bf = A.adjoint(X[kidx].permute(0, 2, 1), freq, Pi, Pr, Pt, cinv, tau_foc, apod_tx, an, am, keep_rx=keep_rx, keep_tx=keep_tx)
            frames.append(bf.reshape(Isz[::-1] + (Nn, Vv)).permute(2, 1, 0, 3, 4))
        b = torch.stack(frames, 3).reshape(Isz + Fsz + (Nn, Vv)) if frames else torch.zeros(Isz + Fsz + (Nn, Vv), dtype=torch.complex64, device=dev)
        if not return_delays:
            return (b, ksel) if return_bins else b
        tt = lambda a: torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float64, device=dev)
        Pg = tt(self.scan.positions())
        ct = tt(cv if cv.size == 1 else cv.reshape(Isz)).reshape(Isz + (1,) if cv.size != 1 else (1, 1, 1, 1))
        tau = lambda P: torch.linalg.norm(Pg[..., None] - tt(P)[:, None, None, None, :], dim=0) / ct
        out = (b, tau(Pr), tau(Pt).unsqueeze(3), tau_foc)
        return out + (ksel,) if return_bins else out

    def bfMigration(self, chd: ChannelData, Nfft=None, c0=None, fmod=0.0, keep_tx=False, interp="cubic", jacobian=True, bsize=None):
        """``[b, bscan] = bfMigration(us, chd, [F, K], 'c0', c0, 'fmod', fc, 'keep_tx', tf, 'interp', method, 'jacobian', tf, 'bsize', B)`` (reference
        ``src/UltrasoundSystem.m:4675-4887``): plane-wave Stolt f-k migration.  ``b`` is ``min(T,F) x min(N,K) x [M] x frames...`` complex64 on the
        data's device; ``bscan`` is the ``Scan.cartesian`` it is defined on: ``x = x0 + pitch (0 : N'-1)``, ``z = offset_z + z(1) + mean(diff(z)) (0 : T'-1)``
        with ``z = c0 / 2 (t0 + (0 : F-1) / fs)`` -- the reference's regularised axis.

        Both are ALWAYS returned.  The reference's resampling of ``b`` onto ``us.scan`` when only one output is requested is deliberately not built:
        it is an ``interp2`` of a complex image, which the reference itself warns against ("Resampling a complex image can produce artefacts").

        ``Nfft = [F, K]`` (default ``[T, N]``) zero-pads or truncates.  Lengths the in-LDS kernels take (products of 2, 3, 5, 7, 11, 13 up to
        8192, K up to 600) run ``qdas_migration`` (``qups_amd.migration.migrate``); any other length runs ``qups_amd.migration.compose`` (torch.fft
        and ``wsinterpd``), whose transmit blocks ``bsize`` bounds; the library bounds its own work buffer.  complex64 data only.
        A per-transmit ``t0`` raises: the transmits would land on different depth axes and their sum has no scan -- ``ChannelData.rectifyt0`` first."""
        import warnings
        import torch
        from . import _lib, migration as MG
        if not isinstance(chd, ChannelData):
            raise DasError("bfMigration: chd must be one ChannelData")
        if interp not in _lib.INTERP_FLAGS:
            raise DasError("Interp option not recognized: " + str(interp))
        if self.seq.type != "PW":
            warnings.warn(f'Expected a Sequence of type "PW", but instead it was type "{self.seq.type}". Unexpected results may occur.')
        if self.xdc.kind != "TransducerArray":
            warnings.warn(f'Expected a TransducerArray but the Transducer is a {self.xdc.kind}". Unexpected results may occur.')
        chd = chd.rectifyDims()
        x = chd._torch_data()
        if x.dtype != torch.complex64:
            raise DasError(f"bfMigration: complex64 data only, got {str(x.dtype).replace('torch.', '')}")
        if np.size(chd.t0) != 1:
            raise DasError("bfMigration: t0 must be a scalar: transmits with different start times land on different depth axes -- "
                           "resample them onto one with ChannelData.rectifyt0 first")
        if x.ndim < 3:
            x = x.reshape(tuple(x.shape) + (1,) * (3 - x.ndim))
        T, N, M = (int(v) for v in x.shape[:3])
        F, K = MG._nfft(Nfft, T, N)
        if bsize is not None and (int(bsize) != bsize or bsize < 1):
            raise DasError("bfMigration: bsize must be a positive integer")
        if N != self.xdc.numel:
            raise DasError("Number of receives must match number of receiver elements.")
        c0 = float(self.seq.c0 if c0 is None else c0)
        sq = Sequence(self.seq.type, self.seq.focus, c0, self.seq.numPulse)
        tau = np.asarray(sq.delays(self.xdc), float)
        if tau.shape != (N, M):
            raise DasError(f"Number of transmits ({M}) must match the sequence's delays ({tau.shape[0]} x {tau.shape[1]}).")
        pn = np.asarray(self.xdc.positions(), float)
        pitch = self.xdc.pitch if self.xdc.pitch is not None else float(np.linalg.norm(pn[:, 1] - pn[:, 0]))
        gam = MG.gamma(self.seq.focus) if self.seq.type == "PW" else np.zeros(M)
        t0, fs = float(np.asarray(chd.t0, float).reshape(-1)[0]), float(chd.fs)
        if not x.is_cuda:
            if not torch.cuda.is_available():
                raise RuntimeError("qups_amd: no HIP device visible -- the migration beamformer has no CPU fallback")
            x = x.cuda()
        b = MG.bmode(x, t0, fs, tau, gam, pitch, c0, (F, K), fmod, interp, jacobian, keep_tx, None if bsize is None else int(bsize))
        Tn, Nn = min(T, F), min(N, K)
        zax = c0 / 2.0 * (t0 + np.arange(F) / fs)
        z = float(self.xdc.offset[2]) + zax[:Tn]
        z = z[0] + (np.mean(np.diff(z)) if Tn > 1 else 0.0) * np.arange(Tn)
        return b, Scan.cartesian(pn[0, 0] + pitch * np.arange(Nn), z, (float(self.xdc.offset[1]),))

    def bfDASLUT(self, chd: ChannelData, tau_rx, tau_tx, *apods, apod=1, fmod=0.0, interp="cubic", keep_tx=False,
                 keep_rx=False, prec=None, bsize=None):
        """``b = bfDASLUT(us, chd, tau_rx, tau_tx, ...)`` (reference ``src/UltrasoundSystem.m:4476-4673``):
        ``tau_rx`` is ``I1 x I2 x I3 x N``, ``tau_tx`` is ``I1 x I2 x I3 x M`` (times).  Output
        ``I1 x I2 x I3 x F... x [N] x [M]``: the aperture dimensions are moved behind the frame dimensions exactly as the
        reference does (``:4663-4664``) -- the same layout as ``DAS`` (``:3361``).

        ``bsize``: transmits per block (reference ``:4573``: default from a 1 GB bound on the multiplied-out weights; ``:4641-4655``: the
        transmits are spliced, the apodization arrays with a transmit dimension are indexed per block, blocks are summed -- or, with
        ``keep_tx``, concatenated).  The multiplied-out ``I x N x M`` weight array never exists for more than one block."""
        chds, chddim = self._chd_array(chd)
        # (:4580-4587, :4604-4611) the tables serve every ChannelData of the array: one receiver count, one transmit count
        Ns = sorted({int(c.data.shape[c.order.index("N")]) for c in chds})
        if len(Ns) != 1:
            raise DasError("Expected a single receiver size, but instead they have sizes [" + ",".join(str(v) for v in Ns) + "].",
                           "QUPS:UltrasoundSystem:bfDASLUT:nonUniqueReceiverSize")
        Ms = sorted({int(c.data.shape[c.order.index("M")]) for c in chds})
        if len(Ms) != 1:
            raise DasError("Expected a single transmit size, but instead they have sizes [" + ",".join(str(v) for v in Ms) + "].",
                           "QUPS:UltrasoundSystem:bfDASLUT:nonUniqueTransmitSize")
        if len(chds) > 1 or chddim is not None:          # each ChannelData on its own (:4629), images concatenated along the array's dimension (:4670-4672)
            import torch
            outs = [self.bfDASLUT(c, tau_rx, tau_tx, *apods, apod=apod, fmod=fmod, interp=interp, keep_tx=keep_tx, keep_rx=keep_rx, prec=prec, bsize=bsize)
                    for c in chds]
            nd = max(max(o.ndim for o in outs), (chddim or 0) + 1)
            outs = [o.reshape(tuple(o.shape) + (1,) * (nd - o.ndim)) for o in outs]
            return outs[0] if chddim is None else torch.cat(outs, dim=chddim)
        chd = chds[0]
        if chd.order[:3] != "TNM":
            chd = chd.rectifyDims()
        Isz = self.scan.size
        tr, tt = np.asarray(tau_rx) if not hasattr(tau_rx, "shape") else tau_rx, tau_tx
        N, M = Ns[0], Ms[0]
        if tuple(tr.shape) != Isz + (N,):
            raise DasError(f"Expected a receive delay table of size {Isz + (N,)}, got {tuple(tr.shape)}.",
                           "QUPS:UltrasoundSystem:bfDASLUT:incompatibleReceiveDelayTable")
        if tuple(tt.shape) != Isz + (M,):
            raise DasError(f"Expected a transmit delay table of size {Isz + (M,)}, got {tuple(tt.shape)}.",
                           "QUPS:UltrasoundSystem:bfDASLUT:incompatibleTransmitDelayTable")
        ws = [np.asarray(a) for a in list(apods) + ([] if (np.isscalar(apod) and apod == 1) else [apod])]
        ws = [a.reshape(a.shape + (1,) * (5 - a.ndim)) for a in ws]
        if bsize is None:                                  # the reference's heuristic (:4573): blocks whose multiplied-out weights stay below 1 GB (8-byte entries)
            full = np.max([a.shape for a in ws], axis=0) if ws else np.ones(5, int)
            gb = 2.0 ** -30 * 8 * float(np.prod(full))
            bsize = max(1, min(M, int(np.floor(M / gb)) if gb > 0 else M))
        bsize = int(bsize)
        if bsize < 1:
            raise DasError("bsize must be a positive integer")
        sdim = set() if keep_rx else {"rx"}
        sdim |= set() if keep_tx else {"tx"}
        kw = {"prec": prec} if prec else {}
        w0 = None                                          # arrays without a transmit dimension: multiplied once (:4644)
        for a in ws:
            if a.shape[4] == 1:
                w0 = a if w0 is None else w0 * a
        t0a = np.asarray(chd.t0, dtype=np.float64).reshape(-1)
        parts, total = [], None
        for m0 in range(0, M, bsize):
            sl = slice(m0, min(M, m0 + bsize))
            w = w0
            for a in ws:                                   # per-block factors (:4647-4650)
                if a.shape[4] != 1:
                    w = a[..., sl] if w is None else w * a[..., sl]
            bm = sample2sep(chd.data[:, :, sl], t0a if t0a.size == 1 else t0a[sl], chd.fs, tr, tt[..., sl], interp=interp, w=w, sdim=sdim, fmod=fmod, **kw)
            if keep_tx:
                parts.append(bm)
            else:
                total = bm if total is None else total + bm
        b = _cat_tx(parts) if keep_tx else total          # I1 x I2 x I3 x [N] x [M] x F...
        return b.permute(0, 1, 2, *range(5, b.ndim), 3, 4)           # move the aperture dimensions to the end (:4663-4664)
