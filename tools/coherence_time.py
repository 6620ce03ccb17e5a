"""Time slsc (average, ensemble), dmas, cohfac and pcf on receive-kept images (complex64, default lags) in the layout DAS(keep_rx=True)
returns (I1 fastest, the aperture slowest), plus an aperture-fastest input, against the same estimators composed in plain torch.

    python tools/coherence_time.py [--sizes C2,C3] [--reps 20]

C2: 512 x 512 pixels x N = 128 (268 MB); C3: 1024 x 1024 x N = 256 (2.1 GB).  Device-event ms, median of --reps after warm-up.  The roof is
the larger of bytes / 6.0 TB/s (measured HBM copy rate) and flops / 157.3 TFLOP/s (FP32 vector); "roof %" = roof time / measured time.
The aperture-fastest row counts the estimator's bytes and flops; the transposition it needs first is extra time, printed beside it.
Bytes and flops are algorithmic (from shapes): one read of the image and one write of the output; 4 flop per receiver pair and lag for
SLSC (two FMA of Re(a conj b)), 8 per sample for the O(N) DMAS, 4 per sample for cohfac, ~40 per sample for pcf (atan2 included)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from qups_amd import cohfac, dmas, pcf, slsc  # noqa: E402

HBM, VALU = 6.0e12, 157.3e12
SIZES = {"C2": (512, 512, 128), "C3": (1024, 1024, 256)}


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return statistics.median(ts)


# ---- the estimators composed in plain torch (x: I1 x I2 x N, aperture last)
def t_slsc_avg(x, L):
    N = x.shape[-1]
    xh = torch.nan_to_num(x / x.abs(), nan=0.0)
    z = 0
    for lag in range(1, L + 1):
        z = z + (xh[..., :-lag] * xh[..., lag:].conj()).real.sum(-1, keepdim=True) / (L * (N - lag))
    return z


def t_slsc_ens(x, L):
    z = a = 0
    for lag in range(1, L + 1):
        u, v = x[..., :-lag], x[..., lag:]
        z = z + 2 * (u * v.conj()).real.sum(-1, keepdim=True)
        a = a + (u.abs() ** 2).sum(-1, keepdim=True) + (v.abs() ** 2).sum(-1, keepdim=True)
    return z / a


def t_dmas(x):
    s = x.sum(-1, keepdim=True)
    b = (s * s - (x * x).sum(-1, keepdim=True)) / 2
    return torch.polar(b.abs().sqrt(), b.angle())


def t_cohfac(x):
    return x.sum(-1, keepdim=True).abs() ** 2 / (x.abs() ** 2).sum(-1, keepdim=True) / x.shape[-1]


def t_pcf(x):
    ph = x.angle()
    s0 = ph.std(-1, correction=0, keepdim=True)
    sa = (ph - torch.pi * ph.sign()).std(-1, correction=0, keepdim=True)
    return (1 - torch.fmin(s0, sa) / (torch.pi / 3) ** 0.5).clamp_min(0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="C2,C3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-torch", action="store_true")
    a = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}")
    print(f"{'size':4s} {'function':16s} {'layout':9s} {'ms':>8s} {'GB':>7s} {'GFLOP':>8s} {'bound':5s} {'roof %':>6s} {'torch ms':>9s} {'speed-up':>8s}")
    g = torch.Generator(device="cuda").manual_seed(0)
    for name in a.sizes.split(","):
        I1, I2, N = SIZES[name]
        P = I1 * I2
        L = max(1, N // 4)
        xr = torch.randn((N, I2, I1, 2), generator=g, device="cuda", dtype=torch.float32)
        xc = torch.view_as_complex(xr)                       # N x I2 x I1 contiguous ...
        b = xc.permute(2, 1, 0)                              # ... seen as I1 x I2 x N: the DAS(keep_rx=True) layout
        del xr
        pairs = L * N - L * (L + 1) // 2
        rd, wr = P * N * 8, P * 8
        cases = [
            ("slsc average", lambda: slsc(b, 3), lambda: t_slsc_avg(b, L), rd + wr, 4 * pairs * P),
            ("slsc ensemble", lambda: slsc(b, 3, None, "ensemble"), lambda: t_slsc_ens(b, L), rd + wr, (4 * pairs + 3 * N) * P),
            ("dmas", lambda: dmas(b, 3), lambda: t_dmas(b), rd + wr, 8 * N * P),
            ("cohfac", lambda: cohfac(b, 3), lambda: t_cohfac(b), rd + P * 4, 4 * N * P),
            ("pcf", lambda: pcf(b, 3), lambda: t_pcf(b), rd + P * 8, 40 * N * P),
        ]

        def row(fname, layout, f, tf, byts, flop, extra=""):
            ms = timed(f, a.reps)
            tb, tv = byts / HBM * 1e3, flop / VALU * 1e3
            tms = None if a.no_torch else timed(tf, max(3, a.reps // 4))
            print(f"{name:4s} {fname:16s} {layout:9s} {ms:8.3f} {byts / 1e9:7.3f} {flop / 1e9:8.1f} {'HBM' if tb >= tv else 'VALU':5s} "
                  f"{100 * max(tb, tv) / ms:6.1f} " + (f"{tms:9.3f} {tms / ms:8.1f}x" if tms is not None else "") + extra)

        for fname, f, tf, byts, flop in cases:
            row(fname, "DAS view", f, tf, byts, flop)
        # aperture-fastest input (a contiguous I1 x I2 x N tensor, torch's own layout for it): qdas_permute3 first, then the kernel.  The bytes and the
        # roof are the estimator's (the transposition is extra work the layout costs); the torch composition runs on the same tensor.
        bc = b.contiguous()
        from qups_amd import coherence as Q
        ms_perm = timed(lambda: Q._to_canonical(bc, [2]), a.reps)
        row("slsc average", "N fastest", lambda: slsc(bc, 3), lambda: t_slsc_avg(bc, L), rd + wr, 4 * pairs * P,
            f"   (qdas_permute3 transposition: {ms_perm:.3f} ms of it)")
        del b, bc, xc
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
