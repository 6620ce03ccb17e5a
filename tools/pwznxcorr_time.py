"""Time pwznxcorr (one qdas_pwznxcorr launch for all lags) beside the same steps composed in plain torch -- torch.roll + conv1d, one pass per
lag, which stands in for the reference's convn / circshift implementation -- on two shapes, complex64, zero = norm = pad = true:

    python tools/pwznxcorr_time.py [--shapes chd,img] [--reps 10]

chd: a channel-data record, T = 2816 x N = 256, L = 8 (17 lags), W = 64, neighbouring channels.
img: a receive-kept image, 512 x 512 x 128 (depth fastest, receivers slowest: the DAS(keep_rx=True) view), correlated along depth across
     receivers, L = 4 (9 lags), W = 16.
The two are timed in the same process with interleaved repeats (kernel, composition, kernel, ...) after a warm-up of both; device-event ms,
median [min .. max].  Before timing the two results are compared at the timed size.  Bytes and flops are algorithmic (from shapes): one read
of x and one write of y; per output sample and lag 2 W FMA for K(c) of a complex sample, 2 W for K(xlz cz), W for K(|cz|^2) -- 10 W flop --
plus 12 for the products.  The roof is the larger of bytes / 6.0 TB/s (measured HBM copy rate) and flops / 157.3 TFLOP/s (FP32 vector)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from qups_amd import pwznxcorr  # noqa: E402

HBM, VALU = 6.0e12, 157.3e12
SHAPES = {"chd": dict(T=2816, N=256, B=1, L=8, W=64), "img": dict(T=512, N=128, B=512, L=4, W=16)}


def conv_same(a, w):
    """MATLAB's conv 'same' along the last dimension of a complex or real (R, Tp) tensor: offset floor(W / 2) of the full convolution"""
    W = w.numel()
    h = W // 2
    cplx = a.is_complex()
    r = torch.view_as_real(a).permute(0, 2, 1).reshape(-1, 1, a.shape[-1]) if cplx else a.unsqueeze(1)
    r = F.conv1d(F.pad(r, (W - 1 - h, h)), w.flip(0).view(1, 1, W))
    if cplx:
        return torch.view_as_complex(r.reshape(a.shape[0], 2, a.shape[-1]).permute(0, 2, 1).contiguous())
    return r.squeeze(1)


def composition(xl, xr, w, lags):
    """xl, xr: (R, T) records, time contiguous; returns (len(lags), R, T)"""
    T = xl.shape[-1]
    P = max(abs(l) for l in lags)
    xl, xr = F.pad(xl, (0, P)), F.pad(xr, (0, P))
    xlz = xl - conv_same(xl, w)
    xln = conv_same((xlz * xlz.conj()).real, w).sqrt()
    out = torch.empty((len(lags),) + tuple(xl.shape[:-1]) + (T,), dtype=xl.dtype, device=xl.device)
    for i, l in enumerate(lags):
        c = torch.roll(xr, -l, -1).conj_physical()
        cz = c - conv_same(c, w)
        y = conv_same(xlz * cz, w)
        xrn = conv_same((cz * cz.conj()).real, w).sqrt()
        out[i] = (y / (xln * xrn))[..., :T]
    return out


def interleaved(fa, fb, reps):
    for _ in range(2):
        fa()
        fb()
    torch.cuda.synchronize()
    ta, tb = [], []
    for _ in range(reps):
        for f, ts in ((fa, ta), (fb, tb)):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            torch.cuda.synchronize()
            ts.append(e0.elapsed_time(e1))
    return ta, tb


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="chd,img")
    ap.add_argument("--reps", type=int, default=10)
    a = ap.parse_args()
    print(f"device: {torch.cuda.get_device_name(0)}")
    g = torch.Generator(device="cuda").manual_seed(0)
    for name in a.shapes.split(","):
        s = SHAPES[name]
        T, N, B, L, W = s["T"], s["N"], s["B"], s["L"], s["W"]
        lags = list(range(-L, L + 1))
        X = torch.view_as_complex(torch.randn((N, B, T, 2), generator=g, device="cuda", dtype=torch.float32))   # N x B x T, time fastest
        X = X * (1 + 3 * torch.rand((N, 1, 1), generator=g, device="cuda"))
        x = X.permute(2, 1, 0)                               # T x B x N: tdim = 1, ndim = 3 (the DAS view; B = 1: a T x N record)
        w = torch.ones(W, device="cuda")
        fk = lambda: pwznxcorr(x, L, W, tdim=1, ndim=3)
        ft = lambda: composition(X[:-1].reshape(-1, T), X[1:].reshape(-1, T), w, lags)
        yk = fk().permute(3, 2, 1, 0).reshape(len(lags), -1, T)          # lags x (N - 1) B x T
        yt = ft()
        err = float((yk - yt).abs().max() / yt.abs().max())
        del yk, yt
        tk, tt = interleaved(fk, ft, a.reps)
        mk, mt = statistics.median(tk), statistics.median(tt)
        outs = (N - 1) * B * T * len(lags)
        byts, flop = N * B * T * 8 + outs * 8, outs * (10 * W + 12)
        tb, tv = byts / HBM * 1e3, flop / VALU * 1e3
        print(f"{name}: T={T} N={N} batch={B} lags={len(lags)} W={W} complex64   max|kernel - composition| / max = {err:.2e}")
        print(f"  qdas_pwznxcorr    {mk:9.3f} ms  [{min(tk):.3f} .. {max(tk):.3f}]   {byts / 1e9:.3f} GB  {flop / 1e9:.1f} GFLOP  "
              f"roof {max(tb, tv):.3f} ms ({'HBM' if tb >= tv else 'VALU'}) = {100 * max(tb, tv) / mk:.1f} %")
        print(f"  torch composition {mt:9.3f} ms  [{min(tt):.3f} .. {max(tt):.3f}]   ratio composition / kernel = {mt / mk:.1f}x")
        del X, x
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
