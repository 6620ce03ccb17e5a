"""QDAS_PLAN_JIT: the tiled kernel compiled by hiprtc with the plan's sizes as constants -- the reference's const-compile
specialisation (src/UltrasoundSystem.m:5626-5748 getDASConstCudaDef, src/sizes.cu:17-52; its own check: test/ParTest.m:322-327)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

from tests.cases import stock_kernel, cinv_f32, make_case, rel_err


def test_hiprtc_builds_the_specialised_kernel_without_a_device(tmp_path, monkeypatch):
    """(CPU) libqdas.so carries the kernel headers and hiprtc compiles a specialisation of them for gfx950 -- no spills, no scratch"""
    import sys
    from qups_amd import _lib
    monkeypatch.setenv("QDAS_CACHE_DIR", str(tmp_path))
    L = _lib.lib()
    f = L.qdas_debug_jit_compile
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_char_p, C.c_size_t, C.POINTER(C.c_ulonglong)]
    monkeypatch.setenv("QDAS_JIT_NARROW", "1")            # the reciprocal build plans use: 128-sample windows, 32 transmits per stage
    monkeypatch.setenv("QDAS_JIT_MB", "32")
    for interp, dtype, sym, fmod in ((3, 1, 1, 0), (2, 2, 0, 1)):
        msg, n = C.create_string_buffer(4000), C.c_ulonglong()
        rc = f(interp, dtype, sym, fmod, 64, 64, 1024, msg, 4000, C.byref(n))
        if rc and b"hiprtc not available" in msg.value:
            pytest.skip(msg.value.decode())
        assert rc == 0, msg.value.decode()
        assert n.value > 10000 and os.path.exists(tmp_path / (msg.value.decode() + ".hsaco"))     # cached on disk under its key
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_regs
    rows = [r for fn in os.listdir(tmp_path) if fn.endswith(".hsaco") for r in kernel_regs.kernel_table(str(tmp_path / fn))]
    assert len(rows) == 2 and all(r["name"].startswith("qdas_jit_tile__") and r["vgpr_spill"] == 0 and r["scratch"] == 0 for r in rows), rows


def test_disk_cache_is_checked_and_private(tmp_path, monkeypatch):
    """(CPU) the code-object cache: a second request is served from disk, a truncated or tampered file is rejected and rebuilt, a
    group-/world-writable cache directory is not used at all, and nothing is cached without HOME / QDAS_CACHE_DIR"""
    import stat
    import time
    from qups_amd import _lib
    L = _lib.lib()
    f = L.qdas_debug_jit_compile
    f.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_ulonglong, C.c_ulonglong, C.c_ulonglong, C.c_char_p, C.c_size_t, C.POINTER(C.c_ulonglong)]

    def build(N):
        msg, n = C.create_string_buffer(4000), C.c_ulonglong()
        t = time.perf_counter()
        rc = f(1, 1, 0, 0, N, 16, 512, msg, 4000, C.byref(n))
        if rc and b"hiprtc not available" in msg.value:
            pytest.skip(msg.value.decode())
        assert rc == 0, msg.value.decode()
        return msg.value.decode(), n.value, time.perf_counter() - t

    cache = tmp_path / "c"
    monkeypatch.setenv("QDAS_CACHE_DIR", str(cache))
    key, size, t_cold = build(24)
    path = cache / (key + ".hsaco")
    raw = path.read_bytes()
    assert raw[:4] == b"\x7fELF" and raw[-24:-16] == b"QDASHSA1" and len(raw) == size + 24          # the code object + its trailer
    assert stat.S_IMODE(os.stat(cache).st_mode) == 0o700 and stat.S_IMODE(os.stat(path).st_mode) == 0o600
    # (a second process would load it from disk; in this process the in-memory cache answers -- so tamper and ask for ANOTHER key)
    key2, size2, _ = build(40)
    p2 = cache / (key2 + ".hsaco")
    good = p2.read_bytes()
    for bad in (good[:-30], good[:100] + bytes([good[100] ^ 1]) + good[101:], b"\x7fELF" + b"\0" * 64):
        p2.write_bytes(bad)
        out = subprocess.run([sys.executable, "-c",
                              "import ctypes as C, sys; sys.path.insert(0, %r); from qups_amd import _lib; L = _lib.lib(); f = L.qdas_debug_jit_compile;"
                              "f.argtypes = [C.c_int] * 4 + [C.c_ulonglong] * 3 + [C.c_char_p, C.c_size_t, C.POINTER(C.c_ulonglong)];"
                              "m = C.create_string_buffer(4000); n = C.c_ulonglong(); rc = f(1, 1, 0, 0, 40, 16, 512, m, 4000, C.byref(n)); print(rc, m.value.decode(), n.value)"
                              % os.path.dirname(os.path.dirname(os.path.abspath(__file__)))],
                             capture_output=True, text=True, env=dict(os.environ), timeout=300)
        assert out.returncode == 0 and out.stdout.split()[:2] == ["0", key2], (out.stdout, out.stderr[-500:])
        assert p2.read_bytes() == good                                      # rejected, rebuilt, rewritten
    os.chmod(cache, 0o777)                                                   # a directory others can write to: not used
    key3, _, _ = build(56)
    assert not (cache / (key3 + ".hsaco")).exists()
    os.chmod(cache, 0o700)


@pytest.mark.gpu
@pytest.mark.parametrize("seq,interp,prec,extra", [
    ("FSA", "lanczos3", "single", {}), ("PW", "cubic", "single", {}), ("FC", "linear", "single", {}), ("DV", "nearest", "single", {}),
    ("FSA", "cubic", "halfT", {}), ("PW", "lanczos3", "single", {"fmod": 2.5e6}), ("FSA", "linear", "single", {"noreci": True}),
])
def test_jit_plan_matches_prebuilt_and_oracle(seq, interp, prec, extra, tmp_path, monkeypatch):
    import torch
    from oracle import das_oracle as O
    from qups_amd import DasPlan, build_problem, parse_options
    monkeypatch.setenv("QDAS_CACHE_DIR", str(tmp_path))
    case = make_case(seq=seq, interp=interp, seed=31, N=16, I1=150, I2=37)
    x = torch.from_numpy(case["x"])
    fmod = float(np.float32(extra.get("fmod", 0.0)))
    va = list(case["opt"]) + ["interp", interp, "input-precision", prec, "modulation", fmod]
    opts = parse_options(x, va)
    T, N, M = case["x"].shape
    prob = build_problem("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], (T, N, M), case["t0"], case["fs"], case["c"], opts)
    ys, names = [], []
    for jit in (False, True):
        plan = DasPlan(prob, kernel=2, jit=jit, reciprocal=not extra.get("noreci", False))
        y = plan.feval(x)
        ys.append(torch.view_as_real(y).float().cpu().numpy().view(np.complex64)[..., 0] if prec == "halfT" else y.cpu().numpy())
        names.append(plan.kernel_name())
        plan.close()
    assert stock_kernel(names[0]) and "[jit " in names[1], names          # the hiprtc kernel really ran
    # ... and its code object is in the disk cache (unless this process had built the same key before: then the in-memory cache answered)
    assert len([f for f in os.listdir(tmp_path) if f.endswith(".hsaco")]) <= 2       # (+ the stock variant, when it is one that is built on demand)
    ref = O.das_spec("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], case["x"], case["t0"], case["fs"], cinv_f32(case["c"]),
                     VS=case["VS"], DV=case["DV"], interp=interp, fmod=fmod).reshape(-1, order="F")     # feval: I x 1 x 1, I1 fastest
    tol = 2e-3 if prec == "halfT" else (1e-2 if interp == "nearest" else 2e-5 if not fmod else 2e-4)
    assert rel_err(ys[1].reshape(-1), ref) <= tol
    assert rel_err(ys[1], ys[0]) <= 1e-6                                     # same arithmetic as the prebuilt instantiation


@pytest.mark.gpu
@pytest.mark.parametrize("N", [32, 64])
@pytest.mark.parametrize("prec", ["single", "halfT"])
@pytest.mark.parametrize("wtab", [False, True], ids=["plain", "weight-table"])
def test_jit_reciprocal_32_transmit_stages(N, prec, wtab, tmp_path, monkeypatch):
    """The headline kernel variant at test size: FSA with N % 32 == 0 takes the reciprocal mode, and its hiprtc build runs 32-transmit
    stages (csrc/qdas_api.hip: ``k.mb = 32``) -- a configuration that exists ONLY as a hiprtc build.  fp32 and fp16 data, with and
    without a pixel-independent N x M weight table; against the float64 oracle and the prebuilt 16-transmit kernel."""
    import torch
    from oracle import das_oracle as O
    from qups_amd import DasPlan, build_problem, parse_options
    monkeypatch.setenv("QDAS_CACHE_DIR", str(tmp_path))
    case = make_case(seq="FSA", interp="lanczos3", seed=77 + N, N=N, I1=160, I2=40, pitch=0.2e-3, zlim=(5e-3, 16e-3), xspan=5e-3)
    x = torch.from_numpy(case["x"])
    va = list(case["opt"]) + ["interp", "lanczos3", "input-precision", prec]
    ap = ()
    if wtab:                                         # Hann receive x transmit windows: 1 x 1 x 1 x N and 1 x 1 x 1 x 1 x M
        wn = np.hanning(N + 2)[1:-1].astype(np.float32)
        a_rx, a_tx = wn.reshape(1, 1, 1, N, 1), (0.5 + 0.5 * wn).reshape(1, 1, 1, 1, N)
        va += ["apod", a_rx, "apod", a_tx]
        ap = (a_rx.astype(np.float64), a_tx.astype(np.float64))
    opts = parse_options(x, va)
    T = case["x"].shape[0]
    prob = build_problem("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], (T, N, N), case["t0"], case["fs"], case["c"], opts)
    ys, names, rec = [], [], []
    for jit in (False, True):
        with DasPlan(prob, kernel=2, jit=jit, mirror=False) as plan:       # (this array and scan are mirror-symmetric as well: that mode has its own tests, tests/test_gpu_mirror.py)
            y = plan.feval(x)
            ys.append(torch.view_as_real(y).float().cpu().numpy().view(np.complex64)[..., 0] if prec == "halfT" else y.cpu().numpy())
            names.append(plan.kernel_name()); rec.append(plan.reciprocal)
            assert plan.fallback_tiles() == 0
    assert all(rec), names
    # (one-set plans on fp32 frames -- fp16 data fold into one -- whose tiles fit 128-sample windows take 64-transmit stages instead: csrc/qdas_api.hip plan_stage_shape)
    assert stock_kernel(names[0]) and "[jit " in names[1] and ",sym" in names[1], names
    assert ",mb=32," in names[1] or (N >= 64 and ",mb=64,W=128" in names[1]), names
    assert ("wtab" in names[1]) == wtab, names
    ref = O.das_spec("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], case["x"], case["t0"], case["fs"], cinv_f32(case["c"]),
                     VS=case["VS"], DV=case["DV"], interp="lanczos3", apod=ap).reshape(-1, order="F")
    tol = 2e-3 if prec == "halfT" else 2e-5
    assert rel_err(ys[1].reshape(-1), ref) <= tol, names[1]
    assert rel_err(ys[0].reshape(-1), ref) <= tol, names[0]
    assert rel_err(ys[1], ys[0]) <= (2e-6 if prec == "single" else 1e-5)    # another stage partition: fp32 re-association only


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["general", "fold", "mirror"])
def test_jit_stage_shapes_of_plans_whose_tiles_fit_128_sample_windows(mode, tmp_path, monkeypatch):
    """csrc/qdas_api.hip plan_stage_shape: a plan-specialised build takes 64 transmits x 128 samples per stage for one-set plans (general mode, the fold
    without the mirror mode) and 32 x 2 x 128 for mirror plans when every tile fits 128-sample windows -- shapes that exist ONLY as hiprtc builds.  Against
    the float64 oracle and the prebuilt shape of the same mode (another stage partition: fp32 re-association only); QDAS_NO_STAGE_SHAPE keeps the prebuilt shape."""
    import torch
    from oracle import das_oracle as O
    from qups_amd import DasPlan, build_problem, parse_options
    monkeypatch.setenv("QDAS_CACHE_DIR", str(tmp_path))
    N = 128
    case = make_case(seq="FSA", interp="cubic", seed=5, N=N, I1=128, I2=64, pitch=0.2e-3, zlim=(20e-3, 24e-3), xspan=4e-3)
    x = torch.from_numpy(case["x"])
    opts = parse_options(x, list(case["opt"]) + ["interp", "cubic"])
    T = case["x"].shape[0]
    prob = build_problem("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], (T, N, N), case["t0"], case["fs"], case["c"], opts)
    kw = dict(general=dict(reciprocal=False, mirror=False), fold=dict(reciprocal=True, mirror=False), mirror=dict(reciprocal=False, mirror=True))[mode]
    want = dict(general=",mb=64,W=128>", fold=",sym,fold,mb=64,W=128>", mirror=",mirror,mb=32,W=128>")[mode]
    ys, names = [], []
    for shape_off in (False, True):
        if shape_off:
            monkeypatch.setenv("QDAS_NO_STAGE_SHAPE", "1")
        with DasPlan(prob, kernel=2, jit=True, **kw) as plan:
            ys.append(plan.feval(x).cpu().numpy())
            names.append(plan.kernel_name())
            assert plan.fallback_tiles() == 0
    assert want in names[0] and "[jit " in names[0], names
    assert want not in names[1], names
    ref = O.das_spec("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], case["x"], case["t0"], case["fs"], cinv_f32(case["c"]),
                     VS=case["VS"], DV=case["DV"], interp="cubic").reshape(-1, order="F")
    assert rel_err(ys[0].reshape(-1), ref) <= 2e-5, names[0]
    assert rel_err(ys[1].reshape(-1), ref) <= 2e-5, names[1]
    assert rel_err(ys[0], ys[1]) <= 2e-6, names


@pytest.mark.gpu
@pytest.mark.parametrize("prec", ["single", "halfT"])
@pytest.mark.parametrize("weights", ["array", "generated"])
def test_jit_long_stages_with_a_pixel_by_receiver_weight(prec, weights, tmp_path, monkeypatch):
    """round 6: lateral-mirror plans WITH a pixel x receiver weight take the long-stage shape as well -- fp16 data 32 transmits x 2 sets x 256 samples, fp32 data
    32 x 2 x 128 (one accumulator per pixel made the room for the weighted totals) -- when every tile fits the one-KiB windows.  Against the float64 oracle fed the
    materialised mask, and against the shape of round 5 (QDAS_NO_STAGE_SHAPE=1: another stage partition, fp32 re-association only); no build may use scratch."""
    import torch
    from oracle import das_oracle as O
    from qups_amd import DasPlan, build_problem, parse_options
    from qups_amd import apodization as A
    monkeypatch.setenv("QDAS_CACHE_DIR", str(tmp_path))
    N = 64
    case = make_case(seq="FSA", interp="cubic", seed=8, N=N, I1=128, I2=64, pitch=0.2e-3, zlim=(20e-3, 24e-3), xspan=4e-3)
    nrm = np.tile(np.array([[0.0], [0.0], [1.0]]), (1, N))
    mask = A.ap_acceptance_angle(case["Pi"], case["Pr"], nrm, 8.0).astype(np.float32)          # (I1 x I2 x 1 x N: a band of receivers per pixel)
    assert 0.1 < float((mask != 0).mean()) < 0.9
    x = torch.from_numpy(case["x"])
    extra = ["apod", mask] if weights == "array" else ["rx-apod", A.rx_apod_spec("acceptance", normals=nrm, theta=8.0)]
    opts = parse_options(x, list(case["opt"]) + ["interp", "cubic", "input-precision", prec] + extra)
    T = case["x"].shape[0]
    prob = build_problem("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], (T, N, N), case["t0"], case["fs"], case["c"], opts)
    want = ",mirror,mb=32,W=256>" if prec == "halfT" else ",mirror,mb=32,W=128>"
    ys, names = [], []
    for shape_off in (False, True):
        if shape_off:
            monkeypatch.setenv("QDAS_NO_STAGE_SHAPE", "1")
        with DasPlan(prob, kernel=2, jit=True, reciprocal=False) as plan:
            ys.append(plan.feval(x).to(torch.complex64).cpu().numpy())
            names.append(plan.kernel_name())
            assert plan.fallback_tiles() == 0 and plan.mirror
    assert want in names[0] and "[jit " in names[0], names
    assert want not in names[1], names
    xo = case["x"] if prec == "single" else case["x"].astype(np.complex64).view(np.float32).astype(np.float16).astype(np.float32).view(np.complex64)
    mo = mask if prec == "single" else mask.astype(np.float16).astype(np.float32)
    ref = O.das_spec("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], xo, case["t0"], case["fs"], cinv_f32(case["c"]),
                     VS=case["VS"], DV=case["DV"], interp="cubic", apod=(mo.astype(np.float64).reshape(128, 64, 1, N, 1),)).reshape(-1, order="F")
    tol = 2e-3 if prec == "halfT" else 3e-5
    assert rel_err(ys[0].reshape(-1), ref) <= tol, (names[0], rel_err(ys[0].reshape(-1), ref))
    assert rel_err(ys[1].reshape(-1), ref) <= tol, names[1]
    assert rel_err(ys[0], ys[1]) <= (1e-3 if prec == "halfT" else 5e-6), names
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_regs
    rows = [r for fn in os.listdir(tmp_path) if fn.endswith(".hsaco") for r in kernel_regs.kernel_table(str(tmp_path / fn))]
    built = [r for r in rows if ("mb32_w256" in r["name"] or "mb32_w128" in r["name"])]
    assert built and any(r["vgpr_spill"] == 0 and r["scratch"] == 0 for r in built), rows       # (the kernel that ran: a first, spilling attempt may sit beside its plain-loop rebuild)


@pytest.mark.gpu
def test_jit_modes_syn_mul_and_pixel_weights(tmp_path, monkeypatch):
    """the specialised kernel also serves kept dimensions (planes) and a pixel x receiver apodization"""
    import torch
    from qups_amd import das_spec
    monkeypatch.setenv("QDAS_CACHE_DIR", str(tmp_path))
    case = make_case(seq="PW", interp="cubic", seed=33, N=12, M=10, I1=100, I2=20)
    args = (case["Pi"], case["Pr"], case["Pv"], case["Nv"], torch.from_numpy(case["x"]), case["t0"], case["fs"], case["c"])
    rng = np.random.default_rng(5)
    a_pix = rng.random((100, 20, 1, 12, 1)).astype(np.float32)
    for fun, ap in (("SYN", None), ("MUL", None), ("DAS", a_pix)):
        extra = ["apod", ap] if ap is not None else []
        y0, p0 = das_spec(fun, *args, *case["opt"], "interp", "cubic", *extra, return_plan=True, kernel=2)
        y1, p1 = das_spec(fun, *args, *case["opt"], "interp", "cubic", *extra, return_plan=True, kernel=2, jit=True)
        assert "[jit " in p1.kernel_name() and stock_kernel(p0.kernel_name())
        assert rel_err(y1.cpu().numpy(), y0.cpu().numpy()) <= 1e-6, fun
        p0.close(); p1.close()


@pytest.mark.gpu
def test_environment_default_builds_the_specialised_kernel(tmp_path, monkeypatch):
    """QDAS_JIT=1: every das_spec / UltrasoundSystem call asks for the plan-specialised kernel (as the reference compiles its kernel per call)"""
    import torch
    from qups_amd import das_spec
    from tests.cases import make_case
    monkeypatch.setenv("QDAS_CACHE_DIR", str(tmp_path))
    case = make_case(seq="PW", interp="linear", seed=3, N=16, M=8, I1=64, I2=8)
    args = (case["Pi"], case["Pr"], case["Pv"], case["Nv"], torch.from_numpy(case["x"]), case["t0"], case["fs"], case["c"])
    y0, p0 = das_spec("DAS", *args, *case["opt"], "interp", "linear", return_plan=True)
    monkeypatch.setenv("QDAS_JIT", "1")
    y1, p1 = das_spec("DAS", *args, *case["opt"], "interp", "linear", return_plan=True)
    assert stock_kernel(p0.kernel_name()) and "[jit " in p1.kernel_name()
    a, b = y0.cpu().numpy(), y1.cpu().numpy()
    assert np.abs(a - b).max() <= 2e-6 * np.abs(a).max()


@pytest.mark.gpu
@pytest.mark.parametrize("mirror", [False, True], ids=["plain", "mirror"])
def test_jit_plan_streams_share_launches(mirror, tmp_path, monkeypatch):
    """a stream of frames through a plan with a hiprtc build: groups of four / two frames run the prebuilt frame-sharing kernels (shared tap
    indices and weights beat the specialisation), the odd frame the hiprtc build; every frame equals its one-by-one result"""
    import torch
    from qups_amd import DasPlan, build_problem, parse_options
    from qups_amd.das_spec import _colmajor
    monkeypatch.setenv("QDAS_CACHE_DIR", str(tmp_path))
    case = make_case(seq="PW", interp="cubic", seed=41, N=16, M=12, I1=128, I2=24)
    rng = np.random.default_rng(9)
    F = 7
    xs = np.stack([case["x"]] + [(rng.standard_normal(case["x"].shape) + 1j * rng.standard_normal(case["x"].shape)).astype(np.complex64) for _ in range(F - 1)], axis=3)
    xt = torch.from_numpy(xs)
    prob = build_problem("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], tuple(xt.shape), case["t0"], case["fs"], case["c"],
                         parse_options(xt, list(case["opt"]) + ["interp", "cubic"]))
    xc = _colmajor(xt.cuda())
    with DasPlan(prob, kernel=2, jit=True, mirror=mirror) as plan:
        assert "[jit " in plan.kernel_name() and plan.mirror == mirror
        y = plan.execute_colmajor(xc, F).cpu().numpy().reshape(F, -1)
        monkeypatch.setenv("QDAS_NO_FB2", "1")
        monkeypatch.setenv("QDAS_NO_FRAMES_TWIN", "1")
        y1 = plan.execute_colmajor(xc, F).cpu().numpy().reshape(F, -1)
    for f in range(F):
        assert rel_err(y[f], y1[f]) <= (3e-5 if mirror else 2e-6), f    # (mirror plans stream groups of four through their twin without the mirror mode: another summation order)
    assert rel_err(y[0], y[1]) > 1e-2                       # (different frames)


# ------------------------------------------------------------------------------------------ variants built on demand (das_tile_cfg.h TILE_PREBUILT)
def test_on_demand_variants_build_without_a_device(tmp_path, monkeypatch):
    """(CPU) a point of the template's matrix that libqdas.so does not carry compiles from the embedded headers with the template arguments the
    prebuilt instantiation would have had -- no spills, no scratch --, lands in the disk cache, and the matrix query answers consistently"""
    import sys
    from qups_amd import _lib, warm
    monkeypatch.setenv("QDAS_CACHE_DIR", str(tmp_path))
    L = _lib.lib()
    assert L.qdas_kernel_variant_prebuilt(17, 3, 0, 0) == 1          # the headline: folded, mirror, lanczos3
    assert L.qdas_kernel_variant_prebuilt(0, 5, 0, 0) == 0           # cubic_dev: on demand
    assert L.qdas_kernel_variant_prebuilt(1, 1, 0, 0) == -1 and L.qdas_kernel_variant_prebuilt(19, 1, 0, 1) == -1 and L.qdas_kernel_variant_prebuilt(0, 4, 0, 0) == -1
    assert L.qdas_kernel_variant_build(17, 3, 0, 0) == 2 and L.qdas_kernel_variant_build(1, 1, 0, 0) == 3
    rc = L.qdas_kernel_variant_build(2, 5, 1, 1)                      # fp16, cubic_dev, remodulation + weight table
    if rc == 1 and b"hiprtc not available" in (L.qdas_last_error() or b""):
        pytest.skip("hiprtc not available")
    assert rc == 0, L.qdas_last_error()
    assert warm.warm([(19, 1, 1, 0), (17, 3, 0, 0)], jobs=2) == 0     # one worker process per variant; the second is prebuilt: nothing to do
    files = [f for f in os.listdir(tmp_path) if f.endswith(".hsaco")]
    assert len(files) == 2, files
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import kernel_regs
    rows = [r for fn in files for r in kernel_regs.kernel_table(str(tmp_path / fn))]
    assert len(rows) == 2 and all(r["name"].startswith("qdas_jit_tile__") and r["vgpr_spill"] == 0 and r["scratch"] == 0 and r["vgpr"] + r["agpr"] <= 128 for r in rows), rows
    # the suite's own list (tests/conftest.py warms it on a GPU box) names variants of the matrix only
    vs = warm.read_census([os.path.join(os.path.dirname(os.path.abspath(__file__)), "suite_kernels.txt")])
    assert len(vs) > 50 and all(L.qdas_kernel_variant_prebuilt(*v) >= 0 for v in vs)


def test_bench_and_suite_hiprtc_kernels_do_not_spill(tmp_path, monkeypatch):
    """(CPU) "no kernel spills" as a test: EVERY plan-specialised kernel the bench workloads build (tests/jit_kernels.txt: the complete JitSpecs a GPU run
    of tools/jit_specs_collect.sh logged -- the tile shapes are probed on the device, the builds are not) and EVERY on-demand variant the GPU suite launches
    (tests/suite_kernels.txt) is rebuilt here without a device, one compiler process per core: no spilled VGPR, no scratch, at most 128 registers"""
    from qups_amd import _lib, warm
    L = _lib.lib()
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    here = os.path.dirname(os.path.abspath(__file__))
    specs = warm.read_specs([os.path.join(here, "jit_kernels.txt")])
    assert len(specs) >= 20
    cache = tmp_path / "jit"
    cache.mkdir()
    jobs = max(1, min(os.cpu_count() or 4, 16))
    if warm.warm_specs(specs[:1], str(cache), jobs=1):
        L.qdas_kernel_variant_build(2, 5, 1, 1)
        if b"hiprtc not available" in (L.qdas_last_error() or b""):
            pytest.skip("hiprtc not available")
        raise AssertionError("the first spec of tests/jit_kernels.txt does not build")
    assert warm.warm_specs(specs[1:], str(cache), jobs=jobs, quiet=False) == 0
    # the suite's on-demand variants (the prebuilt ones are covered by tests/test_build_regs.py)
    monkeypatch.setenv("QDAS_CACHE_DIR", str(cache))
    monkeypatch.setenv("QDAS_VARIANT_CACHE_DIR", str(cache))
    vs = [v for v in warm.read_census([os.path.join(here, "suite_kernels.txt")]) if L.qdas_kernel_variant_prebuilt(*v) == 0]
    assert len(vs) > 50
    assert warm.warm(vs, jobs=jobs) == 0
    sys.path.insert(0, os.path.join(root, "tools"))
    import kernel_regs
    rows = [r for fn in sorted(os.listdir(cache)) if fn.endswith(".hsaco") for r in kernel_regs.kernel_table(str(cache / fn))]
    assert len(rows) >= len(set(specs)) + len(vs) - 2, (len(rows), len(specs), len(vs))
    bad = [(r["name"], r["vgpr"], r["vgpr_spill"], r["scratch"]) for r in rows if r["vgpr_spill"] != 0 or r["vgpr"] + r["agpr"] > 128]
    assert not bad, bad
    # The plan-specialised builds of the GPU SUITE (tests/suite_jit_kernels.txt): a build that uses any scratch memory is refused at run time (csrc/jit.hip
    # scratch_refusal: 0 bytes for a plan-specialised build -- its plan runs the stock kernel), so a spill there is a silent loss of the specialisation, not
    # an error.  The three that do are known (round 6); a fourth would show up here.
    known = {"qdas_jit_tile__linear_f32_fmod_mirror_mb16_w192_n8_m16_t452", "qdas_jit_tile__lanczos3_f32_lut_fmod_mirror_mb32_w128_n1_m32_t268",
             "qdas_jit_tile__linear_f32_lut_fmod_mirror_mb32_w128_n2_m32_t534"}
    suite = tmp_path / "suite_jit"
    suite.mkdir()
    sspecs = warm.read_specs([os.path.join(here, "suite_jit_kernels.txt")])
    assert warm.warm_specs(sspecs, str(suite), jobs=jobs, quiet=True) == 0
    srows = [r for fn in sorted(os.listdir(suite)) if fn.endswith(".hsaco") for r in kernel_regs.kernel_table(str(suite / fn))]
    spilling = {r["name"] for r in srows if r["vgpr_spill"] != 0 or r["scratch"] > 0}
    assert spilling <= known, sorted(spilling - known)
    # a private segment without a spilled register is tolerated only when NO instruction touches it (a dead stack slot of the 2-tap weight array: one
    # on-demand variant of the table-driven kernel has one)
    objdump = "/opt/rocm/lib/llvm/bin/llvm-objdump"
    for fn in sorted(os.listdir(cache)):
        if not fn.endswith(".hsaco"):
            continue
        rs = kernel_regs.kernel_table(str(cache / fn))
        if any(r["scratch"] != 0 for r in rs):
            dis = subprocess.run([objdump, "-d", str(cache / fn)], capture_output=True, text=True).stdout
            assert "scratch_" not in dis and "buffer_store" not in dis, (fn, rs)


@pytest.mark.gpu
@pytest.mark.parametrize("seq,interp,prec,fmod", [("PW", "cubic_dev", "single", 0.0), ("FSA", "linear", "single", 2.5e6), ("DV", "linear", "halfT", 2.5e6)])
def test_on_demand_variant_runs_and_matches_oracle(seq, interp, prec, fmod, tmp_path, monkeypatch):
    """a plan whose instantiation libqdas.so does not carry builds it at plan creation (never inside an execute), says so in its kernel name, and
    matches the oracle and the generic kernel"""
    import torch
    from oracle import das_oracle as O
    from qups_amd import DasPlan, build_problem, parse_options
    monkeypatch.setenv("QDAS_CACHE_DIR", str(tmp_path))
    case = make_case(seq=seq, interp=interp if interp != "cubic_dev" else "cubic", seed=57, N=16, I1=150, I2=36)
    x = torch.from_numpy(case["x"])
    fm = float(np.float32(fmod))
    va = list(case["opt"]) + ["interp", interp, "input-precision", prec, "modulation", fm]
    prob = build_problem("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], case["x"].shape, case["t0"], case["fs"], case["c"], parse_options(x, va))
    out = {}
    for kernel in (2, 1):
        with DasPlan(prob, kernel=kernel) as plan:
            y = plan.feval(x)
            out[kernel] = (torch.view_as_real(y).float().cpu().numpy().view(np.complex64)[..., 0] if prec == "halfT" else y.cpu().numpy()).reshape(-1)
            if kernel == 2:
                name = plan.kernel_name()
                assert plan.kernel == "tiled" and "[built on demand " in name, name
    tol = 2e-3 if prec == "halfT" else 2e-4 if fm else 2e-5
    assert rel_err(out[2], out[1]) <= tol
    if interp != "cubic_dev":
        ref = O.das_spec("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], case["x"], case["t0"], case["fs"], cinv_f32(case["c"]),
                         VS=case["VS"], DV=case["DV"], interp=interp, fmod=fm).reshape(-1, order="F")
        assert rel_err(out[2], ref) <= (1e-2 if interp == "nearest" else tol)


@pytest.mark.gpu
def test_without_a_compiler_on_demand_variants_run_the_generic_kernel(tmp_path, monkeypatch):
    """QDAS_NO_LAZY=1 stands for a host without libhiprtc.so: a plan that needs a variant libqdas.so does not carry is made on the generic kernel (and
    says why), a QDAS_KERNEL_TILED request fails with QDAS_EUNSUPPORTED; a stream of frames whose two-frame variant cannot be built runs one frame per launch"""
    import torch
    from qups_amd import DasPlan, build_problem, parse_options, _lib
    from qups_amd.das_spec import _colmajor
    monkeypatch.setenv("QDAS_CACHE_DIR", str(tmp_path))
    case = make_case(seq="PW", interp="cubic", seed=58, N=16, M=12, I1=128, I2=24)
    x = torch.from_numpy(case["x"])
    va = list(case["opt"]) + ["interp", "cubic_dev"]
    prob = build_problem("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], case["x"].shape, case["t0"], case["fs"], case["c"], parse_options(x, va))
    with DasPlan(prob, kernel=2, mirror=False) as plan:
        y_ref = plan.feval(x).cpu().numpy()
    monkeypatch.setenv("QDAS_CACHE_DIR", str(tmp_path / "other"))          # (this process has the variant in memory: another one is needed)
    va2 = list(case["opt"]) + ["interp", "cubic_dev", "modulation", float(np.float32(1e6))]
    prob2 = build_problem("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], case["x"].shape, case["t0"], case["fs"], case["c"], parse_options(x, va2))
    monkeypatch.setenv("QDAS_NO_LAZY", "1")
    with pytest.raises(_lib.QdasError) as ei:
        DasPlan(prob2, kernel=2, mirror=False)
    assert ei.value.code == 2 and "built on demand" in str(ei.value)
    with DasPlan(prob2, kernel=0, mirror=False) as plan:
        assert plan.kernel == "generic"
    # streams: PW + cubic + fp32 is prebuilt one frame per launch (cfg 0) and two per launch (cfg 3); cubic_dev's two-frame variant is not
    F = 3
    rng = np.random.default_rng(4)
    xs = np.stack([case["x"]] + [(rng.standard_normal(case["x"].shape) + 1j * rng.standard_normal(case["x"].shape)).astype(np.complex64) for _ in range(F - 1)], axis=3)
    xt = torch.from_numpy(xs)
    prob3 = build_problem("DAS", case["Pi"], case["Pr"], case["Pv"], case["Nv"], tuple(xt.shape), case["t0"], case["fs"], case["c"], parse_options(xt, va))
    monkeypatch.delenv("QDAS_NO_LAZY")
    plan = DasPlan(prob3, kernel=2, mirror=False)                            # (the one-frame variant: in memory since the first plan)
    monkeypatch.setenv("QDAS_NO_LAZY", "1")
    ys = plan.execute_colmajor(_colmajor(xt.cuda()), F).cpu().numpy().reshape(F, -1)
    plan.close()
    assert rel_err(ys[0], y_ref.reshape(-1)) <= 1e-6
    assert rel_err(ys[1], ys[0]) > 1e-2
