// das_tile_cfg.h -- launch configurations of the tiled kernel, shared by its translation units (internal).
#pragma once
// elements per pass of the prologue's tile-wide reductions (LDS scratch = 2 * waves * min(max(N, M), chunk) floats, aliasing the windows)
#define QDAS_PROLOGUE_CHUNK 512u
namespace qdas {
// ------------------------------------------------------------------------------------------
// Launch configurations: ONE row per configuration number, and everything a number means is a field of its row.  The kernel template is instantiated
// from a row (das_tile_impl.h launch_tile_i; jit.hip lazy_tile_source writes the same arguments for hiprtc), select_cfg() below is the only place that
// turns a launch into a number, and libqdas.so compiles das_tile_inst.hip once per row that has a translation unit (Makefile TILE_CFGS).
struct Cfg {
    int waves, mb, w, nbuf, psz, bpc;      // stage shape: waves per workgroup, transmits per stage, samples per window, window buffers, bytes per DMA piece, workgroups per CU
    int bytes;                             // of one sample: 4 (fp16 pairs), 8 (fp32), 16 (fp64)
    int frames;                            // frames per launch: 1 | 2 | 4 (general mode, 2: also the two window sets of a lateral-mirror plan's single frame)
    bool sym, mirq, fold, big, lut, bfm;   // reciprocal mode; + lateral mirror; reciprocity-folded data; descriptor re-basing; table-driven delays; 'BF'
    bool tu;                               // libqdas.so has a translation unit for it (false: hiprtc-specialised builds only)
};
constexpr int NCFG = 22;
constexpr int CFG_NONE = -1;
static constexpr Cfg CFGS[NCFG] = {
    //                          bytes frames sym mirq fold big lut bfm  tu
    {16, 32, 192, 2, 16, 1,      8,   1,    0,  0,   0,   0,  0,  0,   1},   // 0   general case: 16-wave workgroup = 64 x 16 pixel tile, 32 transmits per stage, 2 window buffers, one workgroup per CU
    {16, 16, 192, 2, 16, 1,      8,   1,    1,  0,   0,   0,  0,  0,   0},   // 1   reciprocal mode: the same tile with 16 transmits per stage and direct + mirror windows
    {16, 32, 384, 2, 16, 1,      4,   1,    0,  0,   0,   0,  0,  0,   1},   // 2   fp16 data, general
    {16, 16, 192, 2, 16, 1,      8,   2,    0,  0,   0,   0,  0,  0,   1},   // 3   two frames per launch: 16 transmits x 2 frames per stage -- the reciprocal mode's window layout
    {16, 16, 384, 2, 16, 1,      4,   2,    0,  0,   0,   0,  0,  0,   1},   // 4   ... fp16 data
    {16,  8, 192, 2, 16, 1,      8,   4,    0,  0,   0,   0,  0,  0,   1},   // 5   four frames per launch: 8 transmits x 4 frames per stage
    {16,  8, 384, 2, 16, 1,      4,   4,    0,  0,   0,   0,  0,  0,   1},   // 6   ... fp16 data
    {16, 16, 128, 2, 16, 1,      8,   1,    1,  0,   0,   0,  0,  0,   0},   // 7   reciprocal mode with 128-sample windows (a third less staging traffic; used when every tile of some footprint fits them)
    {16, 16, 256, 2, 16, 1,      4,   1,    1,  0,   0,   0,  0,  0,   1},   // 8   reciprocal mode for fp16 data (256-sample windows = one 1024-byte DMA piece, like 7)
    {16, 32, 192, 2, 16, 1,      8,   1,    0,  0,   0,   1,  0,  0,   1},   // 9   0 with descriptor re-basing (transposed fp32 frames beyond 2 GiB)
    {16, 32, 192, 2, 16, 1,      8,   1,    0,  0,   0,   0,  1,  0,   1},   // 10  0 with table-driven delays (the split-delay flavour: qdas_das_lut)
    {16, 32, 384, 2, 16, 1,      4,   1,    0,  0,   0,   0,  1,  0,   1},   // 11  2 (fp16 data) with table-driven delays
    {16, 32, 192, 2, 16, 1,      8,   1,    0,  0,   0,   0,  0,  1,   1},   // 12  0 keeping BOTH aperture dimensions ('BF': one output plane per (receiver, transmit) pair, nothing is summed)
    {16, 16, 192, 2, 16, 1,     16,   1,    0,  0,   0,   0,  0,  0,   1},   // 13  fp64 data: 16 transmits per stage, 192-sample windows -- the LDS image of 0
    {16, 16, 384, 2, 16, 1,      8,   1,    0,  0,   0,   0,  0,  0,   1},   // 14  fp32 data with 384-sample windows and 16 transmits per stage (the LDS image of 0): the second attempt of a plan whose
                                                                             //     tiles do not fit 192 samples -- pixel grids coarser than about lambda/2 (volumes, previews), steep delay gradients
    {16, 16, 128, 2, 16, 1,      8,   1,    1,  1,   0,   0,  0,  0,   0},   // 15  reciprocal + lateral-mirror mode: FOUR window sets of 16 one-KiB windows per buffer -- the LDS image of the 32-transmit reciprocal stages hiprtc builds run
    {16, 16, 256, 2, 16, 1,      4,   1,    1,  1,   0,   0,  0,  0,   1},   // 16  ... fp16 data
    {16, 32, 128, 2, 16, 1,      8,   1,    1,  1,   1,   0,  0,  0,   1},   // 17  reciprocity-FOLDED fp32 data (TileCfg::FOLD, fold.hip) with the lateral-mirror mode: TWO window sets of 32 one-KiB windows (the LDS image of 15)
    {16, 16, 192, 2, 16, 1,      8,   1,    1,  1,   1,   0,  0,  0,   1},   // 18  ... of 16 192-sample windows: tiles that do not fit 128 samples
    {16, 32, 192, 2, 16, 1,      8,   1,    1,  0,   1,   0,  0,  0,   1},   // 19  folded data without the mirror mode: ONE set of 32 192-sample windows (the LDS image of 0)
    {16, 16, 128, 2, 16, 1,      8,   2,    1,  1,   1,   0,  0,  0,   1},   // 20  two FRAMES of folded data per launch, mirror mode: four window sets of 16 one-KiB windows (the LDS image of 15)
    {16, 16, 192, 2, 16, 1,      8,   2,    1,  0,   1,   0,  0,  0,   1},   // 21  ... without the mirror mode: two sets of 16 x 192
};
// THE selector: which configuration a launch runs (CFG_NONE: there is none).  First match wins.  The arguments are what plan_modes.h launch_legal derives:
// nf: frames per launch (1 | 2 | 4; 2 also for the single frame of a general-mode lateral-mirror plan)
// narrow: window variant -- 1: reciprocal mode with 128-sample windows; 2: general mode, fp32 data, 384-sample windows
// mirq: reciprocal + lateral-mirror mode (sym && mir && !probe);  fold: reciprocity-folded fp32 data (sym && fold && fp32)
// probe: the plan-time window-fit test (prologue only, one frame): every fp32 reciprocal plan probes with the folded rows (the same prologue; 128- or
//        192-sample windows), 'BF' and re-basing plans with row 0, table-driven plans with their own rows
constexpr int select_cfg(int dtype, int sym, int nf = 1, int narrow = 0, int mirq = 0, int fold = 0, int big = 0, int lut = 0, int bf = 0, int probe = 0) {
    const bool f16 = dtype == 2, f32 = dtype == 1;
    if (dtype == 0) return 13;
    if (sym && f32 && (fold || probe)) {
        if (probe) return narrow ? 17 : 19;
        if (nf == 2) return !mirq ? 21 : narrow ? 20 : CFG_NONE;      // (two frames in mirror mode: four window sets, which only the 128-sample windows leave room for)
        if (nf > 2) return CFG_NONE;
        return !mirq ? 19 : narrow ? 17 : 18;
    }
    if (lut) return f16 ? 11 : 10;
    if (sym && f16) return mirq ? 16 : 8;
    if (sym) return mirq ? 15 : narrow ? 7 : 1;                        // (fp32 without the fold: rows without a translation unit -- a hiprtc build's stage shape)
    if (nf == 4) return f16 ? 6 : 5;
    if (nf == 2) return f16 ? 4 : 3;
    if (f16) return 2;
    if (narrow == 2) return 14;
    if (bf && !probe) return 12;
    if (big && !probe) return 9;
    return 0;
}
// the row whose STAGE SHAPE a plan-level mode has (plan_modes.h tile_config / tile_lds_bytes, plan-specialised builds): the selector without a launch in hand.
// fb: frames per launch (1 | 2 | 4).  Always a row: folded data has rows for one and for two frames (any other count: the one-frame row's shape), and two
// frames in mirror mode have the narrow-window row only.
constexpr int cfg_index(int dtype, int sym, int fb = 1, int narrow = 0, int mirq = 0, int fold = 0) {
    if (fold && sym && dtype == 1) { fb = fb == 2 ? 2 : 1; if (fb == 2 && mirq) narrow = 1; }
    return select_cfg(dtype, sym, fb, narrow, mirq, fold);
}
// ------------------------------------------------------------------------------------------
// Which points of the template's matrix libqdas.so carries.  Everything else is built on demand by hiprtc from the same template arguments (jit.hip
// lazy_tile_launch; ~2 s once per variant and machine, cached on disk) -- the reference builds ALL its kernels per system that way
// (src/UltrasoundSystem.m:5527-5625).  The prebuilt set is what the BASELINE configurations, the benches and the test suite launch
// (QDAS_KERNEL_CENSUS, tools/kernel_census.py: the census of a GPU run of all of them), so that none of those ever waits for a compiler.
// Probe instantiations (the plan-time window-fit test: the prologue only, ~8 KB each) are all prebuilt.
// Row = launch configuration, column = interpolator flag (0 nearest, 1 linear, 2 cubic, 3 lanczos3, 5 cubic_dev), value = mask over the variants
// 1: plain, 2: remodulation, 4: weight table, 8: both.  The set: what `bench.py` launches for C1 ... C5 and its switches (general / reciprocal / mirror,
// frame streams, fp16, fp64, windows; prebuilt and hiprtc-specialised), what __graft_entry__.smoke() launches, plus the plain variant of every
// interpolator on the general fp32 / fp16 configurations and of `cubic` (the reference's default, src/UltrasoundSystem.m:3289) on the folded ones.
// `tools/warm_cache.py` (python -m qups_amd.warm) builds any other set ahead of time, in parallel; tests/conftest.py does so for the GPU suite.
static constexpr unsigned char TILE_PREBUILT[NCFG][6] = {
    {0x1, 0x1, 0x5, 0x7, 0x0, 0x0},   // cfg 0   fp32, general
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0},   // cfg 1   (unfolded fp32 reciprocal: hiprtc-specialised builds only)
    {0x1, 0x1, 0x1, 0x1, 0x0, 0x0},   // cfg 2   fp16, general
    {0x0, 0x1, 0x5, 0x7, 0x0, 0x0},   // cfg 3   fp32, two frames per launch / lateral-mirror mode
    {0x0, 0x0, 0x1, 0x1, 0x0, 0x0},   // cfg 4   fp16, two frames per launch / lateral-mirror mode
    {0x0, 0x1, 0x1, 0x1, 0x0, 0x0},   // cfg 5   fp32, four frames per launch
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0},   // cfg 6   fp16, four frames per launch
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0},   // cfg 7   (as cfg 1)
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0},   // cfg 8   fp16 reciprocal, unfolded (QDAS_PLAN_NO_FOLD)
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0},   // cfg 9   fp32, transposed frames beyond 2 GiB
    {0x0, 0x1, 0x1, 0x1, 0x0, 0x0},   // cfg 10  fp32, table-driven delays (bfDASLUT)
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0},   // cfg 11  fp16, table-driven delays
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0},   // cfg 12  'BF'
    {0x0, 0x0, 0x3, 0x0, 0x0, 0x0},   // cfg 13  fp64
    {0x0, 0x1, 0x0, 0x0, 0x0, 0x0},   // cfg 14  fp32, 384-sample windows
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0},   // cfg 15  (as cfg 1)
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0},   // cfg 16  fp16 reciprocal + mirror, unfolded
    {0x0, 0x0, 0x1, 0x3, 0x0, 0x0},   // cfg 17  folded, mirror, 128-sample windows (the headline: C3)
    {0x0, 0x0, 0x0, 0x0, 0x0, 0x0},   // cfg 18  folded, mirror, 192-sample windows
    {0x0, 0x0, 0x1, 0x3, 0x0, 0x0},   // cfg 19  folded
    {0x0, 0x0, 0x1, 0x1, 0x0, 0x0},   // cfg 20  folded, mirror, two frames per launch
    {0x0, 0x0, 0x1, 0x1, 0x0, 0x0},   // cfg 21  folded, two frames per launch
};
constexpr bool tile_prebuilt(int ci, int interp, bool fm, bool wt, bool probe) {
    if (probe) return true;
    return ((TILE_PREBUILT[ci][interp] >> ((fm ? 1 : 0) + (wt ? 2 : 0))) & 1) != 0;
}
}  // namespace qdas
