// demod_core.h -- the index and phase arithmetic of demod.hip: the polyphase split of the taps, the extent of the input span a tile stages, the zero-fill
// rule, the LDS address map and the float64 phase reductions.  Plain C++ with no HIP in it: the same text compiles for the host, where
// tests/demod_core_host.cpp walks the kernel's loops on the CPU under the sanitizers (every LDS block a heap block of exactly its size).
//
// THE SPLIT.  out[j] = sum_k h[k] x[jR - k] with k = mR + s, s = k mod R: phase s in [0, S), S = min(R, K), has the taps m = 0 .. (K-1-s)/R and reads the
// ROW x_s[n] = x[nR - s] at n = j - m -- a stride-1 FIR per phase.  Samples of a phase s >= S (K < R) are read by no output and are never loaded.
//
// THE TILE.  A workgroup of LANES lanes owns TILE = LANES * OPL consecutive outputs j0 .. j0 + TILE - 1 of one trace; lane t owns outputs j0 + OPL t + r.
// Taps go in groups of OPL: NG = Mmax / OPL + 1 groups cover m = 0 .. Mmax = (K-1)/R.  A row holds n = j0 - OPL NG .. j0 + TILE - 1, EN = OPL (NG + LANES)
// elements; element e (n = j0 - OPL NG + e) of the row of phase s is sample i = n R - s, ZERO when i < 0 (the causal start) or i >= T (never x_ld padding).
//
// THE LDS MAP.  Rows are de-interleaved by (e mod OPL): element e of the d-th staged phase lives at word (d OPL + (e mod OPL)) QP + e / OPL.  In the tap loop
// lane t reads plane w at quad NG + t - g: the lanes of a wave read consecutive elements -- conflict-free for 4-, 8- and 16-byte elements alike.  QP, the
// padded plane length, is the smallest value >= NG + LANES with QP = 2 (mod 32) for 4-byte elements and QP = 1 (mod 16) for wider ones: the staging stores of
// a wave (lanes along the global index: the phases of one n, then the next n) then spread over the banks -- exactly for R = 4 (the 16 planes a 32-lane group
// touches start 2 words apart, each takes 2 of them), at most two-way for the other ratios up to PG_MAX, which a store's own issue time covers.
// At most PG_MAX phases are staged at a time (R <= PG_MAX: the whole span in one coalesced sweep); more phases go in groups.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define QDAS_DM_HD __host__ __device__ inline
#else
#define QDAS_DM_HD inline
#endif

namespace qdas {
namespace dm {

constexpr int LANES = 64;                 // one wave per workgroup
constexpr int OPL = 4;                    // outputs per lane = taps per group
constexpr int TILE = LANES * OPL;         // outputs per workgroup
constexpr int PG_MAX = 8;                 // phases staged at a time
constexpr int64_t MAX_K = 1024, MAX_R = 4096;
constexpr uint32_t LDS_MAX = 65536;       // bytes of dynamic LDS a launch may ask for without an attribute

struct Geom {
    int32_t S;          // phases that have taps: min(R, K)
    int32_t NG;         // tap groups
    int32_t QP;         // padded plane length, elements
    int32_t EN;         // row elements staged per phase
    int32_t PG;         // phases per staging group (0: does not fit)
    uint32_t tap_bytes; // the modulated taps, K complex values, rounded up to 16 bytes
    uint32_t lds_bytes; // taps + PG rows; at least TILE complex values behind the taps (the epilogue's transpose)
};

QDAS_DM_HD uint64_t out_len(uint64_t T, uint64_t R) { return R ? T / R + (T % R != 0) : 0; }

// taps of phase s: m = 0 .. last_tap(K, R, s)   (s < min(R, K))
QDAS_DM_HD int32_t last_tap(int64_t K, int64_t R, int64_t s) { return (int32_t)((K - 1 - s) / R); }

QDAS_DM_HD int32_t plane_len(int32_t quads, int elem_bytes) {
    const int mod = elem_bytes == 4 ? 32 : 16, want = elem_bytes == 4 ? 2 : 1;
    return quads + ((want - quads % mod) % mod + mod) % mod;
}

// the epilogue's transpose: output e of the tile (lane e / OPL, r = e mod OPL) at complex word (e mod OPL) out_plane + e / OPL; the plane length keeps both the
// lane-major stores and the output-major loads off each other's banks (72: 8-byte values, 68: 16-byte values)
QDAS_DM_HD int32_t out_plane(int cplx_bytes) { return cplx_bytes == 8 ? 72 : 68; }
QDAS_DM_HD int32_t out_word(int32_t e, int cplx_bytes) { return (e & (OPL - 1)) * out_plane(cplx_bytes) + (e >> 2); }

// elem_bytes: one staged sample (4 | 8 | 16); cplx_bytes: one complex value of the compute precision (8 | 16)
QDAS_DM_HD Geom geometry(int64_t K, int64_t R, int elem_bytes, int cplx_bytes) {
    Geom g;
    g.S = (int32_t)(R < K ? R : K);
    g.NG = (int32_t)((K - 1) / R) / OPL + 1;
    g.QP = plane_len(g.NG + LANES, elem_bytes);
    g.EN = OPL * (g.NG + LANES);
    g.tap_bytes = (uint32_t)((K * cplx_bytes + 15) / 16 * 16);
    const uint32_t row = (uint32_t)OPL * (uint32_t)g.QP * (uint32_t)elem_bytes;
    int64_t pg = g.tap_bytes < LDS_MAX ? (LDS_MAX - g.tap_bytes) / row : 0;
    if (pg > PG_MAX) pg = PG_MAX;
    if (pg > g.S) pg = g.S;
    g.PG = (int32_t)pg;
    uint32_t body = (uint32_t)g.PG * row;
    const uint32_t tr = (uint32_t)(OPL * out_plane(cplx_bytes) * cplx_bytes);
    if (body < tr) body = tr;
    g.lds_bytes = g.tap_bytes + body;
    return g;
}

// word (in elements) of element e of the d-th staged phase
QDAS_DM_HD int32_t lds_word(int32_t d, int32_t e, int32_t QP) { return (d * OPL + (e & (OPL - 1))) * QP + (e >> 2); }

// global sample index of element e of phase s in the tile whose first output is j0; the element is zero unless 0 <= index < T
QDAS_DM_HD int64_t sample_index(int64_t j0, int32_t NG, int32_t e, int64_t R, int32_t s) { return (j0 - (int64_t)OPL * NG + e) * R - s; }

// the quad lane t reads in tap group g: its window entry w (-OPL .. OPL-1; output r, tap u of the group uses w = r - u) is row element OPL quad + (w mod OPL).
// The kernel and the host program both take their quads from here; the kernel unrolls two groups per trip (even groups load the lower half of its eight
// registers, odd groups the upper), the host program takes one group per trip with the same halves and the same rotation.
QDAS_DM_HD int32_t window_quad(int32_t NG, int32_t t, int32_t g, int32_t w) { return NG + t - g - (w < 0); }

// ---- phases, in cycles, reduced in float64
QDAS_DM_HD double frac(double v) { return v - floor(v); }
QDAS_DM_HD double centred(double cyc) { return cyc >= 0.5 ? cyc - 1.0 : cyc; }                                      // [0, 1] -> [-1/2, 1/2], the same angle
QDAS_DM_HD double tap_cycles(int64_t k, double fc_over_fs) { return frac((double)k * fc_over_fs); }                 // tap k is b[k] exp(+2 pi i tap_cycles)
QDAS_DM_HD double out_cycles(double cyc0, int64_t j, double step) { return frac(cyc0 + frac((double)j * step)); }   // output j is exp(-2 pi i out_cycles) * sum

}  // namespace dm
}  // namespace qdas
