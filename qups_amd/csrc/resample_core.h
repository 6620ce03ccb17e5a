// resample_core.h -- the index arithmetic of resample.hip: the polyphase split of the taps, the span of inputs a tile of outputs reads, the zero and
// odd-reflection rule as an index map, the LDS address map, the tile choice and the LDS byte count.  Plain C++ with no HIP in it: the same text compiles for
// the host, where tests/resample_core_host.cpp walks the kernel's loops on the CPU under the sanitizers (every LDS block a heap block of exactly its size).
//
// THE CONTRACT.  out[j] = sum_i h[off + j q - i p] X[i], over every integer i with 0 <= off + j q - i p < K.
// THE SPLIT.  With n = off + j q, d = n div p and phi = n mod p the sum is sum_m h[phi + m p] X[d - m]: phase phi has the taps m = 0 .. (K-1-phi)/p, a phase
// phi >= K has none.  Mmax = (K-1)/p is the longest phase's last tap and rem = (K-1) mod p: phase phi ends at m = Mmax - (phi > rem) -- no division per output.
//
// THE TILE.  A workgroup owns TJ consecutive outputs j0 .. j0 + nj - 1 (nj = min(TJ, J - j0)) of one trace.  With d0 = (off + j0 q) div p they read the SPAN
// X[d0 - Mmax .. d_hi], d_hi = (off + (j0 + nj - 1) q) div p: at most ceil((TJ-1) q / p) + Mmax + 1 samples.  TJ is a power of two: the largest of 1024 .. 64
// whose taps and span take at most LDS_PREF = 40 KiB (four workgroups on a CU's 160 KiB); a rate that needs more per output (q/p large) takes the largest of
// 64 .. 1 that fits LDS_MAX = 64 KiB; a call that does not fit with one output per workgroup is refused.
//
// THE LDS MAP.  Taps first: tap m of phase phi at real word phi + m p -- the taps' own order, exactly K words.  At one m the lanes of a wave read the words
// of their phases: different phases below 32 are different banks; two phases 32 apart collide (p > 32 only).  Rows per phase at an odd pitch would collide
// for exactly the same pairs of phases (an odd pitch is invertible mod 32) and cost up to half the table in padding, so there are none.  Then, 16-byte
// aligned, the span: X[d0 - Mmax + e] at element e.
//
// THE EDGE.  ZERO: X[i] = 0 outside 0 <= i < T.  ODD: X[-i] = 2 x[0] - x[i], X[T-1+i] = 2 x[T-1] - x[T-1-i] for 1 <= i <= T-1; the entry refuses a call
// whose outputs read beyond that (reach()), so a span element beyond it is read by no output and is staged as zero, never loaded.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define QDAS_RS_HD __host__ __device__ inline
#else
#define QDAS_RS_HD inline
#endif

namespace qdas {
namespace rs {

constexpr int WAVE = 64;
constexpr int LANES_MAX = 256;            // lanes per workgroup: min(max(TJ, 64), 256)
constexpr int TILE_MAX = 1024;            // outputs per workgroup, at most (four per lane)
constexpr int TILE_WAVE = 64;             // the smallest tile that fills a wave
constexpr int64_t MAX_K = 8192, MAX_PQ = 4096;
constexpr uint32_t LDS_MAX = 65536;       // bytes of dynamic LDS a launch may ask for without an attribute
constexpr uint32_t LDS_PREF = 40960;      // what a tile of 64 outputs or more is held to
constexpr int EDGE_ZERO = 0, EDGE_ODD = 1;

struct Geom {
    int32_t S;          // phases that have taps: min(p, K)
    int32_t Mmax;       // last tap of the longest phase: (K-1) / p
    int32_t rem;        // (K-1) mod p: phases above it end one tap earlier
    int32_t TJ;         // outputs per workgroup (0: does not fit)
    int32_t lanes;      // lanes per workgroup
    int32_t span;       // span elements of a full tile
    uint32_t tap_bytes; // K reals, rounded up to 16 bytes
    uint32_t lds_bytes; // taps + span
};

QDAS_RS_HD uint64_t resample_len(uint64_t T, uint64_t p, uint64_t q) {                    // ceil(T p / q)
    if (!q) return 0;
    const unsigned __int128 v = (unsigned __int128)T * p;
    return (uint64_t)((v + q - 1) / q);
}
QDAS_RS_HD uint64_t upfirdn_len(uint64_t T, uint64_t K, uint64_t p, uint64_t q) {         // ceil(((T-1) p + K) / q)
    if (!q || !T) return 0;
    const unsigned __int128 v = (unsigned __int128)(T - 1) * p + K;
    return (uint64_t)((v + q - 1) / q);
}

// last tap m of phase phi (-1: the phase has no taps)
QDAS_RS_HD int32_t last_tap(int32_t Mmax, int32_t rem, int32_t phi) { return Mmax - (phi > rem); }

// span elements of a tile of nj outputs at most: ceil((nj-1) q / p) + Mmax + 1
QDAS_RS_HD int64_t span_len(int64_t nj, int64_t K, int64_t p, int64_t q) { return ((nj - 1) * q + p - 1) / p + (K - 1) / p + 1; }

QDAS_RS_HD uint32_t lds_need(int64_t TJ, int64_t K, int64_t p, int64_t q, int elem_bytes, uint32_t tap_bytes) {
    const int64_t v = (int64_t)tap_bytes + span_len(TJ, K, p, q) * elem_bytes;
    return v > 0x7fffffff ? 0x7fffffffu : (uint32_t)v;
}

// elem_bytes: one staged sample (4 | 8 | 16); real_bytes: one tap (4 | 8).  1 <= K <= MAX_K, 1 <= p, q <= MAX_PQ.
QDAS_RS_HD Geom geometry(int64_t K, int64_t p, int64_t q, int elem_bytes, int real_bytes) {
    Geom g;
    g.S = (int32_t)(p < K ? p : K);
    g.Mmax = (int32_t)((K - 1) / p);
    g.rem = (int32_t)((K - 1) % p);
    g.tap_bytes = (uint32_t)((K * real_bytes + 15) / 16 * 16);
    g.TJ = 0;
    for (int tj = TILE_MAX; tj >= TILE_WAVE && !g.TJ; tj >>= 1)
        if (lds_need(tj, K, p, q, elem_bytes, g.tap_bytes) <= LDS_PREF) g.TJ = tj;
    for (int tj = TILE_WAVE; tj >= 1 && !g.TJ; tj >>= 1)
        if (lds_need(tj, K, p, q, elem_bytes, g.tap_bytes) <= LDS_MAX) g.TJ = tj;
    g.lanes = g.TJ < WAVE ? WAVE : (g.TJ > LANES_MAX ? LANES_MAX : g.TJ);
    g.span = g.TJ ? (int32_t)span_len(g.TJ, K, p, q) : 0;
    g.lds_bytes = g.TJ ? lds_need(g.TJ, K, p, q, elem_bytes, g.tap_bytes) : 0;
    return g;
}

// real word of tap m of phase phi
QDAS_RS_HD int32_t tap_word(int32_t phi, int32_t m, int32_t p) { return phi + m * p; }

// a tile's extent: d0 = (off + j0 q) div p and f0 = (off + j0 q) mod p (THE 64-bit division of the tile), the first span index and the elements staged
struct Tile { int64_t d0; int32_t f0; int64_t i_lo; int32_t len; };
QDAS_RS_HD Tile tile_extent(int64_t off, int64_t j0, int32_t nj, int32_t p, int32_t q, int32_t Mmax) {
    Tile t;
    const int64_t n0 = off + j0 * q;
    t.d0 = n0 / p;
    t.f0 = (int32_t)(n0 - t.d0 * p);
    t.i_lo = t.d0 - Mmax;
    t.len = (int32_t)(((uint32_t)t.f0 + (uint32_t)(nj - 1) * (uint32_t)q) / (uint32_t)p) + Mmax + 1;      // f0 + 1023 * 4096 < 2^23
    return t;
}

// lane t's first output j0 + t: its phase and b = d - d0 (one 32-bit division per lane; the outputs behind it advance by carries: advance())
QDAS_RS_HD void lane_start(int32_t f0, int32_t t, int32_t p, int32_t qd, int32_t qm, int32_t &b, int32_t &phi) {
    const uint32_t v = (uint32_t)f0 + (uint32_t)t * (uint32_t)qm;
    const uint32_t c = v / (uint32_t)p;
    phi = (int32_t)(v - c * (uint32_t)p);
    b = t * qd + (int32_t)c;
}
// (b, phi) += (sd, sm) with sd = (step q) div p, sm = (step q) mod p
QDAS_RS_HD void advance(int32_t &b, int32_t &phi, int32_t sd, int32_t sm, int32_t p) {
    b += sd; phi += sm;
    if (phi >= p) { phi -= p; ++b; }
}

// THE EDGE RULE as an index map.  X[i] = x[src] when anchor < 0, 2 x[anchor] - x[src] otherwise; src = -1: zero, nothing is loaded.
QDAS_RS_HD int64_t edge_source(int64_t i, int64_t T, int edge, int64_t &anchor) {
    anchor = -1;
    if (i >= 0 && i < T) return i;
    if (edge != EDGE_ODD) return -1;
    if (i < 0) { if (-i > T - 1) return -1; anchor = 0; return -i; }
    if (i > 2 * (T - 1)) return -1;
    anchor = T - 1;
    return 2 * (T - 1) - i;
}

QDAS_RS_HD int64_t floor_div(int64_t a, int64_t b) { const int64_t c = a / b; return c - ((a % b != 0) && ((a < 0) != (b < 0))); }

// the lowest and highest index any output reads: output j reads i = ceil((n - K + 1) / p) .. floor(n / p), n = off + j q, when that range is not empty.
// Both ends grow with j, and the phases repeat after at most p outputs: the first and the last output with taps are among the first and last p.
// false: no output reads anything (every phase met is >= K).
QDAS_RS_HD bool reach(int64_t off, int64_t J, int64_t p, int64_t q, int64_t K, int64_t &lo, int64_t &hi) {
    bool any = false;
    const int64_t look = J < p ? J : p;
    for (int64_t j = 0; j < look && !any; ++j) {
        const int64_t n = off + j * q, a = -floor_div(-(n - K + 1), p), b = floor_div(n, p);
        if (a <= b) { lo = a; any = true; }
    }
    if (!any) return false;
    for (int64_t j = J - 1; j >= J - look; --j) {
        const int64_t n = off + j * q, a = -floor_div(-(n - K + 1), p), b = floor_div(n, p);
        if (a <= b) { hi = b; break; }
    }
    return true;
}

}  // namespace rs
}  // namespace qdas
