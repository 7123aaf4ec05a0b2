// agc_track.hpp -- the AGCBank's level tracker in integers, for host and device
// (include/ldsp.h has the definition).  Levels are int32 in units of 2^-24 octave
// of amplitude, between kAgcFloor and kAgcCeil.  For a row's blocks b = 0, 1, ..
//   w_b = max(peak_q[b - H .. b])                       (blocks before the stream: kAgcFloor)
//   L_b = max(w_b, L_{b-1} - d, kAgcFloor),  L_{-1} = kAgcFloor
// The recursion is a scan of the pairs (w_b, 1) under
//   (v1, n1) o (v2, n2) = (max(v1 - n2 d, v2), n1 + n2)
// whose values never fall below kAgcFloor (every w does not), so the one
// product n2 d is the only term that leaves int32; it is taken in int64.  The
// operator is associative and has no rounding: every partition of a row's
// blocks gives the same L.  k_agcbank_track spreads a row over the lanes of a
// workgroup with these functions; agc_track_partitioned() is the same
// evaluation on the host, for any partition width (ldsp_debug_agcbank_track).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>
#ifdef __HIPCC__
#include <hip/hip_runtime.h>
#define LDSP_HD __host__ __device__
#else
#define LDSP_HD
#endif

namespace ldsp {
namespace agc {

constexpr int kAgcQBits = 24;
constexpr double kAgcQ = 16777216.0;                  // units per octave
constexpr int32_t kAgcFloor = -(64 << kAgcQBits);     // -64 octaves
constexpr int32_t kAgcCeil = 64 << kAgcQBits;         // +64 octaves (2^30)
constexpr int kAgcMaxHang = 255;

struct Pair {
    int32_t v;        // the level the segment leaves behind on its own
    int64_t n;        // its length in blocks
};

LDSP_HD inline int32_t agc_max(int32_t a, int32_t b) { return a > b ? a : b; }

// v lowered by n blocks of decay, not below the floor
LDSP_HD inline int32_t agc_decayed(int32_t v, int64_t n, int64_t d)
{
    const int64_t r = (int64_t)v - n * d;
    return r < (int64_t)kAgcFloor ? kAgcFloor : (int32_t)r;
}

// a then b
LDSP_HD inline Pair agc_combine(const Pair& a, const Pair& b, int64_t d)
{
    return Pair{agc_max(agc_decayed(a.v, b.n, d), b.v), a.n + b.n};
}

// The pair of the n window maxima at w (n >= 1)
template <class W>
LDSP_HD inline Pair agc_fold(const W& w, int64_t n, int64_t d)
{
    int32_t v = w[0];
    for (int64_t i = 1; i < n; i++) v = agc_max(agc_decayed(v, 1, d), w[i]);
    return Pair{v, n};
}

// One partition from the level before it: L[i] for its n window maxima; returns the last
template <class W, class O>
LDSP_HD inline int32_t agc_eval(int32_t before, const W& w, int64_t n, int64_t d, O&& out)
{
    int32_t v = before;
    for (int64_t i = 0; i < n; i++) {
        v = agc_max(agc_decayed(v, 1, d), w[i]);
        out(i, v);
    }
    return v;
}

// gain_q = min(T - L, Gmax): T and Gmax lie within +-32 octaves, so the difference stays in int32
LDSP_HD inline int32_t agc_gain_q(int32_t T, int32_t L, int32_t Gmax)
{
    const int32_t g = T - L;
    return g < Gmax ? g : Gmax;
}

// One doubling step of the hang window's running maximum: from m[i] = max of the
// k entries ending at i to the max of the `span` entries ending at i,
// k <= span <= 2 k.  Entries before the array count as the floor.
template <class M>
LDSP_HD inline int32_t agc_window_step(const M& m, int64_t i, int64_t k, int64_t span)
{
    const int64_t j = i - (span - k);
    return agc_max(m[i], j >= 0 ? m[j] : kAgcFloor);
}

// Host evaluation over n new peaks: `tail` holds the H peaks before them, oldest
// first, and receives the last H of the stream; *level is L before and after.
// The blocks are cut into partitions of `width`; each partition's pair is
// folded, the pairs are scanned, and each partition is evaluated from the level
// before it -- what the kernel does with lanes, waves and passes.
inline void agc_track_partitioned(const int32_t* peak_q, size_t n, unsigned H, int64_t d, size_t width, int32_t* level,
                                  int32_t* tail, int32_t* L)
{
    std::vector<int32_t> a(H + n), b(H + n);
    for (unsigned i = 0; i < H; i++) a[i] = tail[i];
    for (size_t i = 0; i < n; i++) a[H + i] = peak_q[i];
    for (unsigned i = 0; i < H; i++) tail[i] = a[n + i];
    const int64_t S = (int64_t)H + 1;
    int64_t k = 1;
    while (k < S) {                                   // the running maximum over H + 1 entries by doubling
        const int64_t span = std::min<int64_t>(2 * k, S);
        for (int64_t i = 0; i < (int64_t)a.size(); i++) b[i] = agc_window_step(a, i, k, span);
        a.swap(b);
        k = span;
    }
    const int32_t* w = a.data() + H;
    const size_t parts = (n + width - 1) / width;
    std::vector<Pair> agg(parts);
    for (size_t p = 0; p < parts; p++)
        agg[p] = agc_fold(w + p * width, (int64_t)std::min(width, n - p * width), d);
    Pair run{*level, 0};                              // the level before the first partition
    for (size_t p = 0; p < parts; p++) {
        const size_t o = p * width;
        agc_eval(run.v, w + o, (int64_t)std::min(width, n - o), d, [&](int64_t i, int32_t v) { L[o + i] = v; });
        run = agc_combine(run, agg[p], d);
    }
    *level = run.v;
}

} // namespace agc
} // namespace ldsp
