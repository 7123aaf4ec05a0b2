// k_sqbank.hip -- per-row level and squelch gate over the rows of a bank
// (SquelchBank): for every row c of a complex64 [C][n] block, the smoothed power
// per block of B samples, liquid's agc squelch state stepped once per block, and
// optionally the rows with the closed blocks zeroed.  The definition is the
// project's own (include/ldsp.h):
//   p[c][b] = (1/B) sum_{i<B} |x[c][bB + i]|^2
//   s[c][b] = s[c][b-1] + alpha (p[c][b] - s[c][b-1])       (float64)
//   level[c][b] = (float) s[c][b];  hi = level[c][b] > thr[c]
//   mode[c][b] = agc_squelch_update_mode(mode[c][b-1], hi), timeout in blocks
//   y[c][bB + i] = mode in {RISE, SIGNALHI, FALL, SIGNALLO} ? x[c][bB + i] : +0
// A row's stream in a call is its `fill` carried samples (the object's history
// buffer) followed by the call's n; the call works on the whole blocks of that
// stream and carries the rest.  Three plain launches, no workgroup waits on
// another:
//
// k_sqbank_power: the grid is (tiles, rows); a workgroup of 256 threads owns
//   T = sqbank_tile(B) consecutive blocks of one row.  G lanes share a block
//   (G: the smallest power of two that holds the block's B / 2 sample pairs, 8 ..
//   64), so a wave sums 64 / G blocks at a time and the 256 / G groups of the
//   workgroup take the tile's blocks round-robin: neighbouring groups read
//   neighbouring memory.  Lane l of a group adds the pairs l, l + G, l + 2G, ..
//   of its block in that order into one float64 (re*re + im*im per sample; the
//   float32 products are exact in float64), each pair one 16-byte load; an odd
//   B's last sample goes to lane (B / 2) mod G after its pairs; the G sums meet in
//   an xor butterfly.  The order depends on B alone, so a block's p has the same
//   bits wherever the block falls in a tile or a call and whatever C is.  Tile 0
//   of each row also writes the row's next carry into the other buffer of the
//   pair.
// k_sqbank_fsm: one lane per row, serial over the call's blocks: the smoothing,
//   the compare on the float32 value stored, the mode step, the stores.  p is
//   loaded eight blocks ahead, so the dependent chain is ALU only.
// k_sqbank_gate (not launched for a measurement): the power kernel's geometry;
//   open blocks are copied 16 bytes per lane, closed ones written as zeros
//   without being read.
#include "kernels.hpp"
#include "ldsp_common.hpp"

namespace ldsp {
namespace k {

namespace {

constexpr int kSqThreads = 256;
constexpr int kSqTileSamples = 8192;          // a tile is about this many samples (64 KiB)
constexpr int kSqAhead = 8;                   // blocks of p the state machine loads ahead

enum { SQ_ENABLED = 1, SQ_RISE, SQ_SIGNALHI, SQ_FALL, SQ_SIGNALLO, SQ_TIMEOUT };   // liquid's codes

// lanes that share a block
constexpr int sq_lanes(int B)
{
    int g = 8;
    while (g < 64 && 2 * g < B) g *= 2;
    return g;
}

struct SqArgs {
    long n, ldx, nblocks;
    int fill, carry;              // carried samples before / after the call
    int B, G, T;
    double invB;                  // 1 / B
};

// two samples side by side (re, im, re, im): 16 bytes at the 8-byte alignment of a complex64 row
typedef float SqVec4 __attribute__((ext_vector_type(4)));
typedef SqVec4 SqPair __attribute__((aligned(8)));

__device__ __forceinline__ double sq_norm(float re, float im)
{
    return (double)re * (double)re + (double)im * (double)im;
}

// Sample g of a row's stream in the call's coordinates: g >= 0 is x[g], g < 0 one of the carried samples
__device__ __forceinline__ float2 sq_one(const float2* __restrict__ xr, const float2* __restrict__ hr, int fill, long g)
{
    if (g >= 0) return xr[g];
    return hr[fill + g];
}
__device__ __forceinline__ SqPair sq_pair(const float2* __restrict__ xr, const float2* __restrict__ hr, int fill, long g)
{
    if (g >= 0) return *reinterpret_cast<const SqPair*>(xr + g);
    const float2 a = hr[fill + g], b = sq_one(xr, hr, fill, g + 1);
    return SqVec4{a.x, a.y, b.x, b.y};
}

__global__ void __launch_bounds__(kSqThreads)
    k_sqbank_power(const SqArgs a, const float2* __restrict__ x, const float2* __restrict__ hist,
                   float2* __restrict__ hist_out, double* __restrict__ p)
{
    const int tid = threadIdx.x;
    const int B = a.B, G = a.G, fill = a.fill;
    const int row = blockIdx.y;
    const float2* __restrict__ xr = x + (long)row * a.ldx;
    const float2* __restrict__ hr = hist + (long)row * B;

    if (blockIdx.x == 0) {                            // the row's next carry: the last a.carry samples of its stream
        float2* __restrict__ ho = hist_out + (long)row * B;
        const long first = a.n - a.carry;             // in the call's coordinates; >= -fill
        for (int i = tid; i < a.carry; i += kSqThreads) ho[i] = sq_one(xr, hr, fill, first + i);
    }
    if (a.nblocks == 0) return;                       // a call too short for a block: state only

    const int l = tid & (G - 1), gi = tid / G, NG = kSqThreads / G;
    const int half = B >> 1;
    const long t0 = (long)blockIdx.x * a.T;
    const SqVec4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int it = 0; it < a.T; it += NG) {
        const long blk = t0 + it + gi;
        const bool valid = blk < a.nblocks;
        const long g0 = blk * B - fill;               // the block's first sample
        double acc = 0.0;
        if (valid) {
            for (int j = l; j < half; j += 4 * G) {
                // four pairs in flight; one past the block's end is read at the last pair's place
                // and counts as +0, so the sum keeps its bits
                SqVec4 v[4];
                if (g0 >= 0) {
#pragma unroll
                    for (int u = 0; u < 4; u++)
                        v[u] = *reinterpret_cast<const SqPair*>(xr + g0 + 2 * min(j + u * G, half - 1));
                } else {                              // the block that starts in the carried samples
#pragma unroll
                    for (int u = 0; u < 4; u++) v[u] = sq_pair(xr, hr, fill, g0 + 2 * min(j + u * G, half - 1));
                }
#pragma unroll
                for (int u = 0; u < 4; u++) {
                    const SqVec4 w = j + u * G < half ? v[u] : zero;
                    acc = acc + sq_norm(w.x, w.y);
                    acc = acc + sq_norm(w.z, w.w);
                }
            }
            if ((B & 1) && l == (half & (G - 1))) {
                const float2 w = sq_one(xr, hr, fill, g0 + B - 1);
                acc = acc + sq_norm(w.x, w.y);
            }
        }
        for (int m = G >> 1; m > 0; m >>= 1) acc = acc + __shfl_xor(acc, m, 64);
        if (valid && l == 0) p[(long)row * a.nblocks + blk] = acc * a.invB;
    }
}

__global__ void __launch_bounds__(64)
    k_sqbank_fsm(int C, long nblocks, long lds, long ldl, double alpha, int timeout, const float* __restrict__ thr,
                 SqState* __restrict__ st, const double* __restrict__ p, uint8_t* __restrict__ status,
                 float* __restrict__ level)
{
    LDSP_LATENCY_CRITICAL();
    const int c = blockIdx.x * 64 + threadIdx.x;
    if (c >= C) return;
    const double* __restrict__ pr = p + (long)c * nblocks;
    uint8_t* __restrict__ sr = status + (long)c * lds;
    float* __restrict__ lr = level + (long)c * ldl;
    const float t = thr[c];
    double s = st[c].s;
    int mode = st[c].mode, timer = st[c].timer;

    auto step = [&](double pv, long b) {
        s = s + alpha * (pv - s);
        const float lv = (float)s;
        const bool hi = lv > t;
        // agc_squelch_update_mode as selects: with hi ENABLED rises and the others go to
        // SIGNALHI; without it ENABLED stays, RISE and SIGNALHI fall, FALL and SIGNALLO go low
        const int up = mode == SQ_ENABLED ? SQ_RISE : SQ_SIGNALHI;
        const int down = mode == SQ_ENABLED ? SQ_ENABLED : (mode >= SQ_FALL ? SQ_SIGNALLO : SQ_FALL);
        int next = hi ? up : down;
        timer = mode == SQ_FALL ? timeout : (mode == SQ_SIGNALLO ? timer - 1 : timer);
        next = mode == SQ_SIGNALLO && timer == 0 ? SQ_TIMEOUT : next;
        mode = mode == SQ_TIMEOUT ? SQ_ENABLED : next;
        lr[b] = lv;
        sr[b] = (uint8_t)mode;
    };
    // whole groups of kSqAhead blocks with the next group's p in flight (read at the row's last
    // block where the call ends before it), then the rest
    const long last = nblocks - 1;
    double cur[kSqAhead], nxt[kSqAhead];
#pragma unroll
    for (int u = 0; u < kSqAhead; u++) cur[u] = pr[min((long)u, last)];
    long b0 = 0;
    for (; b0 + kSqAhead <= nblocks; b0 += kSqAhead) {
#pragma unroll
        for (int u = 0; u < kSqAhead; u++) nxt[u] = pr[min(b0 + kSqAhead + u, last)];
#pragma unroll
        for (int u = 0; u < kSqAhead; u++) step(cur[u], b0 + u);
#pragma unroll
        for (int u = 0; u < kSqAhead; u++) cur[u] = nxt[u];
    }
#pragma unroll
    for (int u = 0; u < kSqAhead; u++)
        if (b0 + u < nblocks) step(cur[u], b0 + u);
    st[c].s = s;
    st[c].mode = mode;
    st[c].timer = timer;
}

__global__ void __launch_bounds__(kSqThreads)
    k_sqbank_gate(const SqArgs a, const float2* __restrict__ x, const float2* __restrict__ hist,
                  const uint8_t* __restrict__ status, long lds, float2* __restrict__ y, long ldy)
{
    const int tid = threadIdx.x;
    const int B = a.B, G = a.G, fill = a.fill;
    const int row = blockIdx.y;
    const float2* __restrict__ xr = x + (long)row * a.ldx;
    const float2* __restrict__ hr = hist + (long)row * B;
    const uint8_t* __restrict__ sr = status + (long)row * lds;
    float2* __restrict__ yr = y + (long)row * ldy;
    const int l = tid & (G - 1), gi = tid / G, NG = kSqThreads / G;
    const int half = B >> 1;
    const long t0 = (long)blockIdx.x * a.T;
    const SqVec4 zero = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int it = 0; it < a.T; it += NG) {
        const long blk = t0 + it + gi;
        if (blk >= a.nblocks) continue;
        const bool open = (unsigned)(sr[blk] - SQ_RISE) <= (unsigned)(SQ_SIGNALLO - SQ_RISE);
        const long g0 = blk * B - fill;
        float2* __restrict__ yb = yr + blk * B;
#pragma unroll 4
        for (int j = l; j < half; j += G)
            *reinterpret_cast<SqPair*>(yb + 2 * j) = open ? sq_pair(xr, hr, fill, g0 + 2 * j) : zero;
        if ((B & 1) && l == 0) yb[B - 1] = open ? sq_one(xr, hr, fill, g0 + B - 1) : make_float2(0.0f, 0.0f);
    }
}

} // namespace

int sqbank_tile(int B)
{
    const int NG = kSqThreads / sq_lanes(B);
    return ((kSqTileSamples + B - 1) / B + NG - 1) / NG * NG;
}

void sqbank(const SqbankCall& c, hipStream_t s)
{
    if (c.n == 0) return;
    LDSP_REQUIRE(c.C >= 1 && c.C <= kSqbankMaxC, "sqbank: row count out of range");
    LDSP_REQUIRE(c.B >= kSqbankMinB && c.B <= kSqbankMaxB, "sqbank: block length out of range");
    LDSP_REQUIRE(c.timeout >= 1 && c.alpha > 0.0 && c.alpha <= 1.0, "sqbank: bad parameters");
    LDSP_REQUIRE(c.n < ((size_t)1 << 36), "sqbank: call too long");
    LDSP_REQUIRE(c.ldx >= c.n && c.fill < (size_t)c.B, "sqbank: bad call geometry");
    LDSP_REQUIRE(c.nblocks == (c.fill + c.n) / c.B, "sqbank: block count does not match the call");
    LDSP_REQUIRE(c.lds >= c.nblocks && c.ldl >= c.nblocks && (!c.y || c.ldy >= c.nblocks * c.B),
                 "sqbank: output row stride below the call's blocks");
    SqArgs a;
    a.n = (long)c.n;
    a.ldx = (long)c.ldx;
    a.nblocks = (long)c.nblocks;
    a.fill = (int)c.fill;
    a.carry = (int)((c.fill + c.n) % c.B);
    a.B = c.B;
    a.G = sq_lanes(c.B);
    a.T = sqbank_tile(c.B);
    a.invB = 1.0 / (double)c.B;
    const unsigned grid = (unsigned)std::max<long>((a.nblocks + a.T - 1) / a.T, 1);
    {
        LDSP_PROF(s, "k_sqbank_power");
        hipLaunchKernelGGL(k_sqbank_power, dim3(grid, (unsigned)c.C), dim3(kSqThreads), 0, s, a, (const float2*)c.x,
                           (const float2*)c.hist, (float2*)c.hist_out, c.p);
        LDSP_HIP(hipGetLastError());
    }
    if (c.nblocks == 0) return;
    {
        LDSP_PROF(s, "k_sqbank_fsm");
        hipLaunchKernelGGL(k_sqbank_fsm, dim3((unsigned)(c.C + 63) / 64), dim3(64), 0, s, c.C, a.nblocks, (long)c.lds,
                           (long)c.ldl, c.alpha, c.timeout, c.thr, c.st, (const double*)c.p, c.status, c.level);
        LDSP_HIP(hipGetLastError());
    }
    if (c.y) {
        LDSP_PROF(s, "k_sqbank_gate");
        hipLaunchKernelGGL(k_sqbank_gate, dim3(grid, (unsigned)c.C), dim3(kSqThreads), 0, s, a, (const float2*)c.x,
                           (const float2*)c.hist, (const uint8_t*)c.status, (long)c.lds, (float2*)c.y, (long)c.ldy);
        LDSP_HIP(hipGetLastError());
    }
}

} // namespace k
} // namespace ldsp
