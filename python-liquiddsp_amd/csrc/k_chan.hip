// k_chan.hip -- polyphase analysis filter bank (Channelizer): one wideband
// complex stream to M channel rows.  No reference counterpart (liquid's firpfbch
// family is the same structure); the definition is the project's own:
//   y[k][n] = scale sum_{j<L} h[j] x[nD - j] exp(-2 pi i k (nD - j) / M),  k < M,
// computed in polyphase form with P = ceil(L / M) taps per branch,
//   u_p[n]  = sum_{q<P} h[p + qM] x[nD - p - qM]                         p < M
//   y[k][n] = scale rot(k, n) sum_p u_p[n] exp(+2 pi i k p / M)
// rot = 1 for D = M and (-1)^(k n) for D = M / 2 (n the absolute output index).
//
// A workgroup of 256 threads owns F consecutive output frames (columns):
//  1. The tile's input span -- (F - 1) D + P M samples ending at the last frame's
//     x[nD]; history before the call's first sample, zeros past its last -- is
//     staged in LDS with unit-stride loads.
//  2. Branch sums, lane per branch: thread (g, p) keeps branch p's P taps in
//     registers and sums frames g, g + G, ... (G = 256 / M).  Neighbouring lanes
//     read neighbouring samples, and neighbouring lane groups read frames D <= M
//     samples apart, so the 32 lanes of a ds_read_b64 group cover at most 32
//     consecutive samples: no bank conflict at any D.  (Lane per frame would put
//     the lanes D * 8 B apart: every lane on the same banks from D = 16 up.)
//     The sums stay in registers until every lane has read its samples; then
//     they overwrite the span as U[f][p], rows M + 1 samples long.
//  3. The M-point inverse DFT per frame, lane per frame from here on: the odd
//     row length makes the lanes' 8-byte accesses conflict-free.  M <= 16 is one
//     register transform (fft_butterflies.hpp).  M = R1 R2 above that: R2-point
//     transforms over p2 (p = p2 R1 + p1) in place, the twiddle
//     exp(2 pi i k2 p1 / M) from the host's table, one barrier, then R1-point
//     transforms over p1 give k = k1 R2 + k2.
//  4. scale and the sign, then stores with consecutive lanes on consecutive
//     columns of one row (F >= 32: at least 256 B per row and tile).
// Every frame runs the same operations in the same order wherever it falls in a
// tile or a call, so an output's bits do not depend on the cut of the stream.
// Workgroup 0 also writes the next call's history (the last P M - 1 samples of
// history ++ input) into the other buffer of the pair.
#include "chan_dft.hpp"
#include "kernels.hpp"
#include "ldsp_common.hpp"
#include "ldsp_math.hpp"

#include <type_traits>

namespace ldsp {
namespace k {

namespace {

constexpr int chan_slots(int M, int D)
{
    const int F = chan_frames(M);
    const int xs = (F - 1) * D + kChanMaxP * M, us = F * (M + 1);
    return xs > us ? xs : us;
}

// n: input samples of the call (> 0); skip: samples before the call's first
// frame; ncols: its frames; par: parity of the first frame's absolute index.
// IQ16: x holds int16 (I, Q) pairs, one 4-byte word per sample, converted where
// they are loaded (iq_sample); the history stays complex64, so the calls of one
// stream may be of either kind.
template <int M, int D, bool IQ16>
__global__ void __launch_bounds__(256) k_chan(const std::conditional_t<IQ16, int, float2>* __restrict__ x,
                                              const float2* __restrict__ hist, float2* __restrict__ hist_out, long n,
                                              int skip, long ncols, int par, const float* __restrict__ taps, int P,
                                              const float2* __restrict__ tw, float scale, float2* __restrict__ y,
                                              long ld)
{
    using X = std::conditional_t<IQ16, int, float2>;
    constexpr int F = chan_frames(M);
    constexpr int G = 256 / M;                        // frames summed side by side
    constexpr int NF = F / G;                         // frames per thread in the sums
    constexpr int R2 = chan_r2(M), R1 = M / R2;
    constexpr int ROW = M + 1;
    static_assert(F % G == 0 && (F * R1) % 256 == 0 && (F * R2) % 256 == 0, "whole items per thread");
    __shared__ __attribute__((aligned(16))) float2 S[chan_slots(M, D)];
    const int tid = threadIdx.x;
    const int PM = P * M, H = PM - 1;
    const long c0 = (long)blockIdx.x * F;             // first frame of the tile
    const int cnt = (int)min((long)F, ncols - c0);

    if (blockIdx.x == 0) {                            // the next call's history
        for (int j = tid; j < H; j += 256) {
            const long g = n - H + j;
            if constexpr (IQ16) hist_out[j] = g < 0 ? hist[g + H] : iq_sample(x[g]);
            else hist_out[j] = g < 0 ? hist[g + H] : x[g];
        }
    }
    if (cnt <= 0) return;                             // a call shorter than skip: workgroup 0 alone, history only

    const int p = tid % M, g = tid / M;
    float hq[kChanMaxP];                              // taps holds kChanMaxP * M floats, zero past L
#pragma unroll
    for (int q = 0; q < kChanMaxP; q++) hq[q] = taps[q * M + p];

    // S[i] = sample g0 + i of the call; frame f of the tile ends at S[f D + PM - 1]
    const long g0 = skip + c0 * D - PM + 1;
    const int span = (F - 1) * D + PM;
    if (g0 >= 0 && g0 + span <= n) {
        // an inner tile reads the input alone: all its loads are issued before the first LDS store
        constexpr int kLd = ((F - 1) * D + kChanMaxP * M + 255) / 256;
        const X* __restrict__ xb = x + g0;
        float2 v[kLd];
#pragma unroll
        for (int i = 0; i < kLd; i++) {
            const int u = tid + 256 * i;
            if constexpr (IQ16) {
                // no guard round the conversion (it would wait for each load in turn):
                // lanes past the span load its last word again and store nothing
                v[i] = iq_sample(xb[min(u, span - 1)]);
            } else {
                v[i] = make_float2(0.0f, 0.0f);
                if (u < span) v[i] = xb[u];
            }
        }
#pragma unroll
        for (int i = 0; i < kLd; i++) {
            const int u = tid + 256 * i;
            if (u < span) S[u] = v[i];
        }
    } else {
        for (int i = tid; i < span; i += 256) {
            const long s = g0 + i;
            float2 v = make_float2(0.0f, 0.0f);
            if (s < 0) {
                if (s + H >= 0) v = hist[s + H];
            } else if (s < n) {
                v = iq_sample(x[s]);
            }
            S[i] = v;
        }
    }
    __syncthreads();

    float2 acc[NF];
#pragma unroll
    for (int i = 0; i < NF; i++) acc[i] = make_float2(0.0f, 0.0f);
    const float2* xb = S + (PM - 1 - p) + g * D;
#pragma unroll
    for (int q = 0; q < kChanMaxP; q++) {
        if (q < P) {
            const float h = hq[q];
            const float2* xp = xb - q * M;
#pragma unroll
            for (int i = 0; i < NF; i++) {
                const float2 v = xp[i * G * D];
                acc[i].x = fmaf(h, v.x, acc[i].x);
                acc[i].y = fmaf(h, v.y, acc[i].y);
            }
        }
    }
    __syncthreads();                                  // the span is read; U takes its place
#pragma unroll
    for (int i = 0; i < NF; i++) S[(g + G * i) * ROW + p] = acc[i];
    __syncthreads();

    if constexpr (R2 > 1) {
        constexpr int IA = F * R1 / 256;
#pragma unroll
        for (int i = 0; i < IA; i++) {
            const int it = tid + 256 * i;
            const int f = it % F, p1 = it / F;
            float2* row = S + f * ROW + p1;
            float2 v[R2];
#pragma unroll
            for (int p2 = 0; p2 < R2; p2++) v[p2] = row[p2 * R1];
            chan_idft<R2>(v);
#pragma unroll
            for (int k2 = 1; k2 < R2; k2++) v[k2] = cmul(v[k2], tw[k2 * p1]);
#pragma unroll
            for (int k2 = 0; k2 < R2; k2++) row[k2 * R1] = v[k2];
        }
        __syncthreads();
    }

    constexpr int IB = F * R2 / 256;
#pragma unroll
    for (int i = 0; i < IB; i++) {
        const int it = tid + 256 * i;
        const int f = it % F, k2 = it / F;
        const float2* row = S + f * ROW + k2 * R1;
        float2 v[R1];
#pragma unroll
        for (int p1 = 0; p1 < R1; p1++) v[p1] = row[p1];
        chan_idft<R1>(v);
        if (f < cnt) {
            const long col = c0 + f;
            const bool nodd = D != M && ((par + (int)(col & 1)) & 1);
#pragma unroll
            for (int k1 = 0; k1 < R1; k1++) {
                const int k = k1 * R2 + k2;
                float2 o = make_float2(v[k1].x * scale, v[k1].y * scale);
                if (nodd && (k & 1)) o = make_float2(-o.x, -o.y);
                y[(long)k * ld + col] = o;
            }
        }
    }
}

template <int M, int D, bool IQ16>
void chan_launch(const ChanCall& c, hipStream_t s)
{
    constexpr int F = chan_frames(M);
    const unsigned grid = (unsigned)std::max<size_t>((c.ncols + F - 1) / F, 1);
    hipLaunchKernelGGL((k_chan<M, D, IQ16>), dim3(grid), dim3(256), 0, s,
                       (const std::conditional_t<IQ16, int, float2>*)c.x, (const float2*)c.hist, (float2*)c.hist_out,
                       (long)c.n, (int)c.skip, (long)c.ncols, c.parity, c.taps, c.P, (const float2*)c.tw, c.scale,
                       (float2*)c.y, (long)c.ld);
}
template <int M, int D>
void chan_launch(const ChanCall& c, hipStream_t s)
{
    if (c.iq16) chan_launch<M, D, true>(c, s);
    else chan_launch<M, D, false>(c, s);
}

} // namespace

#define LDSP_CHAN_CASE(m)                                      \
    case m:                                                    \
        if (D == m) {                                          \
            LDSP_PROF(s, "k_chan_m" #m "_crit");               \
            chan_launch<m, m>(c, s);                           \
        } else {                                               \
            LDSP_PROF(s, "k_chan_m" #m "_os2");                \
            chan_launch<m, m / 2>(c, s);                       \
        }                                                      \
        break

void chan(int M, int D, const ChanCall& c, hipStream_t s)
{
    if (c.n == 0) return;
    LDSP_REQUIRE(D == M || 2 * D == M, "chan: decimation must be M or M / 2");
    LDSP_REQUIRE(c.P >= 1 && c.P <= kChanMaxP, "chan: taps per branch out of range");
    LDSP_REQUIRE(c.n < ((size_t)1 << 41), "chan: call too long");
    LDSP_REQUIRE(c.skip < (size_t)D && c.ld >= c.ncols, "chan: bad call geometry");
    LDSP_REQUIRE(c.ncols == (c.n > c.skip ? (c.n - c.skip + D - 1) / D : 0), "chan: column count does not match the call");
    switch (M) {
        LDSP_CHAN_CASE(4);
        LDSP_CHAN_CASE(8);
        LDSP_CHAN_CASE(16);
        LDSP_CHAN_CASE(32);
        LDSP_CHAN_CASE(64);
        LDSP_CHAN_CASE(128);
        LDSP_CHAN_CASE(256);
    default:
        throw Error(LDSP_EINVAL, "chan: channel count must be a power of two in 4 .. 256");
    }
    LDSP_HIP(hipGetLastError());
}
#undef LDSP_CHAN_CASE

} // namespace k
} // namespace ldsp
