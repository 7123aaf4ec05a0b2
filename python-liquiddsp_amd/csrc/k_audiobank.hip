// k_audiobank.hip -- de-emphasis and arbitrary-rate resampling over the rows of
// a bank (AudioBank): for every row c of a float32 [C][n] block, an optional
// one-pole de-emphasis at the input rate followed by liquid's polyphase
// resampler (resamp_rrrf), in one pass.  The definition (include/ldsp.h):
//   e[c][t] = b0 sum_{j>=0} a^j u[c][t-j]          (de-emphasis off: e = u)
//   y[c][k] = sum_{i<2m} h_{b_k}[i] e[c][j_k - i]  (the schedule (j_k, b_k) of ldsp_resamp)
//   out     = y scale, or its 16-bit PCM rounding
//
// k_audiobank<DE, PCM, SKEW>: the grid is (tiles, rows); a workgroup of 256 threads
// owns T <= 256 consecutive outputs of one row (blockIdx.y), so the row count
// never enters an output's arithmetic.
//  1. Span.  resamp_j gives the tile's input span [jlo, jhi] (call-relative;
//     negative indices are the row's history, which holds raw input).  Without
//     de-emphasis it goes straight to LDS.  With it the span is widened down to
//     a block boundary and by the warm-up J in front, and staged raw.
//  2. De-emphasis in LDS, thread per block, as a block scan on an absolute
//     grid.  The row's absolute sample index (counted since creation or reset)
//     is cut into blocks of kAbBlock.  First every block of the raw span runs
//     the recursion v = u + a v from zero and keeps its end value; then a
//     block's start state is the sum over the P = J / kAbBlock blocks before it,
//     c = sum_p (a^kAbBlock)^(p-1) end[m - p] (Horner, oldest first), and the
//     block runs the recursion again from c: e^[t] = (float)(b0 v[t]).  All of
//     it in float64, each output rounded once.  a^J <= 2^-30, so e^ is e to
//     1e-9 of the input's scale, and e^[t] is a function of u and of t's
//     absolute position alone: it does not depend on where a tile or a call
//     begins.  A float32 state misses the 1e-6 gate on a constant row
//     (DESIGN.md section 4).  kAbBlock is odd, so the threads' reads of the raw
//     span (kAbBlock words apart) fall on distinct banks.
//  3. Sums, lane per output: resamp's sequential float32 dot product
//     r = r + h[i] e[i] over the branch's reversed taps (the bits of
//     k_resamp_tile when e = u).  Neighbouring lanes' windows start about
//     1 / rate samples apart -- 32 words at rate 1/32, two banks for a wave.
//     Where that distance is within 1/8 word of a multiple of 4 words (SKEW,
//     decided on the host from step) the span is kept skewed, word p at
//     p + p / 32; elsewhere the lanes spread over the banks by themselves and
//     the span stays linear, its reads one base address plus immediate offsets
//     (the skew costs four address instructions per tap).
//     The tap rows are padded to an odd length (2m + 1).
// Tile 0 of each row also writes the row's next history (the last H raw samples
// of history ++ call) into the other buffer of the pair.  No workgroup waits on
// another.
#include "kernels.hpp"
#include "ldsp_common.hpp"
#include "resamp_dev.hpp"

namespace ldsp {
namespace k {

namespace {

constexpr int kAbThreads = 256;
constexpr int kAbBlock = 33;                          // de-emphasis block (odd)
constexpr int kAbBias = 32 * kAbBlock;                // a multiple of the block above any history length
static_assert(kAbBias >= 2 * kAudiobankMaxM + kAbBlock + kAudiobankMaxJ, "the bias covers the longest history");

__host__ __device__ constexpr int ab_skew(int p) { return p + (p >> 5); }
template <bool SKEW>
__device__ __forceinline__ int ab_at(int p)
{
    return SKEW ? ab_skew(p) : p;
}
// neighbouring windows start step / 2^24 words apart: skew where that is within 1/8 word of a
// multiple of 4 words
constexpr bool ab_skewed(uint32_t step)
{
    const uint32_t r = step & ((1u << 26) - 1);
    return step >= (1u << 26) - (1u << 21) && (r <= (1u << 21) || r >= (1u << 26) - (1u << 21));
}

struct AbArgs {
    long n, K, ldx, ldy;
    uint64_t P0;
    uint32_t step;
    int bits_index, sub_len, T, H;
    int J, ph;                    // warm-up; the call's first sample's absolute index mod kAbBlock
    int ntap, eoff, uoff, noff;   // words of the padded tap table; LDS word offsets of the spans and the block ends
    double a, aB, b0;             // aB = a^kAbBlock
    float scale;
};

// span words a tile of T outputs may need: the windows, widened down to a block boundary with de-emphasis
constexpr int ab_span(int T, uint32_t step, int sub_len, bool de)
{
    return (int)(((uint64_t)(T - 1) * step) >> 24) + sub_len + 2 + (de ? kAbBlock - 1 : 0);
}

template <bool DE, bool PCM, bool SKEW>
__global__ void __launch_bounds__(kAbThreads)
    k_audiobank(const AbArgs a, const float* __restrict__ x, const float* __restrict__ hist, float* __restrict__ hist_out,
                const float* __restrict__ sub, void* __restrict__ y_)
{
    extern __shared__ __attribute__((aligned(16))) float S[];
    const int tid = threadIdx.x;
    const int row = blockIdx.y;
    const int H = a.H, halo = a.sub_len - 1, TROW = a.sub_len + 1;
    const long n = a.n;
    const float* __restrict__ xr = x + (long)row * a.ldx;
    const float* __restrict__ hr = hist + (long)row * H;

    if (blockIdx.x == 0) {                            // the row's next history
        float* __restrict__ ho = hist_out + (long)row * H;
        for (int j = tid; j < H; j += kAbThreads) {
            const long g = n - H + j;
            ho[j] = g >= 0 ? xr[g] : hr[g + H];
        }
    }
    const long k0 = (long)blockIdx.x * a.T;
    const long k1 = min(a.K, k0 + a.T);
    if (k0 >= k1) return;                             // a call without outputs: tile 0 alone, state only

    float* taps = S;                                  // [npfb][TROW]
    float* E = S + a.eoff;                            // the (de-emphasised) span, skewed
    for (int i = tid; i < a.ntap; i += kAbThreads) taps[i] = sub[i];

    const long jlo = resamp_j(a.P0, (uint64_t)k0, a.step) - halo;
    const long jhi = resamp_j(a.P0, (uint64_t)(k1 - 1), a.step);           // < n
    long elo = jlo;
    if (DE) elo -= (jlo + a.ph + kAbBias) % kAbBlock; // down to the block boundary at or below jlo
    const int cntE = (int)(jhi - elo + 1);
    if (DE) {
        float* U = S + a.uoff;                        // the raw span, J samples of warm-up in front
        const int J = a.J;
        const long ulo = elo - J;                     // >= -H
        const int cntU = cntE + J;
        for (int e = tid; e < cntU; e += kAbThreads) {
            const long g = ulo + e;
            U[e] = g >= 0 ? xr[g] : hr[g + H];
        }
        __syncthreads();
        // raw block q holds span words q kAbBlock ..; span block m (the values e^ of E) is raw block m + P
        double* EN = reinterpret_cast<double*>(S + a.noff);
        const int P = J / kAbBlock;
        const int nblk = (cntE + kAbBlock - 1) / kAbBlock;
        const double ad = a.a, aB = a.aB, b0 = a.b0;
        for (int q = tid; q < P + nblk - 1; q += kAbThreads) {   // all whole: (nblk - 1) kAbBlock < cntE
            const float* up = U + q * kAbBlock;
            double v = 0.0;
#pragma unroll
            for (int i = 0; i < kAbBlock; i++) v = fma(ad, v, (double)up[i]);
            EN[q] = v;
        }
        __syncthreads();
        for (int m = tid; m < nblk; m += kAbThreads) {
            double v = EN[m];
            for (int p = 1; p < P; p++) v = fma(aB, v, EN[m + p]);
            const float* up = U + (m + P) * kAbBlock;
            const int cnt = min(kAbBlock, cntE - m * kAbBlock);
            for (int i = 0; i < cnt; i++) {
                v = fma(ad, v, (double)up[i]);
                E[ab_at<SKEW>(m * kAbBlock + i)] = (float)(b0 * v);
            }
        }
    } else {
        for (int e = tid; e < cntE; e += kAbThreads) {
            const long g = elo + e;
            E[ab_at<SKEW>(e)] = g >= 0 ? xr[g] : hr[g + H];
        }
    }
    __syncthreads();
    const long k = k0 + tid;
    if (k >= k1) return;

    const long j = resamp_j(a.P0, (uint64_t)k, a.step);
    const uint64_t ph = a.P0 + (uint64_t)k * a.step - ((uint64_t)j << 24);
    const int b = (int)(ph >> a.bits_index);
    const float* hb = taps + b * TROW;
    int p = (int)(j - halo - elo);                    // 0 <= p, p + halo <= cntE - 1
    float r = 0.0f;
    for (int i = 0; i < a.sub_len; i++, p++) r = r + hb[i] * E[ab_at<SKEW>(p)];
    const float z = r * a.scale;
    if (PCM) {
        const float q = fminf(fmaxf(rintf(z * 32767.0f), -32768.0f), 32767.0f);
        ((short*)y_)[(long)row * a.ldy + k] = (short)(int)q;
    } else {
        ((float*)y_)[(long)row * a.ldy + k] = z;
    }
}

struct AbPlan {
    int T, ntap, eoff, uoff, noff;
    size_t lds;
};

AbPlan ab_plan(uint32_t step, int sub_len, int npfb, int J)
{
    const bool de = J > 0;
    AbPlan p;
    p.ntap = npfb * (sub_len + 1);
    p.eoff = (p.ntap + 3) & ~3;
    auto fill = [&](int T) {
        const int se = ab_span(T, step, sub_len, de);
        p.T = T;
        p.uoff = p.eoff + ((ab_skew(se) + 1 + 3) & ~3);
        p.noff = p.uoff + (de ? (se + J + 1) & ~1 : 0);            // 8-byte aligned
        p.lds = (size_t)(p.noff + (de ? 2 * (J / kAbBlock + (se + kAbBlock - 1) / kAbBlock) : 0)) * sizeof(float);
    };
    int T = kAbThreads;
    for (fill(T); T > 1 && p.lds > 64 * 1024; fill(T)) T >>= 1;
    return p;
}

} // namespace

int audiobank_tile(uint32_t step, int sub_len, int npfb, int J) { return ab_plan(step, sub_len, npfb, J).T; }

void audiobank(const AudiobankCall& c, hipStream_t s)
{
    if (c.n == 0) return;
    LDSP_REQUIRE(c.C >= 1 && c.C <= kAudiobankMaxC, "audiobank: row count out of range");
    LDSP_REQUIRE(c.sub_len >= 2 && c.sub_len <= 2 * kAudiobankMaxM && c.npfb >= 1 &&
                     c.npfb * c.sub_len <= kAudiobankMaxTaps,
                 "audiobank: branch table out of range");
    LDSP_REQUIRE(c.step >= ((uint32_t)1 << 22) && c.step <= ((uint32_t)1 << 29), "audiobank: rate out of range");
    LDSP_REQUIRE(c.J >= 0 && c.J <= kAudiobankMaxJ && c.J % kAbBlock == 0, "audiobank: warm-up out of range");
    LDSP_REQUIRE(c.H == c.sub_len - 1 + (c.J > 0 ? c.J + kAbBlock - 1 : 0), "audiobank: history length does not match");
    LDSP_REQUIRE(c.n < ((size_t)1 << 36), "audiobank: call too long");
    LDSP_REQUIRE(c.ldx >= c.n && c.ldy >= c.K, "audiobank: bad call geometry");
    const AbPlan p = ab_plan(c.step, c.sub_len, c.npfb, c.J);
    LDSP_REQUIRE(p.lds <= 64 * 1024, "audiobank: the tile does not fit the LDS");
    AbArgs a;
    a.n = (long)c.n;
    a.K = (long)c.K;
    a.ldx = (long)c.ldx;
    a.ldy = (long)c.ldy;
    a.P0 = c.P0;
    a.step = c.step;
    a.bits_index = c.bits_index;
    a.sub_len = c.sub_len;
    a.T = p.T;
    a.H = c.H;
    a.J = c.J;
    a.ph = (int)(c.seen % kAbBlock);
    a.ntap = p.ntap;
    a.eoff = p.eoff;
    a.uoff = p.uoff;
    a.noff = p.noff;
    a.a = c.a;
    a.aB = 1.0;
    for (int i = 0; i < kAbBlock; i++) a.aB *= c.a;
    a.b0 = c.b0;
    a.scale = c.scale;
    const dim3 grid((unsigned)std::max<size_t>((c.K + p.T - 1) / p.T, 1), (unsigned)c.C);
    LDSP_PROF(s, "k_audiobank");
    using Kernel = void (*)(AbArgs, const float*, const float*, float*, const float*, void*);
    static constexpr Kernel table[8] = {
        k_audiobank<false, false, false>, k_audiobank<false, false, true>, k_audiobank<false, true, false>,
        k_audiobank<false, true, true>,   k_audiobank<true, false, false>, k_audiobank<true, false, true>,
        k_audiobank<true, true, false>,   k_audiobank<true, true, true>};
    const Kernel kern = table[(c.J > 0 ? 4 : 0) + (c.pcm16 ? 2 : 0) + (ab_skewed(c.step) ? 1 : 0)];
    hipLaunchKernelGGL(kern, grid, dim3(kAbThreads), p.lds, s, a, c.x, c.hist, c.hist_out, c.sub, c.y);
    LDSP_HIP(hipGetLastError());
}

int audiobank_hist(int sub_len, int J) { return sub_len - 1 + (J > 0 ? J + kAbBlock - 1 : 0); }

int audiobank_warmup(int J) { return (J + kAbBlock - 1) / kAbBlock * kAbBlock; }

} // namespace k
} // namespace ldsp
