// k_ddc.hip -- tuned decimating filter bank (Downconverter): one wideband
// complex stream to C rows, each mixed down by its own 32-bit frequency word,
// low-passed by one real prototype and decimated by D.  liquid's counterpart is
// nco_crcf + firdecim_crcf; the definition is the project's own:
//   y[c][n] = scale sum_{j<L} h[j] x[nD - j] exp(-2 pi i ((nD - j) w_c mod 2^32) / 2^32)
// The phase is additive modulo 2^32, so with the host's complex taps
//   g_c[j]  = h[j] exp(+2 pi i ((j w_c) mod 2^32) / 2^32)
//   y[c][n] = scale rot_c(n) sum_j g_c[j] x[nD - j],   rot_c(n) = exp(-2 pi i ((nD w_c) mod 2^32) / 2^32).
//
// A workgroup of 512 threads (8 waves) owns F consecutive output columns of all
// C tuners (F = ddc_frames(D, L): 64, or 32 where the span of 64 would not fit
// the LDS):
//  1. The tile's input span -- (F - 1) D + L samples ending at the last
//     column's x[nD]; history before the call's first sample, zeros past its
//     last -- is staged in LDS residue-major: span sample i at
//     (i mod D) ROW + i / D, ROW odd.  Column f and span offset k = L - 1 - j
//     then meet at slot(k) + f, slot(k) = (k mod D) ROW + k / D (the host's
//     table ddc_slot, so the walk over k has no wrap to test): lanes on
//     consecutive columns read consecutive addresses at any D (lane per column
//     on a plain span would put the lanes D * 8 B apart), and the odd ROW
//     spreads the staging stores.
//  2. Sums, lane per column.  Wave w takes the part [w Lq, (w + 1) Lq) of the
//     offsets k, Lq = ceil(L / 8), and walks it in order with four accumulators
//     per tuner, offset i of the part into accumulator i mod 4: 32 partial
//     sums per output (one running float32 sum misses the 1e-6 gate for
//     long prototypes).  A wave carries TB = ddc_block(C) tuners at once, so one
//     ds_read_b64 feeds 4 TB multiply-adds; the tuners' taps are uniform across
//     the wave and come from the device table through scalar loads, laid out
//     [tuner block][k][TB] so that one load fetches a step's TB taps.
//  3. Each wave folds its four accumulators as (a0 + a1) + (a2 + a3) and leaves
//     the result in LDS; after a barrier thread (t, f) adds the eight waves' as
//     ((p0 + p1) + (p2 + p3)) + ((p4 + p5) + (p6 + p7)), multiplies by rot --
//     sincospi in double of the exact 32-bit phase, rounded once -- and by
//     scale, and stores with consecutive lanes on consecutive columns of one row.
// Every output runs these operations in this order wherever its column falls in
// a tile or a call, whatever C and TB are and whichever slot its tuner has, so
// a row's bits depend neither on the cut of the stream nor on the other tuners.
// Workgroup 0 also writes the next call's history (the last L - 1 raw samples
// of history ++ input) into the other buffer of the pair.
#include "kernels.hpp"
#include "ldsp_common.hpp"
#include "ldsp_math.hpp"

#include <type_traits>

namespace ldsp {
namespace k {

namespace {

constexpr int kDdcWaves = 8, kDdcThreads = 64 * kDdcWaves;
constexpr size_t kDdcLdsMax = 160 * 1024;
constexpr size_t kDdcRedBytes = kDdcWaves * 4 * 64 * sizeof(float2);   // the waves' sums of one round at TB = 4

// samples per residue row of the staged span: quotients 0 .. F - 1 + (L - 1) / D, odd
constexpr int ddc_row(int F, int D, int L) { return (F + (L - 1) / D) | 1; }
constexpr size_t ddc_lds(int F, int D, int L) { return (size_t)D * ddc_row(F, D, L) * sizeof(float2) + kDdcRedBytes; }

struct DdcArgs {
    long n, ncols, ld;
    unsigned long long col0;      // absolute index of the call's first column
    int skip, D, L, C, F, ROW;
    unsigned magic;               // ceil(2^32 / D): i / D = umulhi(i, magic) for i < 2^32 / D
    float scale;
};

__device__ __forceinline__ void ddc_mac(float2& a, const float2 g, const float2 v)
{
    a.x = fmaf(g.x, v.x, a.x);
    a.x = fmaf(-g.y, v.y, a.x);
    a.y = fmaf(g.x, v.y, a.y);
    a.y = fmaf(g.y, v.x, a.y);
}

// IQ16: x holds int16 (I, Q) pairs, one 4-byte word per sample, converted where
// they are loaded (iq_sample); the history stays complex64, so the calls of one
// stream may be of either kind.
template <int TB, bool IQ16>
__global__ void __launch_bounds__(kDdcThreads)
    k_ddc(const DdcArgs a, const std::conditional_t<IQ16, int, float2>* __restrict__ x, const float2* __restrict__ hist,
          float2* __restrict__ hist_out, const float2* __restrict__ taps, const int* __restrict__ slots,
          const uint32_t* __restrict__ words, float2* __restrict__ y)
{
    using X = std::conditional_t<IQ16, int, float2>;
    extern __shared__ __attribute__((aligned(16))) float2 S[];
    const int tid = threadIdx.x;
    const int D = a.D, L = a.L, F = a.F, ROW = a.ROW, H = L - 1;
    const long n = a.n;
    const long c0 = (long)blockIdx.x * F;             // first column of the tile
    const int cnt = (int)min((long)F, a.ncols - c0);
    float2* red = S + D * ROW;                        // [waves][TB][64]

    if (blockIdx.x == 0) {                            // the next call's history
        for (int j = tid; j < H; j += kDdcThreads) {
            const long g = n - H + j;
            if constexpr (IQ16) hist_out[j] = g < 0 ? hist[g + H] : iq_sample(x[g]);
            else hist_out[j] = g < 0 ? hist[g + H] : x[g];
        }
    }
    if (cnt <= 0) return;                             // a call shorter than skip: workgroup 0 alone, history only

    // span sample i = sample g0 + i of the call; column f of the tile ends at span sample f D + L - 1
    const long g0 = a.skip + c0 * D - H;
    const int span = (F - 1) * D + L;
    if (g0 >= 0 && g0 + span <= n) {                  // an inner tile reads the input alone
        const X* __restrict__ xb = x + g0;
#pragma unroll 4
        for (int i = tid; i < span; i += kDdcThreads) {
            const int q = (int)__umulhi((unsigned)i, a.magic);
            S[(i - q * D) * ROW + q] = iq_sample(xb[i]);
        }
    } else {
        for (int i = tid; i < span; i += kDdcThreads) {
            const long s = g0 + i;
            float2 v = make_float2(0.0f, 0.0f);
            if (s < 0) {
                if (s + H >= 0) v = hist[s + H];
            } else if (s < n) {
                v = iq_sample(x[s]);
            }
            const int q = (int)__umulhi((unsigned)i, a.magic);
            S[(i - q * D) * ROW + q] = v;
        }
    }
    __syncthreads();

    const int lane = tid & 63, f = lane & (F - 1);    // F = 32: the upper half-wave repeats the lower
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Lq = (L + kDdcWaves - 1) / kDdcWaves;
    const int k0 = min(w * Lq, L), k1 = min(k0 + Lq, L);
    const int ntb = (a.C + TB - 1) / TB;
    const float2* xf = S + f;

    for (int tb = 0; tb < ntb; tb++) {
        // the part's taps and the LDS slots of its offsets (column 0), both read ahead through scalar loads
        const float2* __restrict__ gp = taps + ((size_t)tb * L + k0) * TB;
        const int* __restrict__ sp = slots + k0;
        float2 acc[4][TB];
#pragma unroll
        for (int u = 0; u < 4; u++)
#pragma unroll
            for (int t = 0; t < TB; t++) acc[u][t] = make_float2(0.0f, 0.0f);

        // whole groups of four offsets as two pairs, each with its own registers:
        // the next pair's samples and taps are on their way while this pair's
        // multiply-adds run
        auto load = [&](float2(&v)[2], float2(&gt)[2][TB]) {
#pragma unroll
            for (int u = 0; u < 2; u++) {
                v[u] = xf[sp[u]];
#pragma unroll
                for (int t = 0; t < TB; t++) gt[u][t] = gp[u * TB + t];
            }
            gp += 2 * TB;
            sp += 2;
        };
        auto mac = [&](int u0, const float2(&v)[2], const float2(&gt)[2][TB]) {
#pragma unroll
            for (int u = 0; u < 2; u++)
#pragma unroll
                for (int t = 0; t < TB; t++) ddc_mac(acc[u0 + u][t], gt[u][t], v[u]);
        };
        const int ng = (k1 - k0) >> 2, rem = (k1 - k0) & 3;
        if (ng > 0) {
            float2 va[2], ga[2][TB], vb[2], gb[2][TB];
            load(va, ga);
            for (int i = 1; i < ng; i++) {
                load(vb, gb);
                mac(0, va, ga);
                load(va, ga);
                mac(2, vb, gb);
            }
            load(vb, gb);
            mac(0, va, ga);
            mac(2, vb, gb);
        }
#pragma unroll
        for (int u = 0; u < 3; u++) {                 // the part's last 0 .. 3 offsets, accumulators in the same turn
            if (u < rem) {
                const float2 v = xf[sp[u]];
#pragma unroll
                for (int t = 0; t < TB; t++) ddc_mac(acc[u][t], gp[u * TB + t], v);
            }
        }

        if (tb > 0) __syncthreads();                  // the round before has read its sums
#pragma unroll
        for (int t = 0; t < TB; t++) {
            const float2 lo = make_float2(acc[0][t].x + acc[1][t].x, acc[0][t].y + acc[1][t].y);
            const float2 hi = make_float2(acc[2][t].x + acc[3][t].x, acc[2][t].y + acc[3][t].y);
            red[(w * TB + t) * 64 + lane] = make_float2(lo.x + hi.x, lo.y + hi.y);
        }
        __syncthreads();

        const int t = tid >> 6, c = tb * TB + t;
        if (t < TB && lane < cnt && c < a.C) {
            float2 p[kDdcWaves];
#pragma unroll
            for (int v = 0; v < kDdcWaves; v++) p[v] = red[(v * TB + t) * 64 + lane];
#pragma unroll
            for (int st = 1; st < kDdcWaves; st *= 2)     // pairs, then pairs of pairs
#pragma unroll
                for (int v = 0; v < kDdcWaves; v += 2 * st) p[v] = make_float2(p[v].x + p[v + st].x, p[v].y + p[v + st].y);
            const float2 s = p[0];
            // rot: the low 32 bits of n D w are ((n D) mod 2^32) w mod 2^32; as a signed
            // count of 2^-31 half-turns it is exact in double
            const unsigned long long col = a.col0 + (unsigned long long)(c0 + lane);
            const uint32_t ph = (uint32_t)(col * (unsigned long long)D) * words[c];
            double sn, cs;
            sincospi((double)(int32_t)ph * (1.0 / 2147483648.0), &sn, &cs);
            const float rc = (float)cs, rs = -(float)sn;
            float2 o = make_float2(rc * s.x - rs * s.y, rc * s.y + rs * s.x);
            o.x *= a.scale;
            o.y *= a.scale;
            y[(long)c * a.ld + c0 + lane] = o;
        }
    }
}

template <int TB, bool IQ16>
void ddc_launch(const DdcArgs& a, const DdcCall& c, size_t lds, hipStream_t s)
{
    static bool attr = false;     // the largest dynamic LDS any launch may ask for, once per kernel
    if (!attr) {
        LDSP_HIP(hipFuncSetAttribute((const void*)k_ddc<TB, IQ16>, hipFuncAttributeMaxDynamicSharedMemorySize,
                                     (int)kDdcLdsMax));
        attr = true;
    }
    const unsigned grid = (unsigned)std::max<long>((a.ncols + a.F - 1) / a.F, 1);
    hipLaunchKernelGGL((k_ddc<TB, IQ16>), dim3(grid), dim3(kDdcThreads), lds, s, a,
                       (const std::conditional_t<IQ16, int, float2>*)c.x, (const float2*)c.hist, (float2*)c.hist_out,
                       (const float2*)c.taps, c.slots, c.words, (float2*)c.y);
}
template <int TB>
void ddc_launch(const DdcArgs& a, const DdcCall& c, size_t lds, hipStream_t s)
{
    if (c.iq16) ddc_launch<TB, true>(a, c, lds, s);
    else ddc_launch<TB, false>(a, c, lds, s);
}

} // namespace

int ddc_frames(int D, int L) { return ddc_lds(64, D, L) <= kDdcLdsMax ? 64 : 32; }

int ddc_slot(int D, int L, int k) { return (k % D) * ddc_row(ddc_frames(D, L), D, L) + k / D; }

void ddc(int D, const DdcCall& c, hipStream_t s)
{
    if (c.n == 0) return;
    LDSP_REQUIRE(D >= 2 && D <= kDdcMaxD, "ddc: decimation out of range");
    LDSP_REQUIRE(c.C >= 1 && c.C <= kDdcMaxC, "ddc: tuner count out of range");
    LDSP_REQUIRE(c.L >= 1 && c.L <= kChanMaxP * D, "ddc: prototype length out of range");
    LDSP_REQUIRE(c.n < ((size_t)1 << 41), "ddc: call too long");
    LDSP_REQUIRE(c.skip < (size_t)D && c.ld >= c.ncols, "ddc: bad call geometry");
    LDSP_REQUIRE(c.ncols == (c.n > c.skip ? (c.n - c.skip + D - 1) / D : 0), "ddc: column count does not match the call");
    DdcArgs a;
    a.n = (long)c.n;
    a.ncols = (long)c.ncols;
    a.ld = (long)c.ld;
    a.col0 = c.col0;
    a.skip = (int)c.skip;
    a.D = D;
    a.L = c.L;
    a.C = c.C;
    a.F = ddc_frames(D, c.L);
    a.ROW = ddc_row(a.F, D, c.L);
    a.magic = (unsigned)((((uint64_t)1 << 32) + D - 1) / D);
    a.scale = c.scale;
    const size_t lds = ddc_lds(a.F, D, c.L);
    LDSP_REQUIRE(lds <= kDdcLdsMax, "ddc: the tile's span does not fit the LDS");
    switch (ddc_block(c.C)) {
    case 1: {
        LDSP_PROF(s, "k_ddc_b1");
        ddc_launch<1>(a, c, lds, s);
        break;
    }
    case 2: {
        LDSP_PROF(s, "k_ddc_b2");
        ddc_launch<2>(a, c, lds, s);
        break;
    }
    default: {
        LDSP_PROF(s, "k_ddc_b4");
        ddc_launch<4>(a, c, lds, s);
        break;
    }
    }
    LDSP_HIP(hipGetLastError());
}

} // namespace k
} // namespace ldsp
