// k_fmbank.hip -- FM discriminator and audio decimator over the rows of a bank
// (FMBank): for every row c of a complex64 [C][n] block, FreqDem's discriminator
// followed by a real decimating FIR, in one pass.  The definition is the
// project's own (include/ldsp.h):
//   d[c][t] = lm_atan2f(im, re) * ref,  (re, im) = conj(x[c][t-1]) * x[c][t]
//   y[c][m] = scale * sum_{j<L} h[j] d[c][mD - j]          (d = 0 before t = 0)
// d is freqdem.hpp's freqdem_disc, the function k_freqdem calls.
//
// k_fmbank<QP> (QP = ceil(L / D), 1 .. kChanMaxP): a workgroup of F threads
// (F = fmbank_frames(D, L): 256, or 128 where the span of 256 takes more than
// 40 KiB of LDS) owns F consecutive output columns of one row (blockIdx.y).
//  1. Discriminator, thread per input sample.  The tile's span is the
//     (cnt - 1) D + L values d[s] ending at its last column's d[mD].  d[s] for
//     s at or after the call's first sample is evaluated from x[s - 1], x[s]
//     (x[-1]: the row's carried previous sample); before it, d[s] comes from
//     the row's history, which holds discriminator values, so "d = 0 before
//     t = 0" is a zeroed buffer.  The span goes to LDS residue-major as k_ddc's:
//     span value i at (i mod D) ROW + i / D, ROW odd.  The full-rate d never
//     reaches HBM.
//  2. Sums, lane per column.  Column f and span offset k = L - 1 - j meet at
//     (k mod D) ROW + k / D + f: consecutive lanes read consecutive words at
//     any D.  The walk is residue by residue (r = k mod D ascending) and, in a
//     residue, quotient by quotient (q = k / D ascending, QP of them for
//     r < L mod D or when D divides L, QP - 1 otherwise; both counts are
//     compile-time, so the reads of a residue are one base address plus
//     immediate offsets and there is no tail to test).  The taps are uniform
//     across the wave and come through scalar loads from the host's table
//     [D][QP], t[r][q] = h[L - 1 - (q D + r)].  Term (r, q) goes to accumulator
//     q mod 16 with one fmaf: up to 16 partial sums per output, each of at
//     most 2 D terms (one running float32 sum misses the 1e-6 gate for long
//     prototypes), folded pairwise in a fixed tree and
//     multiplied by scale.
// Every output runs these operations in this order wherever its column falls in
// a tile or a call and whatever C is, so a row's bits depend neither on the cut
// of the stream nor on the other rows.  Tile 0 of each row also writes the
// row's next history -- the last L - 1 discriminator values of history ++ call,
// from the same function on the same operands -- and its last raw sample into
// the other buffers of the pairs.
//
// k_fmbank_disc (decimation 1, no prototype): y = d, k_freqdem over rows; no
// filter arithmetic, so each row carries FreqDem's bits.
#include "kernels.hpp"
#include "ldsp_common.hpp"
#include "freqdem.hpp"
#include <array>
#include <utility>

namespace ldsp {
namespace k {

namespace {

constexpr int kFmbMaxThreads = 256;
constexpr size_t kFmbLdsWide = 40 * 1024;     // the widest tile's span may take this much LDS

// values per residue row of the staged span: quotients 0 .. F - 1 + (L - 1) / D, odd
constexpr int fmb_row(int F, int D, int L) { return (F + (L - 1) / D) | 1; }
constexpr size_t fmb_lds(int F, int D, int L) { return (size_t)D * fmb_row(F, D, L) * sizeof(float); }

struct FmbArgs {
    long n, ncols, ldx, ldy;
    int skip, D, L, F, ROW;
    int R1;                       // residues r < R1 hold QP taps, the others QP - 1
    unsigned magic;               // ceil(2^32 / D), D > 1: i / D = umulhi(i, magic) for i < 2^32 / D
    float ref, scale;
};

// d[s] of a row: x[s - 1] is read at max(s - 1, 0) and replaced by the carried sample at s = 0, a
// select instead of a branch around the load
__device__ __forceinline__ float fmb_disc_at(const float2* __restrict__ xr, long s, float2 pv, float ref)
{
    const float2 q = xr[s > 0 ? s - 1 : 0];
    return freqdem_disc(s > 0 ? q : pv, xr[s], ref);
}

typedef const float __attribute__((address_space(4)))* cfptr;   // the uniform tap table -> scalar loads

// one residue's Q terms of the column sum: s[q] meets t[q], term q into accumulator q mod 16
template <int Q>
__device__ __forceinline__ void fmb_residue(float (&acc)[16], const float* __restrict__ s, cfptr t)
{
#pragma unroll
    for (int q = 0; q < Q; q++) acc[q & 15] = fmaf(t[q], s[q], acc[q & 15]);
}

template <int QP>
__global__ void __launch_bounds__(kFmbMaxThreads)
    k_fmbank(const FmbArgs a, const float2* __restrict__ x, const float* __restrict__ dhist, float* __restrict__ dhist_out,
             const float2* __restrict__ prev, float2* __restrict__ prev_out, const float* __restrict__ taps,
             float* __restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) float S[];
    const int tid = threadIdx.x;
    const int D = a.D, L = a.L, F = a.F, ROW = a.ROW, H = L - 1;
    const long n = a.n;
    const int row = blockIdx.y;
    const float2* __restrict__ xr = x + (long)row * a.ldx;
    const float* __restrict__ dh = dhist + (long)row * H;
    const float2 pv = prev[row];
    const long c0 = (long)blockIdx.x * F;             // first column of the tile
    const int cnt = (int)min((long)F, a.ncols - c0);

    if (blockIdx.x == 0) {                            // the row's next history and previous sample
        float* __restrict__ dho = dhist_out + (long)row * H;
        for (int j = tid; j < H; j += F) {
            const long g = n - H + j;
            dho[j] = g < 0 ? dh[g + H] : fmb_disc_at(xr, g, pv, a.ref);
        }
        if (tid == 0) prev_out[row] = xr[n - 1];
    }
    if (cnt <= 0) return;                             // a call shorter than skip: tile 0 alone, state only

    // span value i = d[g0 + i] of the call; column f of the tile ends at span value f D + L - 1,
    // and the last one, (cnt - 1) D + L - 1, is the call's sample skip + (c0 + cnt - 1) D < n
    const long g0 = a.skip + c0 * D - H;
    const int span = (cnt - 1) * D + L;
    for (int i = tid; i < span; i += F) {
        const long s = g0 + i;
        float v;
        if (s < 0)
            v = dh[s + H];
        else
            v = fmb_disc_at(xr, s, pv, a.ref);
        const int q = D == 1 ? i : (int)__umulhi((unsigned)i, a.magic);
        S[(i - q * D) * ROW + q] = v;
    }
    __syncthreads();
    if (tid >= cnt) return;

    float acc[16];
#pragma unroll
    for (int u = 0; u < 16; u++) acc[u] = 0.0f;
    const float* sp = S + tid;
    cfptr tp = (cfptr)taps;
    const int R1 = a.R1;
#pragma unroll 2
    for (int r = 0; r < R1; r++) {
        fmb_residue<QP>(acc, sp, tp);
        sp += ROW;
        tp += QP;
    }
    if (QP > 1) {
#pragma unroll 2
        for (int r = R1; r < D; r++) {
            fmb_residue<QP - 1>(acc, sp, tp);
            sp += ROW;
            tp += QP;
        }
    }
#pragma unroll
    for (int st = 1; st < 16; st *= 2)                // pairs, then pairs of pairs
#pragma unroll
        for (int u = 0; u < 16; u += 2 * st) acc[u] = acc[u] + acc[u + st];
    y[(long)row * a.ldy + c0 + tid] = acc[0] * a.scale;
}

__global__ void __launch_bounds__(256)
    k_fmbank_disc(const float2* __restrict__ x, const float2* __restrict__ prev, float2* __restrict__ prev_out, long n,
                  long ldx, long ldy, float ref, float* __restrict__ y)
{
    const int row = blockIdx.y;
    const float2* __restrict__ xr = x + (long)row * ldx;
    float* __restrict__ yr = y + (long)row * ldy;
    const long stride = (long)gridDim.x * 256;
    const long i0 = (long)blockIdx.x * 256 + threadIdx.x;
    const float2 pv = prev[row];
    for (long i = i0; i < n; i += stride) yr[i] = fmb_disc_at(xr, i, pv, ref);
    if (i0 == 0) prev_out[row] = xr[n - 1];
}

template <int QP>
void fmbank_launch(const FmbArgs& a, const FmbankCall& c, size_t lds, hipStream_t s)
{
    const unsigned grid = (unsigned)std::max<long>((a.ncols + a.F - 1) / a.F, 1);
    hipLaunchKernelGGL((k_fmbank<QP>), dim3(grid, (unsigned)c.C), dim3((unsigned)a.F), lds, s, a, (const float2*)c.x,
                       c.dhist, c.dhist_out, (const float2*)c.prev, (float2*)c.prev_out, c.taps, c.y);
}

using FmbLaunch = void (*)(const FmbArgs&, const FmbankCall&, size_t, hipStream_t);
template <int... Q>
constexpr std::array<FmbLaunch, sizeof...(Q)> fmb_table(std::integer_sequence<int, Q...>)
{
    return {{&fmbank_launch<Q + 1>...}};
}

} // namespace

int fmbank_frames(int D, int L) { return fmb_lds(256, D, L) <= kFmbLdsWide ? 256 : 128; }

void fmbank(int D, const FmbankCall& c, hipStream_t s)
{
    if (c.n == 0) return;
    LDSP_REQUIRE(c.C >= 1 && c.C <= kFmbankMaxC, "fmbank: row count out of range");
    LDSP_REQUIRE(D >= 1 && D <= kFmbankMaxD, "fmbank: decimation out of range");
    LDSP_REQUIRE(c.n < ((size_t)1 << 36), "fmbank: call too long");
    LDSP_REQUIRE(c.ldx >= c.n, "fmbank: input row stride below the call's length");
    if (c.L == 0) {                                   // the discriminator alone
        LDSP_REQUIRE(D == 1 && c.ncols == c.n && c.ldy >= c.n, "fmbank: bad call geometry");
        LDSP_PROF(s, "k_fmbank_disc");
        // about 32 Ki workgroups over all rows: with one sample per thread 256 rows of 256 Ki samples
        // took 0.39 ms against 0.26 ms for 16 rows of 4 Mi
        const unsigned grid = (unsigned)std::min<size_t>((c.n + 255) / 256, std::max(32768 / c.C, 1));
        hipLaunchKernelGGL(k_fmbank_disc, dim3(grid, (unsigned)c.C), dim3(256), 0, s, (const float2*)c.x,
                           (const float2*)c.prev, (float2*)c.prev_out, (long)c.n, (long)c.ldx, (long)c.ldy, c.ref, c.y);
        LDSP_HIP(hipGetLastError());
        return;
    }
    LDSP_REQUIRE(c.L >= 1 && c.L <= kChanMaxP * D, "fmbank: prototype length out of range");
    LDSP_REQUIRE(c.skip < (size_t)D && c.ldy >= c.ncols, "fmbank: bad call geometry");
    LDSP_REQUIRE(c.ncols == (c.n > c.skip ? (c.n - c.skip + D - 1) / D : 0), "fmbank: column count does not match the call");
    FmbArgs a;
    a.n = (long)c.n;
    a.ncols = (long)c.ncols;
    a.ldx = (long)c.ldx;
    a.ldy = (long)c.ldy;
    a.skip = (int)c.skip;
    a.D = D;
    a.L = c.L;
    a.F = fmbank_frames(D, c.L);
    a.ROW = fmb_row(a.F, D, c.L);
    a.R1 = c.L % D == 0 ? D : c.L % D;
    a.magic = (unsigned)((((uint64_t)1 << 32) + D - 1) / D);
    a.ref = c.ref;
    a.scale = c.scale;
    const size_t lds = fmb_lds(a.F, D, c.L);
    static_assert(fmb_lds(128, kFmbankMaxD, kChanMaxP * kFmbankMaxD) <= 64 * 1024, "the narrow tile fits the default LDS limit");
    static constexpr auto table = fmb_table(std::make_integer_sequence<int, kChanMaxP>{});
    LDSP_PROF(s, "k_fmbank");
    table[(c.L + D - 1) / D - 1](a, c, lds, s);
    LDSP_HIP(hipGetLastError());
}

} // namespace k
} // namespace ldsp
