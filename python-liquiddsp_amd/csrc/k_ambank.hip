// k_ambank.hip -- coherent AM demodulator over the rows of a bank (AMBank): for
// every row c of a complex64 [C][n] block (a Channelizer, Downconverter or
// SquelchBank output), the carrier and the audio band with the carrier taken out
// by two decimating FIRs over one read of the row, and the feed-forward
// combine, in one launch for all rows.  The definition is the project's own
// (include/ldsp.h):
//   d[j]     = (float)((double)h[j] - (double)g[j])
//   B[c][n]  = sum_{j<L} d[j] x[c][nD-j]
//   Cr[c][n] = sum_{j<L} g[j] x[c][nD-j]
//   m = |Cr|^2,  y[c][n] = m > thr^2 ? Re(B conj(Cr)) / m : 0
// Nothing here depends on the stream position but skip, so the result is exact
// for any stream length.
//
// A workgroup of 256 threads (4 waves) owns F = 64 consecutive output columns of
// one row (blockIdx.y):
//  1. The tile's input span -- (F - 1) D + L samples ending at the last
//     column's x[nD]; the row's history before the call's first sample, zeros
//     past its last -- is staged in LDS as (re, im) pairs, residue-major as
//     k_stbank's: span sample i at pair (i mod D) ROW + i / D, ROW odd.  Column f
//     and span offset k = L - 1 - j meet at slot(k) + f, slot(k) = (k mod D) ROW +
//     k / D: lanes on consecutive columns read consecutive pairs at any D, and
//     an 8-byte LDS read is banked modulo 64 words per 32 lanes, so the 32 pairs
//     of a half-wave fall on 64 different banks whatever ROW is.  ROW is odd for
//     the staging stores, which are banked modulo 32 words per 16 lanes: 16
//     consecutive span samples are 16 residues (D >= 16), 2 ROW words apart.
//  2. Sums, lane per column.  Wave w takes the part [w Lq, (w + 1) Lq) of the
//     offsets k, Lq = ceil(L / 4), and walks it in order with eight accumulators
//     per sum, offset i of the part into accumulator i mod 8: 32 partial sums
//     per output and sum.  One 8-byte LDS read feeds four fused multiply-adds
//     (Re / Im B, Re / Im Cr; two v_pk_fma_f32 over the (re, im) pair as
//     built, see the Makefile).  The two taps of an offset and its slot are
//     uniform across the wave and come from one device table, [L][4] words
//     indexed by k, through scalar loads.
//  3. Each wave folds its eight accumulators pairwise in a fixed tree and
//     leaves the four results in LDS; after a barrier thread f < 64 adds the
//     four waves' as (p0 + p1) + (p2 + p3), forms m and the product with one
//     fused multiply-add each, divides with an IEEE division and stores y.
// Every output runs these operations in this order wherever its column falls in
// a tile or a call and whatever C and the strides are, so a row's bits depend
// neither on the cut of the stream nor on the other rows.  Tile 0 of each row
// also writes the row's next history (the last L - 1 raw samples of history ++
// call) into the other buffer of the pair, and the thread that owns the call's
// last column writes the row's carrier level sqrtf(m).
#include "kernels.hpp"
#include "ldsp_common.hpp"

namespace ldsp {
namespace k {

namespace {

constexpr int kAmbWaves = 4, kAmbThreads = 64 * kAmbWaves;
constexpr int kAmbF = 64;                             // output columns per workgroup
constexpr int kAmbAcc = 8;                            // accumulators per wave and sum
constexpr int kAmbSums = 4;                           // Re B, Im B, Re Cr, Im Cr

// pairs per residue row of the staged span: quotients 0 .. F - 1 + (L - 1) / D, odd
constexpr int amb_row(int D, int L) { return (kAmbF + (L - 1) / D) | 1; }
constexpr size_t amb_lds(int D, int L)
{
    return (size_t)D * amb_row(D, L) * sizeof(float2) + (size_t)kAmbWaves * kAmbSums * 64 * sizeof(float);
}

struct AmbArgs {
    long n, ncols, ldx, ldy;
    int skip, D, L, ROW;
    unsigned magic;               // ceil(2^32 / D), D > 1: i / D = umulhi(i, magic) for i < 2^32 / D
    float thr2;
};

typedef const float __attribute__((address_space(4)))* cfptr;   // the uniform tap table -> scalar loads

// offset k of the part: its sample (column 0's at pair t[2]) into the four sums of accumulator set u
__device__ __forceinline__ void amb_mac(float (&acc)[kAmbAcc][kAmbSums], int u, const float2* __restrict__ xf, cfptr t)
{
    const float2 v = xf[__builtin_bit_cast(int, t[2])];
    acc[u][0] = fmaf(t[0], v.x, acc[u][0]);
    acc[u][1] = fmaf(t[0], v.y, acc[u][1]);
    acc[u][2] = fmaf(t[1], v.x, acc[u][2]);
    acc[u][3] = fmaf(t[1], v.y, acc[u][3]);
}

__global__ void __launch_bounds__(kAmbThreads)
    k_ambank(const AmbArgs a, const float2* __restrict__ x, const float2* __restrict__ hist, float2* __restrict__ hist_out,
             const float* __restrict__ taps, float* __restrict__ y, float* __restrict__ level)
{
    extern __shared__ __attribute__((aligned(16))) float2 S2[];
    const int tid = threadIdx.x;
    const int D = a.D, L = a.L, ROW = a.ROW, H = L - 1;
    const long n = a.n;
    const int row = blockIdx.y;
    const float2* __restrict__ xr = x + (long)row * a.ldx;
    const float2* __restrict__ hr = hist + (long)row * H;
    const long c0 = (long)blockIdx.x * kAmbF;         // first column of the tile
    const int cnt = (int)min((long)kAmbF, a.ncols - c0);
    float* red = (float*)(S2 + D * ROW);              // [waves][sums][64]

    if (blockIdx.x == 0) {                            // the row's next history
        float2* __restrict__ ho = hist_out + (long)row * H;
        for (int j = tid; j < H; j += kAmbThreads) {
            const long g = n - H + j;
            ho[j] = g < 0 ? hr[g + H] : xr[g];
        }
    }
    if (cnt <= 0) return;                             // a call shorter than skip: tile 0 alone, history only

    // span sample i = sample g0 + i of the call (g0 >= -H); column f of the tile ends at span sample f D + L - 1
    const long g0 = a.skip + c0 * D - H;
    const int span = (kAmbF - 1) * D + L;
    for (int i = tid; i < span; i += kAmbThreads) {
        const long s = g0 + i;
        float2 v = make_float2(0.0f, 0.0f);
        if (s < 0)
            v = hr[s + H];
        else if (s < n)
            v = xr[s];
        const int q = D == 1 ? i : (int)__umulhi((unsigned)i, a.magic);
        S2[(i - q * D) * ROW + q] = v;
    }
    __syncthreads();

    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Lq = (L + kAmbWaves - 1) / kAmbWaves;
    const int k0 = min(w * Lq, L), k1 = min(k0 + Lq, L);
    const float2* xf = S2 + lane;
    cfptr tp = (cfptr)taps + (size_t)k0 * 4;

    float acc[kAmbAcc][kAmbSums];
#pragma unroll
    for (int u = 0; u < kAmbAcc; u++)
#pragma unroll
        for (int q = 0; q < kAmbSums; q++) acc[u][q] = 0.0f;
    const int ng = (k1 - k0) / kAmbAcc, rem = (k1 - k0) % kAmbAcc;
    for (int i = 0; i < ng; i++) {
#pragma unroll
        for (int u = 0; u < kAmbAcc; u++) amb_mac(acc, u, xf, tp + u * 4);
        tp += kAmbAcc * 4;
    }
#pragma unroll
    for (int u = 0; u < kAmbAcc - 1; u++)             // the part's last 0 .. 7 offsets, accumulators in the same turn
        if (u < rem) amb_mac(acc, u, xf, tp + u * 4);

#pragma unroll
    for (int st = 1; st < kAmbAcc; st *= 2)           // pairs, then pairs of pairs
#pragma unroll
        for (int u = 0; u < kAmbAcc; u += 2 * st)
#pragma unroll
            for (int q = 0; q < kAmbSums; q++) acc[u][q] = acc[u][q] + acc[u + st][q];
#pragma unroll
    for (int q = 0; q < kAmbSums; q++) red[(w * kAmbSums + q) * 64 + lane] = acc[0][q];
    __syncthreads();
    if (tid >= cnt) return;

    float p[kAmbSums];
#pragma unroll
    for (int q = 0; q < kAmbSums; q++) {
        const float* r = red + q * 64 + tid;
        p[q] = (r[0] + r[kAmbSums * 64]) + (r[2 * kAmbSums * 64] + r[3 * kAmbSums * 64]);
    }
    static_assert(kAmbWaves == 4, "the tree above adds four waves");
    const float br = p[0], bi = p[1], cr = p[2], ci = p[3];
    const float m = fmaf(cr, cr, ci * ci);
    const float re = fmaf(br, cr, bi * ci);           // Re(B conj(Cr))
    const long col = c0 + tid;
    y[(long)row * a.ldy + col] = m > a.thr2 ? __fdiv_rn(re, m) : 0.0f;
    if (col == a.ncols - 1) level[row] = __fsqrt_rn(m);
}

} // namespace

int ambank_frames(int D, int L)
{
    (void)D;
    (void)L;
    return kAmbF;
}

int ambank_slot(int D, int L, int k) { return (k % D) * amb_row(D, L) + k / D; }

void ambank(const AmbankCall& c, hipStream_t s)
{
    if (c.n == 0) return;
    const int D = c.D;
    LDSP_REQUIRE(c.C >= 1 && c.C <= kAmbankMaxC, "ambank: row count out of range");
    LDSP_REQUIRE(D >= 1 && D <= kAmbankMaxD, "ambank: decimation out of range");
    LDSP_REQUIRE(c.L >= 1 && c.L <= kAmbankMaxL, "ambank: prototype length out of range");
    LDSP_REQUIRE(c.n < ((size_t)1 << 36), "ambank: call too long");
    LDSP_REQUIRE(c.ldx >= c.n, "ambank: input row stride below the call's length");
    LDSP_REQUIRE(c.skip < (size_t)D && c.ldy >= c.ncols, "ambank: bad call geometry");
    LDSP_REQUIRE(c.ncols == (c.n > c.skip ? (c.n - c.skip + D - 1) / D : 0), "ambank: column count does not match the call");
    AmbArgs a;
    a.n = (long)c.n;
    a.ncols = (long)c.ncols;
    a.ldx = (long)c.ldx;
    a.ldy = (long)c.ldy;
    a.skip = (int)c.skip;
    a.D = D;
    a.L = c.L;
    a.ROW = amb_row(D, c.L);
    a.magic = (unsigned)((((uint64_t)1 << 32) + D - 1) / D);
    a.thr2 = c.thr2;
    static_assert(amb_lds(kAmbankMaxD, kAmbankMaxL) <= 64 * 1024 && amb_lds(1, kAmbankMaxL) <= 64 * 1024,
                  "the tile fits the default LDS limit");
    const unsigned grid = (unsigned)std::max<size_t>((c.ncols + kAmbF - 1) / kAmbF, 1);
    LDSP_PROF(s, "k_ambank");
    hipLaunchKernelGGL(k_ambank, dim3(grid, (unsigned)c.C), dim3(kAmbThreads), amb_lds(D, c.L), s, a, (const float2*)c.x,
                       (const float2*)c.hist, (float2*)c.hist_out, c.taps, c.y, c.level);
    LDSP_HIP(hipGetLastError());
}

} // namespace k
} // namespace ldsp
