// k_ssbbank.hip -- tuned single-sideband demodulator over the rows of a bank
// (SSBBank): for every row c of a complex64 [C][n] block (a Channelizer,
// Downconverter or SquelchBank output), the row's complex band-pass decimating
// FIR over the chosen sideband and one exact rotation per output, in one launch
// for all rows.  The definition is the project's own (include/ldsp.h):
//   S[c][n]  = sum_{j<L} g_c[j] x[c][nD-j]              (g_c: the host's complex taps of row c)
//   rot_c(n) = exp(-2 pi i ((((nD) mod 2^32) w_c) mod 2^32) / 2^32)
//   y[c][n]  = Re(rot_c(n) S[c][n])
// The phase is additive modulo 2^32, so the BFO's rotation of the input is split
// exactly into the taps' (host) and one rotation per output (here), as k_ddc's.
//
// A workgroup of 256 threads (4 waves) owns F = 128 consecutive output columns of
// one row (blockIdx.y); the staging, the walk and the fold are k_ambank's, with
// two columns per lane:
//  1. The tile's input span -- (F - 1) D + L samples ending at the last
//     column's x[nD]; the row's history before the call's first sample, zeros
//     past its last -- is staged in LDS as (re, im) pairs, residue-major: span
//     sample i at pair (i mod D) ROW + i / D, ROW odd.  Column f and span offset
//     k = L - 1 - j meet at slot(k) + f, slot(k) = (k mod D) ROW + k / D: lanes on
//     consecutive columns read consecutive pairs at any D (no bank conflict on
//     the 8-byte reads; ROW odd keeps the staging stores apart, see k_ambank).
//  2. Sums.  Lane l of every wave owns the columns l and l + 64 of the tile.
//     Wave w takes the part [w Lq, (w + 1) Lq) of the offsets k, Lq = ceil(L / 4),
//     and walks it in order with eight accumulator sets per column, offset i of
//     the part into set i mod 8.  A set holds the four sums
//     P = sum Re g (x_re, x_im) and Q = sum Im g (x_re, x_im).  The taps of an
//     offset and its slot are uniform across the wave and come from the row's
//     part of one device table, [C][L][4] words indexed by k, through scalar
//     loads (4 MiB at the largest, read through L2 by every tile of the row);
//     one read of the two pairs 64 apart (ds_read2st64_b64) and the two scalar
//     taps feed eight fused multiply-adds, so the scalar loads and the address
//     arithmetic per multiply-add are half of k_ambank's.  The two columns of a
//     lane share nothing but the taps: each has its own sets, and the order of
//     its operations is that of a one-column walk.
//  3. Each wave folds the eight sets of a column pairwise in a fixed tree and
//     leaves the four results in LDS; after a barrier thread f < 128 adds the
//     four waves' as (p0 + p1) + (p2 + p3) and forms
//       S_re = P.x - Q.y,  S_im = P.y + Q.x                      (one operation each)
//       rc = (float)cos, rs = (float)sin of the exact 32-bit phase (double sincospi, rounded once)
//       y = fma(rc, S_re, rs * S_im) + 0                          (Re((rc - i rs) S); + 0 turns a -0 of a zero row into +0)
// Every output runs these operations in this order wherever its column falls in
// a tile or a call and whatever C and the strides are, so a row's bits depend
// neither on the cut of the stream nor on the other rows.  Tile 0 of each row
// also writes the row's next history (the last L - 1 raw samples of history ++
// call) into the other buffer of the pair.
#include "kernels.hpp"
#include "ldsp_common.hpp"

namespace ldsp {
namespace k {

namespace {

constexpr int kSsbWaves = 4, kSsbThreads = 64 * kSsbWaves;
constexpr int kSsbCols = 2;                           // output columns per lane
constexpr int kSsbF = 64 * kSsbCols;                  // output columns per workgroup
constexpr int kSsbAcc = 8;                            // accumulator sets per wave and column
constexpr int kSsbSums = 4;                           // P.x, P.y, Q.x, Q.y

// pairs per residue row of the staged span: quotients 0 .. F - 1 + (L - 1) / D, odd
constexpr int ssb_row(int D, int L) { return (kSsbF + (L - 1) / D) | 1; }
constexpr size_t ssb_lds(int D, int L)
{
    return (size_t)D * ssb_row(D, L) * sizeof(float2) + (size_t)kSsbWaves * kSsbCols * kSsbSums * 64 * sizeof(float);
}

struct SsbArgs {
    long n, ncols, ldx, ldy;
    unsigned long long col0;      // absolute index of the call's first column
    int skip, D, L, ROW;
    unsigned magic;               // ceil(2^32 / D), D > 1: i / D = umulhi(i, magic) for i < 2^32 / D
};

typedef const float __attribute__((address_space(4)))* cfptr;   // the uniform tap table -> scalar loads

// offset k of the part: its samples (column 0's at pair t[2]) into the four sums of accumulator set u of each column
__device__ __forceinline__ void ssb_mac(float (&acc)[kSsbAcc][kSsbCols][kSsbSums], int u, const float2* __restrict__ xf, cfptr t)
{
    const float2* xs = xf + __builtin_bit_cast(int, t[2]);
#pragma unroll
    for (int c = 0; c < kSsbCols; c++) {
        const float2 v = xs[64 * c];
        acc[u][c][0] = fmaf(t[0], v.x, acc[u][c][0]);
        acc[u][c][1] = fmaf(t[0], v.y, acc[u][c][1]);
        acc[u][c][2] = fmaf(t[1], v.x, acc[u][c][2]);
        acc[u][c][3] = fmaf(t[1], v.y, acc[u][c][3]);
    }
}

__global__ void __launch_bounds__(kSsbThreads)
    k_ssbbank(const SsbArgs a, const float2* __restrict__ x, const float2* __restrict__ hist, float2* __restrict__ hist_out,
              const float* __restrict__ taps, const uint32_t* __restrict__ words, float* __restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) float2 S2[];
    const int tid = threadIdx.x;
    const int D = a.D, L = a.L, ROW = a.ROW, H = L - 1;
    const long n = a.n;
    const int row = blockIdx.y;
    const float2* __restrict__ xr = x + (long)row * a.ldx;
    const float2* __restrict__ hr = hist + (long)row * H;
    const long c0 = (long)blockIdx.x * kSsbF;         // first column of the tile
    const int cnt = (int)min((long)kSsbF, a.ncols - c0);
    float* red = (float*)(S2 + D * ROW);              // [waves][columns][sums][64]

    if (blockIdx.x == 0) {                            // the row's next history
        float2* __restrict__ ho = hist_out + (long)row * H;
        for (int j = tid; j < H; j += kSsbThreads) {
            const long g = n - H + j;
            ho[j] = g < 0 ? hr[g + H] : xr[g];
        }
    }
    if (cnt <= 0) return;                             // a call shorter than skip: tile 0 alone, history only

    // span sample i = sample g0 + i of the call (g0 >= -H); column f of the tile ends at span sample f D + L - 1
    const long g0 = a.skip + c0 * D - H;
    const int span = (kSsbF - 1) * D + L;
    for (int i = tid; i < span; i += kSsbThreads) {
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
    const int Lq = (L + kSsbWaves - 1) / kSsbWaves;
    const int k0 = min(w * Lq, L), k1 = min(k0 + Lq, L);
    const float2* xf = S2 + lane;
    // the row's part of the table, at most 256 * 1025 * 4 words in; kept in a scalar register (the compiler
    // otherwise carries (long)L through the divergent staging loop in a vector register and the table with it)
    cfptr tp = (cfptr)taps + (unsigned)__builtin_amdgcn_readfirstlane((row * L + k0) * 4);

    float acc[kSsbAcc][kSsbCols][kSsbSums];
#pragma unroll
    for (int u = 0; u < kSsbAcc; u++)
#pragma unroll
        for (int c = 0; c < kSsbCols; c++)
#pragma unroll
            for (int q = 0; q < kSsbSums; q++) acc[u][c][q] = 0.0f;
    const int ng = (k1 - k0) / kSsbAcc, rem = (k1 - k0) % kSsbAcc;
    for (int i = 0; i < ng; i++) {
#pragma unroll
        for (int u = 0; u < kSsbAcc; u++) ssb_mac(acc, u, xf, tp + u * 4);
        tp += kSsbAcc * 4;
    }
#pragma unroll
    for (int u = 0; u < kSsbAcc - 1; u++)             // the part's last 0 .. 7 offsets, sets in the same turn
        if (u < rem) ssb_mac(acc, u, xf, tp + u * 4);

#pragma unroll
    for (int st = 1; st < kSsbAcc; st *= 2)           // pairs, then pairs of pairs
#pragma unroll
        for (int u = 0; u < kSsbAcc; u += 2 * st)
#pragma unroll
            for (int c = 0; c < kSsbCols; c++)
#pragma unroll
                for (int q = 0; q < kSsbSums; q++) acc[u][c][q] = acc[u][c][q] + acc[u + st][c][q];
#pragma unroll
    for (int c = 0; c < kSsbCols; c++)
#pragma unroll
        for (int q = 0; q < kSsbSums; q++) red[((w * kSsbCols + c) * kSsbSums + q) * 64 + lane] = acc[0][c][q];
    __syncthreads();
    if (tid >= cnt) return;

    float p[kSsbSums];
#pragma unroll
    for (int q = 0; q < kSsbSums; q++) {
        const float* r = red + ((tid >> 6) * kSsbSums + q) * 64 + (tid & 63);
        constexpr int W = kSsbCols * kSsbSums * 64;             // one wave's results
        p[q] = (r[0] + r[W]) + (r[2 * W] + r[3 * W]);
    }
    static_assert(kSsbWaves == 4, "the tree above adds four waves");
    const float sre = p[0] - p[3], sim = p[1] + p[2];
    // rot: the low 32 bits of n D w are ((n D) mod 2^32) w mod 2^32; as a signed
    // count of 2^-31 half-turns it is exact in double
    const long col = c0 + tid;
    const uint32_t ph = (uint32_t)((a.col0 + (unsigned long long)col) * (unsigned long long)D) * words[row];
    double sn, cs;
    sincospi((double)(int32_t)ph * (1.0 / 2147483648.0), &sn, &cs);
    const float rc = (float)cs, rs = (float)sn;
    y[(long)row * a.ldy + col] = fmaf(rc, sre, rs * sim) + 0.0f;
}

} // namespace

int ssbbank_frames(int D, int L)
{
    (void)D;
    (void)L;
    return kSsbF;
}

int ssbbank_slot(int D, int L, int k) { return (k % D) * ssb_row(D, L) + k / D; }

void ssbbank(const SsbbankCall& c, hipStream_t s)
{
    if (c.n == 0) return;
    const int D = c.D;
    LDSP_REQUIRE(c.C >= 1 && c.C <= kSsbbankMaxC, "ssbbank: row count out of range");
    LDSP_REQUIRE(D >= 1 && D <= kSsbbankMaxD, "ssbbank: decimation out of range");
    LDSP_REQUIRE(c.L >= 1 && c.L <= kSsbbankMaxL, "ssbbank: prototype length out of range");
    LDSP_REQUIRE(c.n < ((size_t)1 << 36), "ssbbank: call too long");
    LDSP_REQUIRE(c.ldx >= c.n, "ssbbank: input row stride below the call's length");
    LDSP_REQUIRE(c.skip < (size_t)D && c.ldy >= c.ncols, "ssbbank: bad call geometry");
    LDSP_REQUIRE(c.ncols == (c.n > c.skip ? (c.n - c.skip + D - 1) / D : 0), "ssbbank: column count does not match the call");
    SsbArgs a;
    a.n = (long)c.n;
    a.ncols = (long)c.ncols;
    a.ldx = (long)c.ldx;
    a.ldy = (long)c.ldy;
    a.col0 = c.col0;
    a.skip = (int)c.skip;
    a.D = D;
    a.L = c.L;
    a.ROW = ssb_row(D, c.L);
    a.magic = (unsigned)((((uint64_t)1 << 32) + D - 1) / D);
    static_assert(ssb_lds(kSsbbankMaxD, kSsbbankMaxL) <= 64 * 1024 && ssb_lds(1, kSsbbankMaxL) <= 64 * 1024,
                  "the tile fits the default LDS limit");
    const unsigned grid = (unsigned)std::max<size_t>((c.ncols + kSsbF - 1) / kSsbF, 1);
    LDSP_PROF(s, "k_ssbbank");
    hipLaunchKernelGGL(k_ssbbank, dim3(grid, (unsigned)c.C), dim3(kSsbThreads), ssb_lds(D, c.L), s, a, (const float2*)c.x,
                       (const float2*)c.hist, (float2*)c.hist_out, c.taps, c.words, c.y);
    LDSP_HIP(hipGetLastError());
}

} // namespace k
} // namespace ldsp
