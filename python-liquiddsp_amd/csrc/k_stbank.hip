// k_stbank.hip -- FM stereo decoder over the rows of a bank (StereoBank): for
// every row c of a float32 [C][n] block of multiplex samples (an FMBank(C, kf, 1)
// output), the mono sum, the 38 kHz difference and the 19 kHz pilot by three
// decimating FIRs over one read of the row, and the feed-forward combine, in
// one launch for all rows.  The definition is the project's own (include/ldsp.h):
//   s[c][n] = sum_{j<L} h[j] u[c][nD-j]
//   z[c][n] = sum_{j<L} h[j] u[c][nD-j] exp(-2 pi i (((nD-j) 2w) mod 2^32) / 2^32)
//   P[c][n] = sum_{j<L} g[j] u[c][nD-j] exp(-2 pi i (((nD-j)  w) mod 2^32) / 2^32)
//   m = |P|^2,  S = m > thr^2 ? 2 Im(z conj(P)^2) / m : 0,  left = s + S,  right = s - S
// The phase is additive modulo 2^32, so with the host's complex taps
//   gz[j] = h[j] exp(+2 pi i ((j 2w) mod 2^32) / 2^32),  gp[j] = g[j] exp(+2 pi i ((j w) mod 2^32) / 2^32)
//   z = rz(n) z',  z' = sum_j gz[j] u[nD-j],   P = rp(n) P',  P' = sum_j gp[j] u[nD-j]
// with rz(n) = exp(-2 pi i ((nD 2w) mod 2^32) / 2^32) and rp(n) likewise with w.
// (nD 2w) mod 2^32 = 2 ((nD w) mod 2^32) mod 2^32, so rz = rp^2 exactly:
// z conj(P)^2 = z' conj(P')^2 and |P| = |P'|.  Neither m nor S depends on the
// rotations; the kernel evaluates both on z' and P' and applies none.  Nothing
// here depends on the stream position but skip, so the result is exact for any
// stream length.
//
// A workgroup of 256 threads (4 waves) owns F = 64 consecutive output columns of
// one row (blockIdx.y):
//  1. The tile's input span -- (F - 1) D + L samples ending at the last
//     column's u[nD]; the row's history before the call's first sample, zeros
//     past its last -- is staged in LDS residue-major as k_ddc's: span sample i
//     at (i mod D) ROW + i / D, ROW odd.  Column f and span offset k = L - 1 - j
//     meet at slot(k) + f, slot(k) = (k mod D) ROW + k / D: lanes on consecutive
//     columns read consecutive words at any D.
//  2. Sums, lane per column.  Wave w takes the part [w Lq, (w + 1) Lq) of the
//     offsets k, Lq = ceil(L / 4), and walks it in order with eight accumulators
//     per sum, offset i of the part into accumulator i mod 8: 32 partial sums
//     per output and sum.  One LDS read feeds five multiply-adds (s, Re / Im z',
//     Re / Im P').  The five taps of an offset and its slot are uniform across
//     the wave and come from one device table, [L][8] words indexed by k,
//     through scalar loads.
//  3. Each wave folds its eight accumulators pairwise in a fixed tree and
//     leaves the five results in LDS; after a barrier thread f < 64 adds the
//     four waves' as (p0 + p1) + (p2 + p3), forms m, S with an IEEE division,
//     and stores left and right.
// Every output runs these operations in this order wherever its column falls in
// a tile or a call and whatever C and the strides are, so a row's bits depend
// neither on the cut of the stream nor on the other rows.  Tile 0 of each row
// also writes the row's next history (the last L - 1 raw samples of history ++
// call) into the other buffer of the pair, and the thread that owns the call's
// last column writes the row's pilot level sqrtf(m).
#include "kernels.hpp"
#include "ldsp_common.hpp"

namespace ldsp {
namespace k {

namespace {

constexpr int kStbWaves = 4, kStbThreads = 64 * kStbWaves;
constexpr int kStbF = 64;                             // output columns per workgroup
constexpr int kStbAcc = 8;                            // accumulators per wave and sum
constexpr int kStbSums = 5;                           // s, Re z', Im z', Re P', Im P'

// samples per residue row of the staged span: quotients 0 .. F - 1 + (L - 1) / D, odd
constexpr int stb_row(int D, int L) { return (kStbF + (L - 1) / D) | 1; }
constexpr size_t stb_lds(int D, int L)
{
    return ((size_t)D * stb_row(D, L) + (size_t)kStbWaves * kStbSums * 64) * sizeof(float);
}

struct StbArgs {
    long n, ncols, ldx, ldy;
    int skip, D, L, ROW;
    unsigned magic;               // ceil(2^32 / D), D > 1: i / D = umulhi(i, magic) for i < 2^32 / D
    float thr2;
};

typedef const float __attribute__((address_space(4)))* cfptr;   // the uniform tap table -> scalar loads

// offset k of the part: its sample (column 0's at slot t[5]) into the five sums of accumulator set u
__device__ __forceinline__ void stb_mac(float (&acc)[kStbAcc][kStbSums], int u, const float* __restrict__ xf, cfptr t)
{
    const float v = xf[__builtin_bit_cast(int, t[5])];
#pragma unroll
    for (int q = 0; q < kStbSums; q++) acc[u][q] = fmaf(t[q], v, acc[u][q]);
}

__global__ void __launch_bounds__(kStbThreads)
    k_stbank(const StbArgs a, const float* __restrict__ x, const float* __restrict__ hist, float* __restrict__ hist_out,
             const float* __restrict__ taps, float* __restrict__ y, float* __restrict__ level)
{
    extern __shared__ __attribute__((aligned(16))) float S[];
    const int tid = threadIdx.x;
    const int D = a.D, L = a.L, ROW = a.ROW, H = L - 1;
    const long n = a.n;
    const int row = blockIdx.y;
    const float* __restrict__ xr = x + (long)row * a.ldx;
    const float* __restrict__ hr = hist + (long)row * H;
    const long c0 = (long)blockIdx.x * kStbF;         // first column of the tile
    const int cnt = (int)min((long)kStbF, a.ncols - c0);
    float* red = S + D * ROW;                         // [waves][sums][64]

    if (blockIdx.x == 0) {                            // the row's next history
        float* __restrict__ ho = hist_out + (long)row * H;
        for (int j = tid; j < H; j += kStbThreads) {
            const long g = n - H + j;
            ho[j] = g < 0 ? hr[g + H] : xr[g];
        }
    }
    if (cnt <= 0) return;                             // a call shorter than skip: tile 0 alone, history only

    // span sample i = sample g0 + i of the call (g0 >= -H); column f of the tile ends at span sample f D + L - 1
    const long g0 = a.skip + c0 * D - H;
    const int span = (kStbF - 1) * D + L;
    for (int i = tid; i < span; i += kStbThreads) {
        const long s = g0 + i;
        float v = 0.0f;
        if (s < 0)
            v = hr[s + H];
        else if (s < n)
            v = xr[s];
        const int q = D == 1 ? i : (int)__umulhi((unsigned)i, a.magic);
        S[(i - q * D) * ROW + q] = v;
    }
    __syncthreads();

    const int lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Lq = (L + kStbWaves - 1) / kStbWaves;
    const int k0 = min(w * Lq, L), k1 = min(k0 + Lq, L);
    const float* xf = S + lane;
    cfptr tp = (cfptr)taps + (size_t)k0 * 8;

    float acc[kStbAcc][kStbSums];
#pragma unroll
    for (int u = 0; u < kStbAcc; u++)
#pragma unroll
        for (int q = 0; q < kStbSums; q++) acc[u][q] = 0.0f;
    const int ng = (k1 - k0) / kStbAcc, rem = (k1 - k0) % kStbAcc;
    for (int i = 0; i < ng; i++) {
#pragma unroll
        for (int u = 0; u < kStbAcc; u++) stb_mac(acc, u, xf, tp + u * 8);
        tp += kStbAcc * 8;
    }
#pragma unroll
    for (int u = 0; u < kStbAcc - 1; u++)             // the part's last 0 .. 7 offsets, accumulators in the same turn
        if (u < rem) stb_mac(acc, u, xf, tp + u * 8);

#pragma unroll
    for (int st = 1; st < kStbAcc; st *= 2)           // pairs, then pairs of pairs
#pragma unroll
        for (int u = 0; u < kStbAcc; u += 2 * st)
#pragma unroll
            for (int q = 0; q < kStbSums; q++) acc[u][q] = acc[u][q] + acc[u + st][q];
#pragma unroll
    for (int q = 0; q < kStbSums; q++) red[(w * kStbSums + q) * 64 + lane] = acc[0][q];
    __syncthreads();
    if (tid >= cnt) return;

    float p[kStbSums];
#pragma unroll
    for (int q = 0; q < kStbSums; q++) {
        const float* r = red + q * 64 + tid;
        p[q] = (r[0] + r[kStbSums * 64]) + (r[2 * kStbSums * 64] + r[3 * kStbSums * 64]);
    }
    static_assert(kStbWaves == 4, "the tree above adds four waves");
    const float s = p[0], zr = p[1], zi = p[2], pr = p[3], pi = p[4];
    const float m = fmaf(pr, pr, pi * pi);
    // conj(P')^2 = (pr^2 - pi^2) - 2 i pr pi;  Im(z' conj(P')^2) = zi (pr^2 - pi^2) - 2 zr pr pi
    const float qr = fmaf(pr, pr, -(pi * pi)), qi = 2.0f * (pr * pi);
    const float im = fmaf(zi, qr, -(zr * qi));
    const float d = m > a.thr2 ? __fdiv_rn(2.0f * im, m) : 0.0f;
    const long col = c0 + tid;
    y[(long)(2 * row) * a.ldy + col] = s + d;
    y[(long)(2 * row + 1) * a.ldy + col] = s - d;
    if (col == a.ncols - 1) level[row] = __fsqrt_rn(m);
}

} // namespace

int stbank_frames(int D, int L)
{
    (void)D;
    (void)L;
    return kStbF;
}

int stbank_slot(int D, int L, int k) { return (k % D) * stb_row(D, L) + k / D; }

void stbank(const StbankCall& c, hipStream_t s)
{
    if (c.n == 0) return;
    const int D = c.D;
    LDSP_REQUIRE(c.C >= 1 && c.C <= kStbankMaxC, "stbank: row count out of range");
    LDSP_REQUIRE(D >= 1 && D <= kStbankMaxD, "stbank: decimation out of range");
    LDSP_REQUIRE(c.L >= 1 && c.L <= kStbankMaxL, "stbank: prototype length out of range");
    LDSP_REQUIRE(c.n < ((size_t)1 << 36), "stbank: call too long");
    LDSP_REQUIRE(c.ldx >= c.n, "stbank: input row stride below the call's length");
    LDSP_REQUIRE(c.skip < (size_t)D && c.ldy >= c.ncols, "stbank: bad call geometry");
    LDSP_REQUIRE(c.ncols == (c.n > c.skip ? (c.n - c.skip + D - 1) / D : 0), "stbank: column count does not match the call");
    StbArgs a;
    a.n = (long)c.n;
    a.ncols = (long)c.ncols;
    a.ldx = (long)c.ldx;
    a.ldy = (long)c.ldy;
    a.skip = (int)c.skip;
    a.D = D;
    a.L = c.L;
    a.ROW = stb_row(D, c.L);
    a.magic = (unsigned)((((uint64_t)1 << 32) + D - 1) / D);
    a.thr2 = c.thr2;
    static_assert(stb_lds(kStbankMaxD, kStbankMaxL) <= 64 * 1024 && stb_lds(1, kStbankMaxL) <= 64 * 1024,
                  "the tile fits the default LDS limit");
    const unsigned grid = (unsigned)std::max<size_t>((c.ncols + kStbF - 1) / kStbF, 1);
    LDSP_PROF(s, "k_stbank");
    hipLaunchKernelGGL(k_stbank, dim3(grid, (unsigned)c.C), dim3(kStbThreads), stb_lds(D, c.L), s, a, c.x, c.hist,
                       c.hist_out, c.taps, c.y, c.level);
    LDSP_HIP(hipGetLastError());
}

} // namespace k
} // namespace ldsp
