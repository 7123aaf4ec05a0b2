// k_spgram.hip -- streaming Welch periodogram (Spectrogram): one complex stream
// to rows of |X|^2.  No reference counterpart (liquid's spgramcf is the same
// block); the definition is the project's own (ldsp.h):
//   X_s[k] = sum_{i<W} w[i] x[(s + 1) d - W + i] exp(-2 pi i k i / N)     k < N
//   P_s[k] = re(X_s[k])^2 + im(X_s[k])^2
//   row r  = (1 / A) sum_{s = rA}^{rA + A - 1} P_s
// with s the transform's index since reset.
//
// A workgroup is one wave.  It owns a run of consecutive rows, i.e. of
// consecutive transforms, and for each transform
//  1. loads the W window samples with unit stride (lane l holds points l + 64 i,
//     i < N / 64), history before the call's first sample, and multiplies by the
//     window on the way in; points W .. N - 1 are zero.  Consecutive windows of a
//     wave overlap by W - d samples: those come from this CU's L1 / L2, the
//     stream is read from HBM once;
//  2. runs the N-point transform as a Stockham autosort of register radices
//     (fft_butterflies.hpp) over the points a lane holds: a butterfly of radix r
//     takes points t + (N / r) j, which are lane t % 64's own at every pass, and
//     writes q + s (r p + k) (t = q + s p, s the product of the earlier radices)
//     times exp(-2 pi i s p k / N) from the host's table (in LDS; N = 4096: see
//     sp_pass).  Passes exchange through the wave's padded LDS buffer; the last
//     leaves lane l holding bins l + 64 i, the layout of a row store with unit
//     stride;
//  3. adds |X|^2 to the row's sum, in registers, and to the run's sum (in
//     registers up to N = 1024).
// No spectrum reaches memory.
//
// A row is the sum of its transforms in ascending order from zero, by one wave,
// whichever workgroup or call that is: a row the call does not finish leaves its
// partial sum in the carry buffer (float32[N], ping-ponged) and the next call's
// first row continues from it.  A row's bits therefore do not depend on how the
// stream is cut into calls or rows into workgroups.  The run's sum goes to
// part[workgroup][N]; k_spgram_psd adds the runs to the float64 accumulator in a
// fixed order (16 interleaved slices in ascending order, then the slices in
// order): no atomics, and the same for a call with and without row stores.
// An average of 16 or more transforms that is a multiple of kSpgramBlock = 8
// would leave one wave with the whole row, so it is summed in two levels of the
// same kind: this kernel sums blocks of 8 transforms (its "rows", aligned to
// the row's first transform), and k_spgram_rows adds a row's blocks in order,
// with a carried sum of its own.  The shape depends on A and on absolute
// transform indices alone, as before.
// Workgroup 0 also writes the next call's history (the last W - 1 samples of
// history ++ input) into the other buffer of the pair.
#include "fft_butterflies.hpp"
#include "kernels.hpp"
#include "ldsp_common.hpp"
#include "ldsp_math.hpp"

#include <type_traits>

// The int16-IQ instantiations are built from this file in a translation unit of
// their own (k_spgram_iq16.hip defines LDSP_SPGRAM_IQ16): a second set of
// kernels beside the complex64 ones moves their LDS arrays and, with that, the
// compiler's schedule of the complex64 code.
#ifndef LDSP_SPGRAM_IQ16
#define LDSP_SPGRAM_IQ16 0
#endif

namespace ldsp {
namespace k {

void spgram_iq16(int N, const SpgramCall& c, long rg, unsigned grid, hipStream_t s);   // k_spgram_iq16.hip

namespace {

constexpr bool kSpIq16 = LDSP_SPGRAM_IQ16 != 0;

__device__ __forceinline__ int sp_pad(int i) { return i + (i >> 4); }
__device__ __forceinline__ void sp_lds_sync() { asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); }

template <int RAD>
__device__ __forceinline__ void sp_dft(float2 (&a)[RAD])
{
    static_assert(RAD == 4 || RAD == 8 || RAD == 16, "register transforms: 4, 8, 16 points");
    if constexpr (RAD == 4) dft4(a[0], a[1], a[2], a[3]);
    else if constexpr (RAD == 8) dft8(a);
    else dft16(a);
}

// One Stockham pass of radix RAD at stride S over v[i] = data[lane + 64 i]; the
// result is in the same layout.  tw[j] = exp(-2 pi i j / N).
// SPLIT (N = 4096, where the whole table does not fit beside the exchange buffer):
// S divides 64, so S p = (lane - q) + 64 u and the factor is the product of
// tw[(lane - q) k], an index below 1024 and the part of the table that is in LDS,
// and tw[64 u k], the same for all lanes and read from twg with scalar loads.
template <int N, int RAD, int S, bool SPLIT>
__device__ __forceinline__ void sp_pass(float2 (&v)[N / 64], float2* d, const float2* tw, const float2* twg, int lane)
{
    constexpr int R = N / 64, NB = R / RAD;
    constexpr bool LAST = S * RAD == N;
    static_assert(NB >= 1 && N % (S * RAD) == 0, "a lane holds whole butterflies");
#pragma unroll
    for (int u = 0; u < NB; u++) {
        float2 a[RAD];
#pragma unroll
        for (int j = 0; j < RAD; j++) a[j] = v[u + NB * j];
        sp_dft<RAD>(a);
        if constexpr (LAST) {
#pragma unroll
            for (int k = 0; k < RAD; k++) v[u + NB * k] = a[k];
        } else {
            const int t = lane + 64 * u;
            const int q = t & (S - 1), sp = t - q;          // sp = S p
            if constexpr (!SPLIT) {
#pragma unroll
                for (int k = 1; k < RAD; k++) a[k] = cmul(a[k], tw[sp * k]);
            } else {
                static_assert(64 % S == 0 && 63 * (RAD - 1) < 1024 && 64 * (N / 64 / RAD - 1) * (RAD - 1) < N, "split table");
                const int sl = lane - q;
#pragma unroll
                for (int k = 1; k < RAD; k++) {
                    a[k] = cmul(a[k], tw[sl * k]);
                    if (u > 0) a[k] = cmul(a[k], twg[64 * u * k]);
                }
            }
            const int o = q + RAD * sp;
#pragma unroll
            for (int k = 0; k < RAD; k++) d[sp_pad(o + S * k)] = a[k];
        }
    }
    if constexpr (!LAST) {
        sp_lds_sync();
#pragma unroll
        for (int i = 0; i < R; i++) v[i] = d[sp_pad(lane + 64 * i)];
        sp_lds_sync();
    }
}

// forward N-point transform of v[i] = data[lane + 64 i]; on return v[i] = X[lane + 64 i]
// The table sits in LDS up to N = 2048; at 4096 it and the exchange buffer
// together would leave two waves per CU, so only its first 1024 entries do.
constexpr bool sp_tw_lds(int N) { return N <= 2048; }
constexpr int sp_tw_slots(int N) { return sp_tw_lds(N) ? N : 1024; }

// tw: the table in LDS (sp_tw_slots entries); twg: the whole table in memory
template <int N>
__device__ __forceinline__ void sp_fft(float2 (&v)[N / 64], float2* d, const float2* tw, const float2* twg, int lane)
{
    constexpr bool SP = !sp_tw_lds(N);
    if constexpr (N == 256) {
        sp_pass<N, 4, 1, SP>(v, d, tw, twg, lane);
        sp_pass<N, 4, 4, SP>(v, d, tw, twg, lane);
        sp_pass<N, 4, 16, SP>(v, d, tw, twg, lane);
        sp_pass<N, 4, 64, SP>(v, d, tw, twg, lane);
    } else if constexpr (N == 512) {
        sp_pass<N, 8, 1, SP>(v, d, tw, twg, lane);
        sp_pass<N, 8, 8, SP>(v, d, tw, twg, lane);
        sp_pass<N, 8, 64, SP>(v, d, tw, twg, lane);
    } else {
        static_assert(N == 1024 || N == 2048 || N == 4096, "transform sizes: 256 .. 4096");
        sp_pass<N, 16, 1, SP>(v, d, tw, twg, lane);
        sp_pass<N, 16, 16, SP>(v, d, tw, twg, lane);
        sp_pass<N, N / 256, 256, SP>(v, d, tw, twg, lane);
    }
}

// One point of an int16 call's window that may begin in the history: src is the
// first word of a (complex64) history sample if hist, else the word of an (I, Q)
// pair.  Without branches: two 4-byte loads, the halves of the history sample
// or the pair's word twice.
__device__ __forceinline__ float2 sp_point(const int* src, bool hist)
{
    const int lo = src[0], hi = src[hist ? 1 : 0];
    const float2 c = iq_sample(lo);
    return hist ? make_float2(bitsf((uint32_t)lo), bitsf((uint32_t)hi)) : c;
}

// IQ16: x holds int16 (I, Q) pairs, one 4-byte word per sample, converted where
// they are loaded (iq_sample); the history stays complex64, so the calls of one
// stream may be of either kind.
template <int N, bool IQ16>
__global__ void __launch_bounds__(64) k_spgram(const std::conditional_t<IQ16, int, float2>* __restrict__ x,
                                               const float2* __restrict__ hist, float2* __restrict__ hist_out, long n,
                                               int W, int d, long A, long a0, long nt, long base, long rg,
                                               const float* __restrict__ win, const float2* __restrict__ tw,
                                               const float* __restrict__ carry_in, float* __restrict__ carry_out,
                                               float inv_a, float* __restrict__ y, long ld, float* __restrict__ part)
{
    using X = std::conditional_t<IQ16, int, float2>;
    constexpr int R = N / 64;
    __shared__ float2 buf[N + N / 16];
    __shared__ float2 ltw[sp_tw_slots(N)];
    const int lane = threadIdx.x;
    const int H = W - 1;
    if (blockIdx.x == 0) {                            // the next call's history
        for (int j = lane; j < H; j += 64) {
            const long g = n - H + j;
            if constexpr (IQ16) hist_out[j] = g < 0 ? hist[g + H] : iq_sample(x[g]);
            else hist_out[j] = g < 0 ? hist[g + H] : x[g];
        }
    }
    if (nt <= 0) return;                              // a call that takes no transform: history only
    for (int j = lane; j < sp_tw_slots(N); j += 64) ltw[j] = tw[j];
    __syncthreads();
    // the window (zero from W on) stays in registers where they are not needed for the points
    constexpr bool WREG = N <= 1024;
    // and so does the run's sum; above that the run's sum is kept in its place in
    // part (each lane its own floats, written before they are added to): a row
    // begun here adds its sum when it ends, the carried row every transform
    float* __restrict__ pr = part + (long)blockIdx.x * N;
    bool pfirst = true;
    float wv[WREG ? R : 1], pacc[WREG ? R : 1];
    if constexpr (WREG) {
#pragma unroll
        for (int i = 0; i < R; i++) {
            wv[i] = win[lane + 64 * i];
            pacc[i] = 0.0f;
        }
    }
    const long rows = (a0 + nt + A - 1) / A;          // rows the call touches, the unfinished last one included
    const long r0 = (long)blockIdx.x * rg, r1 = min(rows, r0 + rg);
    for (long r = r0; r < r1; r++) {
        const long first = r * A - a0;                // the row's transforms, relative to the call's first
        const long lo = max(first, 0L), hi = min(first + A, nt);
        // lane offsets are formed where they are used (32-bit, beside a uniform
        // base): kept across the loops as 64-bit addresses they would take more
        // registers than the points themselves
        unsigned lr = lane;
        asm volatile("" : "+v"(lr));
        float acc[R];
        if (first < 0) {                              // begun by an earlier call
#pragma unroll
            for (int i = 0; i < R; i++) acc[i] = carry_in[lr + 64u * i];
        } else {
#pragma unroll
            for (int i = 0; i < R; i++) acc[i] = 0.0f;
        }
        for (long s = lo; s < hi; s++) {
            const long g0 = base + s * d;             // the window's first sample, relative to x[0]; > -W
            unsigned ln = lane;                        // LDS and table offsets likewise
            asm volatile("" : "+v"(ln));
            float2 v[R];
            if (g0 >= 0 && W == N) {                  // no history, no padding
                const X* __restrict__ xb = x + g0;
#pragma unroll
                for (int i = 0; i < R; i++) {
                    const unsigned j = ln + 64u * i;
                    const float2 e = iq_sample(xb[j]);
                    const float w = WREG ? wv[WREG ? i : 0] : win[j];
                    v[i] = make_float2(e.x * w, e.y * w);
                }
            } else {
                // without branches: every lane loads a sample of the window (the
                // last one again from W on) and the padding is selected afterwards
#pragma unroll
                for (int i = 0; i < R; i++) {
                    const unsigned j = ln + 64u * i;
                    const long g = g0 + min(j, (unsigned)H);
                    const X* __restrict__ src = g < 0 ? (const X*)(hist + (g + H)) : x + g;
                    float2 e;
                    if constexpr (IQ16) e = sp_point(src, g < 0);
                    else e = *src;
                    const float w = WREG ? wv[WREG ? i : 0] : win[j];
                    v[i] = j < (unsigned)W ? make_float2(e.x * w, e.y * w) : make_float2(0.0f, 0.0f);
                }
            }
            sp_fft<N>(v, buf, ltw, tw, (int)ln);
#pragma unroll
            for (int i = 0; i < R; i++) {
                const float p = fmaf(v[i].x, v[i].x, v[i].y * v[i].y);
                acc[i] += p;
                if constexpr (WREG) pacc[i] += p;
                else if (first < 0) pr[ln + 64u * i] = pfirst ? p : pr[ln + 64u * i] + p;   // this call's part alone
            }
            if (!WREG && first < 0) pfirst = false;
        }
        if constexpr (!WREG) {
            if (first >= 0) {                         // a row begun here: its sum is this call's part
#pragma unroll
                for (int i = 0; i < R; i++) pr[lr + 64u * i] = pfirst ? acc[i] : pr[lr + 64u * i] + acc[i];
                pfirst = false;
            }
        }
        if (first + A <= nt) {
            if (y) {
                float* __restrict__ yr = y + r * ld;
#pragma unroll
                for (int i = 0; i < R; i++) yr[lr + 64u * i] = acc[i] * inv_a;
            }
        } else {
#pragma unroll
            for (int i = 0; i < R; i++) carry_out[lr + 64u * i] = acc[i];
        }
    }
    if constexpr (WREG) {
#pragma unroll
        for (int i = 0; i < R; i++) pr[lane + 64 * i] = pacc[i];
    }
}

template <int N>
void spgram_launch(const SpgramCall& c, long rg, unsigned grid, hipStream_t s)
{
    hipLaunchKernelGGL((k_spgram<N, kSpIq16>), dim3(grid), dim3(64), 0, s,
                       (const std::conditional_t<kSpIq16, int, float2>*)c.x, (const float2*)c.hist, (float2*)c.hist_out,
                       (long)c.n, c.W, c.d, (long)c.A, (long)c.a0, (long)c.nt, (long)c.base, rg, c.win,
                       (const float2*)c.tw, c.carry_in, c.carry_out, c.scale, c.y, (long)c.ld, c.part);
}

#define LDSP_SPGRAM_CASE(m)                          \
    case m: {                                        \
        LDSP_PROF(s, "k_spgram_n" #m);               \
        spgram_launch<m>(c, rg, grid, s);            \
    } break

// the main kernel of a call, this translation unit's kind of input
void spgram_main(int N, const SpgramCall& c, long rg, unsigned grid, hipStream_t s)
{
    switch (N) {
        LDSP_SPGRAM_CASE(256);
        LDSP_SPGRAM_CASE(512);
        LDSP_SPGRAM_CASE(1024);
        LDSP_SPGRAM_CASE(2048);
        LDSP_SPGRAM_CASE(4096);
    default:
        throw Error(LDSP_EINVAL, "spgram: nfft must be a power of two in 256 .. 4096");
    }
    LDSP_HIP(hipGetLastError());
}
#undef LDSP_SPGRAM_CASE

#if !LDSP_SPGRAM_IQ16
// psd[k] += sum_b part[b][k]: slice j of 16 adds runs j, j + 16, ... in ascending
// order, then the slices are added in order.
constexpr int kSpSlices = 16;
__global__ void __launch_bounds__(64 * kSpSlices) k_spgram_psd(const float* __restrict__ part, long nb, int N,
                                                               double* __restrict__ psd)
{
    __shared__ double sl[kSpSlices][64];
    const int c = threadIdx.x & 63, j = threadIdx.x >> 6;
    const int k = blockIdx.x * 64 + c;
    double a = 0.0;
    for (long b = j; b < nb; b += kSpSlices) a += (double)part[b * N + k];
    sl[j][c] = a;
    __syncthreads();
    if (j == 0) {
        double s = sl[0][c];
#pragma unroll
        for (int i = 1; i < kSpSlices; i++) s += sl[i][c];
        psd[k] += s;
    }
}

// Rows of a blocked average (A = M kSpgramBlock): the call's nb finished block
// sums, of which the first row had c0 before the call, are added row by row in
// ascending order from zero, or from the carried sum of a row begun by an earlier
// call.  Thread per bin and row.
__global__ void __launch_bounds__(256) k_spgram_rows(const float* __restrict__ blk, long nb, long M, long c0, int N,
                                                     const float* __restrict__ carry_in, float* __restrict__ carry_out,
                                                     float inv_a, float* __restrict__ y, long ld)
{
    const int k = blockIdx.x * 256 + threadIdx.x;     // N is a multiple of 256
    const long r = blockIdx.y;
    const long first = r * M - c0;
    const long lo = max(first, 0L), hi = min(first + M, nb);
    float acc = first < 0 ? carry_in[k] : 0.0f;
    for (long j = lo; j < hi; j++) acc += blk[j * N + k];
    if (first + M <= nb) {
        if (y) y[r * ld + k] = acc * inv_a;
    } else {
        carry_out[k] = acc;
    }
}

#endif

} // namespace

#if LDSP_SPGRAM_IQ16
void spgram_iq16(int N, const SpgramCall& c, long rg, unsigned grid, hipStream_t s) { spgram_main(N, c, rg, grid, s); }
#else

size_t spgram_runs(int N, size_t A, size_t a0, size_t nt, size_t* rows_per_run)
{
    if (nt == 0) {
        if (rows_per_run) *rows_per_run = 1;
        return 0;
    }
    const size_t rows = (a0 + nt + A - 1) / A;
    size_t rg = std::max<size_t>((size_t)spgram_tile(N) / A, 1);
    rg = std::max(rg, (rows + kSpgramMaxRuns - 1) / kSpgramMaxRuns);
    if (rows_per_run) *rows_per_run = rg;
    return (rows + rg - 1) / rg;
}

void spgram_rows(int N, const float* blk, size_t nb, size_t M, size_t c0, const float* carry_in, float* carry_out,
                 size_t A, float* y, size_t ld, hipStream_t s)
{
    if (nb == 0) return;
    LDSP_REQUIRE(N % 256 == 0 && M >= 1 && c0 < M && carry_in != carry_out, "spgram_rows: bad call geometry");
    LDSP_REQUIRE(y == nullptr || ld >= (size_t)N, "spgram_rows: row stride below nfft");
    const size_t rows = (c0 + nb + M - 1) / M;
    LDSP_REQUIRE(rows <= 65535, "spgram_rows: too many rows in one launch");
    LDSP_PROF(s, "k_spgram_rows");
    hipLaunchKernelGGL(k_spgram_rows, dim3(N / 256, (unsigned)rows), dim3(256), 0, s, blk, (long)nb, (long)M, (long)c0,
                       N, carry_in, carry_out, 1.0f / (float)A, y, (long)ld);
    LDSP_HIP(hipGetLastError());
}

void spgram(int N, const SpgramCall& c, hipStream_t s)
{
    if (c.n == 0) return;
    LDSP_REQUIRE(c.W >= 1 && c.W <= N && c.d >= 1 && c.d <= c.W && c.A >= 1, "spgram: bad window, hop or average");
    LDSP_REQUIRE(c.n < ((size_t)1 << 41), "spgram: call too long");
    LDSP_REQUIRE(c.a0 < c.A && c.base > -(long long)c.W, "spgram: bad call geometry");
    LDSP_REQUIRE(c.nt == 0 || c.base + (long long)(c.nt - 1) * c.d + c.W <= (long long)c.n,
                 "spgram: the last window passes the end of the call");
    LDSP_REQUIRE(c.y == nullptr || c.ld >= (size_t)N, "spgram: row stride below nfft");
    size_t rg = 1;
    const size_t runs = spgram_runs(N, c.A, c.a0, c.nt, &rg);
    const unsigned grid = (unsigned)std::max<size_t>(runs, 1);
    if (c.iq16) spgram_iq16(N, c, (long)rg, grid, s);
    else spgram_main(N, c, (long)rg, grid, s);
    if (runs > 0) {
        LDSP_PROF(s, "k_spgram_psd");
        hipLaunchKernelGGL(k_spgram_psd, dim3(N / 64), dim3(64 * kSpSlices), 0, s, (const float*)c.part, (long)runs, N,
                           c.psd);
        LDSP_HIP(hipGetLastError());
    }
}
#endif

} // namespace k
} // namespace ldsp
