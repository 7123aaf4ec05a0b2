// k_synth.hip -- polyphase synthesis filter bank (Synthesizer): M channel rows
// to one dense complex stream, k_chan.hip's counterpart.  The definition is the
// project's own (column n and output t absolute, zeros before column 0):
//   z[t] = scale sum_{k<M} sum_{n : 0 <= t - nD < L} g[t - nD] y[k][n] exp(+2 pi i k t / M)
// computed in polyphase form with Q = ceil(L / D) taps per output residue,
//   v_n[p]    = sum_k rot(k, n) y[k][n] exp(+2 pi i k p / M)                 p < M
//   z[nD + r] = scale sum_{q<Q} g[qD + r] v_{n-q}[(qD + r) mod M]           r < D
// rot = 1 for D = M and (-1)^(k n) for D = M / 2.
//
// A workgroup of NT threads (256; 512 at M = 128, 1024 at M = 256) owns F
// consecutive input columns and writes their F D output samples:
//  1. Columns c0 - (Q - 1) .. c0 + F - 1 of the M rows go to LDS, lanes along a
//     row (a row's read is contiguous), column slots M + 1 samples long.  Columns
//     before the call's first come from the history ([M][Q - 1]), columns past
//     its last are zeros; the D = M / 2 sign is applied on the way.  A column
//     sits at slot (column - c0) + QM - 1, QM the most Q the shape allows, so
//     every index below is a compile-time expression of the thread's number.
//  2. The M-point inverse DFT per column, lane per column, in place: the odd
//     slot length makes the lanes' 8-byte accesses conflict-free.  M <= 16 is one
//     register transform.  M = R1 R2 above that (k_chan's split and its twiddle
//     table): step 1 stored row k = k1 R2 + k2 at k2 R1 + k1; R1-point transforms
//     over k1, the twiddle exp(2 pi i k2 p1 / M), one barrier, then R2-point
//     transforms over k2 leave p = p2 R1 + p1 at its natural place.
//  3. Output sums, lane per output residue: thread (g, r) keeps g[qD + r], q < Q,
//     in registers and sums columns g, g + G, ... (G = NT / D), up to eight at a time,
//     with one fmaf per component and q ascending.  Neighbouring lanes read
//     neighbouring p of one column slot.
//  4. scale, then stores with consecutive lanes on consecutive t.
// Every output runs the same operations in the same order wherever it falls in a
// tile or a call, so an output's bits do not depend on the cut of the column
// stream.  Workgroup 0 also writes the next call's history (the last Q - 1
// columns of history ++ input) into the other buffer of the pair.
#include "chan_dft.hpp"
#include "kernels.hpp"
#include "ldsp_common.hpp"

namespace ldsp {
namespace k {

namespace {

// threads per workgroup: the M >= 128 tiles fill most of a CU's LDS, so one or two
// workgroups are resident, and they bring the waves that hide each other's latency
constexpr int synth_threads(int M) { return M >= 256 ? 1024 : (M >= 128 ? 512 : 256); }

template <int M, int D>
__global__ void __launch_bounds__(synth_threads(M))
    k_synth(const float2* __restrict__ y, long ld, const float2* __restrict__ hist, float2* __restrict__ hist_out,
            long ncols, int par, const float* __restrict__ taps, int Q, const float2* __restrict__ tw, float scale,
            float2* __restrict__ z)
{
    constexpr int NT = synth_threads(M);
    constexpr int F = synth_cols(M);
    constexpr int QM = synth_qmax(M, D);
    constexpr int NC = F + QM - 1;                    // column slots of the tile
    constexpr int R2 = chan_r2(M), R1 = M / R2;
    constexpr int ROW = M + 1;
    constexpr int G = NT / D;                         // columns summed side by side
    constexpr int NF = F / G;                         // columns per thread in the sums
    constexpr int CH = NF < 8 ? NF : 8;                // of them at a time
    static_assert(D <= NT && F % G == 0 && NF >= 1 && NF % CH == 0, "whole chunks per thread");
    __shared__ __attribute__((aligned(16))) float2 S[NC * ROW];
    const int tid = threadIdx.x;
    const int HQ = Q - 1;
    const long c0 = (long)blockIdx.x * F;             // first column of the tile
    const int cnt = (int)min((long)F, ncols - c0);    // > 0: the grid is ceil(ncols / F)

    if (blockIdx.x == 0) {                            // the next call's history
        for (int k = tid / 64; k < M; k += NT / 64)
            for (int j = tid % 64; j < HQ; j += 64) {
                const long c = ncols - HQ + j;
                hist_out[k * HQ + j] = c < 0 ? hist[k * HQ + (int)(c + HQ)] : y[(long)k * ld + c];
            }
    }

    // 1. S[s ROW + pos(k)] = rot(k, n) y[k][n], n = c0 - (QM - 1) + s; a thread's loads (12 to 25)
    //    are all issued before its first LDS store
    constexpr int NL = M * NC, B = (NL + NT - 1) / NT;
    static_assert(B <= 26, "the tile's loads are held in registers");
    for (int base = 0; base < NL; base += NT * B) {
        float2 v[B];
#pragma unroll
        for (int i = 0; i < B; i++) {
            const int it = base + tid + NT * i;
            const int k = it / NC, s = it - k * NC;
            const long col = c0 - (QM - 1) + s;
            const bool in = it < NL && col >= 0 && col < ncols;
            const bool hi = it < NL && col < 0 && col >= -(long)HQ;
            const float2* src = in ? y + ((long)k * ld + col) : hist + (hi ? k * HQ + (int)(col + HQ) : 0);
            float2 t = *src;
            if (!(in || hi)) t = make_float2(0.0f, 0.0f);
            if (D != M && (k & 1) && ((par + (int)(col & 1)) & 1)) t = make_float2(-t.x, -t.y);
            v[i] = t;
        }
#pragma unroll
        for (int i = 0; i < B; i++) {
            const int it = base + tid + NT * i;
            const int k = it / NC, s = it - k * NC;
            const int pos = R2 == 1 ? k : (k % R2) * R1 + k / R2;
            if (it < NL) S[s * ROW + pos] = v[i];
        }
    }
    __syncthreads();

    // 2. the inverse DFT of every slot in use
    const int s0 = QM - Q;
    if constexpr (R2 > 1) {
        for (int it = tid; it < NC * R2; it += NT) {
            const int s = it % NC, k2 = it / NC;
            if (s < s0) continue;
            float2* row = S + s * ROW + k2 * R1;
            float2 v[R1];
#pragma unroll
            for (int k1 = 0; k1 < R1; k1++) v[k1] = row[k1];
            chan_idft<R1>(v);
#pragma unroll
            for (int p1 = 1; p1 < R1; p1++) v[p1] = cmul(v[p1], tw[k2 * p1]);
#pragma unroll
            for (int p1 = 0; p1 < R1; p1++) row[p1] = v[p1];
        }
        __syncthreads();
        for (int it = tid; it < NC * R1; it += NT) {
            const int s = it % NC, p1 = it / NC;
            if (s < s0) continue;
            float2* row = S + s * ROW + p1;
            float2 v[R2];
#pragma unroll
            for (int k2 = 0; k2 < R2; k2++) v[k2] = row[k2 * R1];
            chan_idft<R2>(v);
#pragma unroll
            for (int p2 = 0; p2 < R2; p2++) row[p2 * R1] = v[p2];
        }
    } else {
        for (int s = tid; s < NC; s += NT) {
            if (s < s0) continue;
            float2* row = S + s * ROW;
            float2 v[M];
#pragma unroll
            for (int k = 0; k < M; k++) v[k] = row[k];
            chan_idft<M>(v);
#pragma unroll
            for (int p = 0; p < M; p++) row[p] = v[p];
        }
    }
    __syncthreads();

    // 3, 4. z[(c0 + f) D + r] = scale sum_q g[qD + r] v_{f - q}[(qD + r) mod M]
    const int r = tid % D, g = tid / D;
    float gq[QM];                                     // taps holds kChanMaxP * M = QM * D floats, zero past L
#pragma unroll
    for (int q = 0; q < QM; q++) gq[q] = taps[q * D + r];
    const float2* Sb = S + (g + QM - 1) * ROW + r;
    float2* zb = z + (c0 + g) * D + r;
    for (int j = 0; j < NF; j += CH) {
        if (j * G >= cnt) break;
        float2 acc[CH];
#pragma unroll
        for (int i = 0; i < CH; i++) acc[i] = make_float2(0.0f, 0.0f);
#pragma unroll
        for (int q = 0; q < QM; q++) {
            if (q < Q) {
                const float h = gq[q];
                const float2* sp = Sb + (j * G - q) * ROW + ((D != M && (q & 1)) ? D : 0);
#pragma unroll
                for (int i = 0; i < CH; i++) {
                    const float2 v = sp[i * G * ROW];
                    acc[i].x = fmaf(h, v.x, acc[i].x);
                    acc[i].y = fmaf(h, v.y, acc[i].y);
                }
            }
        }
#pragma unroll
        for (int i = 0; i < CH; i++) {
            const int f = g + G * (j + i);
            if (f < cnt) zb[(long)G * (j + i) * D] = make_float2(acc[i].x * scale, acc[i].y * scale);
        }
    }
}

template <int M, int D>
void synth_launch(const SynthCall& c, hipStream_t s)
{
    constexpr int F = synth_cols(M);
    const unsigned grid = (unsigned)((c.ncols + F - 1) / F);
    hipLaunchKernelGGL((k_synth<M, D>), dim3(grid), dim3(synth_threads(M)), 0, s, (const float2*)c.y, (long)c.ld,
                       (const float2*)c.hist, (float2*)c.hist_out, (long)c.ncols, c.parity, c.taps, c.Q,
                       (const float2*)c.tw, c.scale, (float2*)c.z);
}

} // namespace

#define LDSP_SYNTH_CASE(m)                                     \
    case m:                                                    \
        if (D == m) {                                          \
            LDSP_PROF(s, "k_synth_m" #m "_crit");              \
            synth_launch<m, m>(c, s);                          \
        } else {                                               \
            LDSP_PROF(s, "k_synth_m" #m "_os2");               \
            synth_launch<m, m / 2>(c, s);                      \
        }                                                      \
        break

void synth(int M, int D, const SynthCall& c, hipStream_t s)
{
    if (c.ncols == 0) return;
    LDSP_REQUIRE(D == M || 2 * D == M, "synth: interpolation must be M or M / 2");
    LDSP_REQUIRE(c.Q >= 1 && c.Q <= kChanMaxP * (M / D), "synth: taps per residue out of range");
    LDSP_REQUIRE(c.ncols < ((size_t)1 << 36), "synth: call too long");
    LDSP_REQUIRE(c.ld >= c.ncols, "synth: bad call geometry");
    switch (M) {
        LDSP_SYNTH_CASE(4);
        LDSP_SYNTH_CASE(8);
        LDSP_SYNTH_CASE(16);
        LDSP_SYNTH_CASE(32);
        LDSP_SYNTH_CASE(64);
        LDSP_SYNTH_CASE(128);
        LDSP_SYNTH_CASE(256);
    default:
        throw Error(LDSP_EINVAL, "synth: channel count must be a power of two in 4 .. 256");
    }
    LDSP_HIP(hipGetLastError());
}
#undef LDSP_SYNTH_CASE

} // namespace k
} // namespace ldsp
