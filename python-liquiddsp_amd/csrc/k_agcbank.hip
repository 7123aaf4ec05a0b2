// k_agcbank.hip -- look-ahead hang AGC over the rows of a bank (AGCBank): per
// row and per block of B samples the peak, an integer level tracker (instant
// attack, a hang of H blocks, then d per block) and a gain that ramps over one
// block towards min(g_b, g_{b+1}).  The definition is the project's own
// (include/ldsp.h); levels are int32 in units of 2^-24 octave (agc_track.hpp).
//
// A row's stream in a call is its `fill` carried samples (the object's history
// buffer, [C][2B]) followed by the call's n.  The carried samples are the ones
// not yet emitted: the block tracked last (pend = 1 once the stream holds one)
// and the unfinished block after it.  The call tracks the nt whole blocks that
// start at stream position off = pend B and emits the ne blocks from position 0.
// Three plain launches, no workgroup waits on another:
//
// k_agcbank_peak<CX>: k_sqbank_power's geometry.  The grid is (tiles, rows); a
//   workgroup of 256 threads owns TILE consecutive blocks of one row, G lanes
//   share a block (G: the smallest power of two that holds the block's 16-byte
//   vectors, 8 .. 64) and the 256 / G groups take the tile's blocks round-robin.
//   A vector is four float32 or two complex64 samples at the row's element
//   alignment; four are in flight per lane.  The block that starts in the carried
//   samples is read one sample per lane.  A maximum has no order, so a block's
//   peak has the same bits wherever it falls.  Lane 0 of the group quantises:
//   one double log2 per block.  Tile 0 writes the row's next carry into the
//   other buffer of the pair.
// k_agcbank_track: one workgroup of 256 lanes per row, a pass of P = 2048 blocks
//   at a time.  The pass's peaks and the H before them go to LDS; the hang
//   window's running maximum is taken by doubling between two LDS arrays; lane t
//   folds its eight consecutive window maxima into a pair, the pairs are scanned
//   by shuffles within a wave and the four wave totals combined through LDS;
//   every lane then walks its eight blocks from the level before them and stores
//   gain_q and g.  The level after a pass is the total every lane has computed,
//   so passes chain through registers.  The lane that owns the last block
//   writes the row's state.
// k_agcbank_apply<CX>: the peak kernel's geometry over the emitted blocks: 16
//   bytes in, 16 bytes out per lane, gamma in float32 from the boundary gains.
#include <cmath>

#include "agc_track.hpp"
#include "kernels.hpp"
#include "ldsp_common.hpp"

namespace ldsp {
namespace k {

namespace {

using namespace ldsp::agc;

constexpr int kAgThreads = 256;
constexpr int kAgTileSamples = 8192;          // a tile is about this many samples
constexpr int kAgPer = 8;                     // consecutive blocks per lane of the track kernel
constexpr int kAgPass = kAgThreads * kAgPer;  // blocks per pass
constexpr int kAgHalo = 256;                  // LDS entries in front of a pass (>= kAgcMaxHang, 16-byte multiple)

typedef float AgF4 __attribute__((ext_vector_type(4)));
typedef AgF4 AgVecR __attribute__((aligned(4)));    // four float32 at a float row's alignment
typedef AgF4 AgVecC __attribute__((aligned(8)));    // two complex64 at a complex row's alignment
typedef int AgI4 __attribute__((ext_vector_type(4)));

template <bool CX>
struct AgT {
    using elem = float;
    using vec = AgVecR;
    using acc = float;
    static constexpr int V = 4;
};
template <>
struct AgT<true> {
    using elem = float2;
    using vec = AgVecC;
    using acc = double;
    static constexpr int V = 2;
};

struct AgArgs {
    long n, ldx, nt, ne;          // the call's samples, input row stride, blocks tracked and emitted
    int fill, carry, off;         // carried samples before / after the call; where the first new block starts
    int B, G, T;
};

// lanes that share a block: its B / V vectors
constexpr int ag_lanes(int B, int V)
{
    int g = 8;
    while (g < 64 && g * V < B) g *= 2;
    return g;
}

// |x| of a real sample, |x|^2 in double of a complex one; a NaN or Inf sample counts as 0
__device__ __forceinline__ float ag_mag(float x)
{
    const float a = fabsf(x);
    return a < INFINITY ? a : 0.0f;
}
__device__ __forceinline__ double ag_mag(float2 x)
{
    const double m = (double)x.x * (double)x.x + (double)x.y * (double)x.y;
    return m < (double)INFINITY ? m : 0.0;
}
__device__ __forceinline__ float ag_vmag(const AgF4& v, float)
{
    return fmaxf(fmaxf(ag_mag(v.x), ag_mag(v.y)), fmaxf(ag_mag(v.z), ag_mag(v.w)));
}
__device__ __forceinline__ double ag_vmag(const AgF4& v, double)
{
    return fmax(ag_mag(make_float2(v.x, v.y)), ag_mag(make_float2(v.z, v.w)));
}
__device__ __forceinline__ float ag_max(float a, float b) { return fmaxf(a, b); }
__device__ __forceinline__ double ag_max(double a, double b) { return fmax(a, b); }
__device__ __forceinline__ double ag_amp(float a) { return (double)a; }
__device__ __forceinline__ double ag_amp(double m) { return sqrt(m); }

// peak_q = clamp(ceil(log2(a) Q), floor, ceil); the floor for a = 0
__device__ __forceinline__ int32_t ag_quantise(double a)
{
    if (!(a > 0.0)) return kAgcFloor;
    const double t = ceil(log2(a) * kAgcQ);
    return (int32_t)fmin(fmax(t, (double)kAgcFloor), (double)kAgcCeil);
}

// Sample p of a row's stream: one of the `fill` carried samples, then x
template <class E>
__device__ __forceinline__ E ag_at(const E* __restrict__ xr, const E* __restrict__ hr, int fill, long p)
{
    return p < fill ? hr[p] : xr[p - fill];
}

template <bool CX>
__global__ void __launch_bounds__(kAgThreads)
    k_agcbank_peak(const AgArgs a, const typename AgT<CX>::elem* __restrict__ x,
                   const typename AgT<CX>::elem* __restrict__ hist, typename AgT<CX>::elem* __restrict__ hist_out,
                   int32_t* __restrict__ pq, long ldq)
{
    using E = typename AgT<CX>::elem;
    using Vec = typename AgT<CX>::vec;
    using Acc = typename AgT<CX>::acc;
    constexpr int V = AgT<CX>::V;
    const int tid = threadIdx.x;
    const int B = a.B, G = a.G, fill = a.fill;
    const int row = blockIdx.y;
    const E* __restrict__ xr = x + (long)row * a.ldx;
    const E* __restrict__ hr = hist + (long)row * 2 * B;

    if (blockIdx.x == 0) {                            // the row's next carry: the last a.carry samples of its stream
        E* __restrict__ ho = hist_out + (long)row * 2 * B;
        const long first = (long)fill + a.n - a.carry;
        for (int i = tid; i < a.carry; i += kAgThreads) ho[i] = ag_at(xr, hr, fill, first + i);
    }
    if (a.nt == 0) return;                            // a call too short for a block: the carry only

    const int l = tid & (G - 1), gi = tid / G, NG = kAgThreads / G;
    const int nvec = B / V, rem = B - nvec * V;
    const long t0 = (long)blockIdx.x * a.T;
    for (int it = 0; it < a.T; it += NG) {
        const long blk = t0 + it + gi;
        const bool valid = blk < a.nt;
        const long s0 = a.off + blk * B;              // the block's first sample in the stream
        Acc acc = 0;
        if (valid) {
            if (s0 >= fill) {
                const E* __restrict__ xb = xr + (s0 - fill);
                for (int j = l; j < nvec; j += 4 * G) {
                    // four vectors in flight; one past the block's end is read at the last vector's
                    // place, which a maximum does not notice
                    AgF4 v[4];
#pragma unroll
                    for (int u = 0; u < 4; u++) v[u] = *reinterpret_cast<const Vec*>(xb + V * min(j + u * G, nvec - 1));
#pragma unroll
                    for (int u = 0; u < 4; u++) acc = ag_max(acc, ag_vmag(v[u], Acc()));
                }
                if (l < rem) acc = ag_max(acc, ag_mag(xb[nvec * V + l]));
            } else {                                  // the block that starts in the carried samples
                for (int i = l; i < B; i += G) acc = ag_max(acc, ag_mag(ag_at(xr, hr, fill, s0 + i)));
            }
        }
        for (int m = G >> 1; m > 0; m >>= 1) acc = ag_max(acc, __shfl_xor(acc, m, 64));
        if (valid && l == 0) pq[(long)row * ldq + blk] = ag_quantise(ag_amp(acc));
    }
}

struct AgTrackArgs {
    long nt, ldq, ldg;
    long d;                       // decay per block, units
    int H, pend;
    int32_t Gmax;
};

__device__ __forceinline__ float ag_gain(int32_t gq) { return (float)exp2((double)gq * (1.0 / kAgcQ)); }

__global__ void __launch_bounds__(kAgThreads)
    k_agcbank_track(const AgTrackArgs a, const int32_t* __restrict__ target, int32_t* __restrict__ level,
                    int32_t* __restrict__ tail, float* __restrict__ edge, const int32_t* __restrict__ pq,
                    int32_t* __restrict__ gq, float* __restrict__ gb)
{
    __shared__ __attribute__((aligned(16))) int32_t A[2][kAgHalo + kAgPass];
    __shared__ int32_t wv_s[kAgThreads / 64], wn_s[kAgThreads / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row = blockIdx.x;
    const int H = a.H;
    const long d = a.d;
    const int32_t* __restrict__ pr = pq + (long)row * a.ldq;
    int32_t* __restrict__ gr = gq + (long)row * a.ldq;
    float* __restrict__ br = gb + (long)row * a.ldg;
    int32_t* __restrict__ tr = tail + (long)row * kAgHalo;
    const int32_t T = target[row];
    const float hprev_old = edge[2 * row], glast_old = edge[2 * row + 1];
    int32_t L = level[row];

    for (long base = 0; base < a.nt; base += kAgPass) {
        // the pass's peaks behind the H before them; the floor elsewhere
        for (int i = tid; i < kAgHalo + kAgPass; i += kAgThreads) {
            const long s = base + i - kAgHalo;
            int32_t v = kAgcFloor;
            if (i >= kAgHalo - H) {
                if (s >= 0) v = s < a.nt ? pr[s] : kAgcFloor;
                else v = tr[i];                       // the first pass: the peaks of earlier calls
            }
            A[0][i] = v;
        }
        __syncthreads();
        int src = 0;
        for (long k = 1, S = H + 1; k < S;) {         // the running maximum over H + 1 blocks by doubling
            const long span = min(2 * k, S);
            const int32_t* __restrict__ m = A[src];
            for (int i = tid; i < kAgHalo + kAgPass; i += kAgThreads) A[1 - src][i] = agc_window_step(m, i, k, span);
            __syncthreads();
            src = 1 - src;
            k = span;
        }
        int32_t w[kAgPer];
        {
            const AgI4* __restrict__ w4 = reinterpret_cast<const AgI4*>(A[src] + kAgHalo + tid * kAgPer);
#pragma unroll
            for (int u = 0; u < kAgPer / 4; u++) {
                const AgI4 q = w4[u];
                w[4 * u] = q.x, w[4 * u + 1] = q.y, w[4 * u + 2] = q.z, w[4 * u + 3] = q.w;
            }
        }
        // the lane's pair, then the pairs of the lanes up to it within the wave
        const Pair own = agc_fold(w, kAgPer, d);
        int32_t v = own.v;
        int n = kAgPer;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int32_t pv = __shfl_up(v, o, 64);
            const int pn = __shfl_up(n, o, 64);
            if (lane >= o) {
                v = agc_max(agc_decayed(pv, n, d), v);
                n += pn;
            }
        }
        if (lane == 63) wv_s[wave] = v, wn_s[wave] = n;
        int32_t ev = __shfl_up(v, 1, 64);
        int en = __shfl_up(n, 1, 64);
        if (lane == 0) ev = kAgcFloor, en = 0;        // nothing before the wave's first lane
        __syncthreads();
        Pair run{L, 0}, before{L, 0};                 // the level before the pass
        for (int q = 0; q < kAgThreads / 64; q++) {
            if (q == wave) before = run;
            run = agc_combine(run, Pair{wv_s[q], wn_s[q]}, d);
        }
        int32_t cur = agc_combine(before, Pair{ev, en}, d).v;
        const long i0 = base + (long)tid * kAgPer;
#pragma unroll
        for (int u = 0; u < kAgPer; u++) {
            const int32_t prev = cur;
            cur = agc_max(agc_decayed(cur, 1, d), w[u]);
            const long idx = i0 + u;
            if (idx < a.nt) {
                const int32_t q = agc_gain_q(T, cur, a.Gmax);
                const float g = ag_gain(q);
                gr[idx] = q;
                br[1 + a.pend + idx] = g;
                if (idx == 0) {                       // what the call's first emitted block ramps from
                    br[0] = a.pend ? hprev_old : g;
                    if (a.pend) br[1] = glast_old;
                }
                if (idx == a.nt - 1) {                // the row's state after the call
                    const float gp = idx > 0 ? ag_gain(agc_gain_q(T, prev, a.Gmax)) : glast_old;
                    level[row] = cur;
                    edge[2 * row] = (idx > 0 || a.pend) ? fminf(gp, g) : g;
                    edge[2 * row + 1] = g;
                }
            }
        }
        L = run.v;
        __syncthreads();                              // the LDS arrays are free for the next pass
    }
    // the last H peaks of the stream, newest at tail[kAgHalo - 1]
    int32_t keep = kAgcFloor;
    if (tid >= kAgHalo - H) {
        const long s = a.nt - (kAgHalo - tid);
        keep = s >= 0 ? pr[s] : tr[tid + a.nt];
    }
    __syncthreads();
    if (tid >= kAgHalo - H) tr[tid] = keep;
}

template <bool CX>
__global__ void __launch_bounds__(kAgThreads)
    k_agcbank_apply(const AgArgs a, const typename AgT<CX>::elem* __restrict__ x,
                    const typename AgT<CX>::elem* __restrict__ hist, const float* __restrict__ gb, long ldg,
                    typename AgT<CX>::elem* __restrict__ y, long ldy)
{
    using E = typename AgT<CX>::elem;
    using Vec = typename AgT<CX>::vec;
    constexpr int V = AgT<CX>::V;
    const int tid = threadIdx.x;
    const int B = a.B, G = a.G, fill = a.fill;
    const int row = blockIdx.y;
    const E* __restrict__ xr = x + (long)row * a.ldx;
    const E* __restrict__ hr = hist + (long)row * 2 * B;
    const float* __restrict__ gr = gb + (long)row * ldg;
    E* __restrict__ yr = y + (long)row * ldy;
    const int l = tid & (G - 1), gi = tid / G, NG = kAgThreads / G;
    const int nvec = B / V, rem = B - nvec * V;
    const float fB = (float)B;
    const long t0 = (long)blockIdx.x * a.T;
    for (int it = 0; it < a.T; it += NG) {
        const long e = t0 + it + gi;
        if (e >= a.ne) continue;
        // boundary gains h = min of the neighbouring blocks' g; gr[0] is the one before the call's first block
        const float g1 = gr[e + 1];
        const float hm = e == 0 ? gr[0] : fminf(gr[e], g1);
        const float dh = fminf(g1, gr[e + 2]) - hm;
        auto gamma = [&](int i) { return hm + dh * (float)(i + 1) / fB; };
        auto scaled = [&](E s, int i) {
            const float gm = gamma(i);
            if constexpr (CX) return make_float2(s.x * gm, s.y * gm);
            else return s * gm;
        };
        const long s0 = e * B;
        E* __restrict__ yb = yr + s0;
        if (s0 >= fill) {
            const E* __restrict__ xb = xr + (s0 - fill);
#pragma unroll 4
            for (int j = l; j < nvec; j += G) {
                AgF4 v = *reinterpret_cast<const Vec*>(xb + V * j);
                if constexpr (CX) {
                    const float ga = gamma(2 * j), gc = gamma(2 * j + 1);
                    v.x *= ga, v.y *= ga, v.z *= gc, v.w *= gc;
                } else {
                    v.x *= gamma(4 * j), v.y *= gamma(4 * j + 1), v.z *= gamma(4 * j + 2), v.w *= gamma(4 * j + 3);
                }
                *reinterpret_cast<Vec*>(yb + V * j) = v;
            }
            if (l < rem) yb[nvec * V + l] = scaled(xb[nvec * V + l], nvec * V + l);
        } else {                                      // a block that starts in the carried samples
            for (int i = l; i < B; i += G) yb[i] = scaled(ag_at(xr, hr, fill, s0 + i), i);
        }
    }
}

template <bool CX>
void launch(const AgcbankCall& c, const AgArgs& a, const AgTrackArgs& t, hipStream_t s)
{
    using E = typename AgT<CX>::elem;
    const unsigned gp = (unsigned)std::max<long>((a.nt + a.T - 1) / a.T, 1);
    {
        LDSP_PROF(s, "k_agcbank_peak");
        hipLaunchKernelGGL(k_agcbank_peak<CX>, dim3(gp, (unsigned)c.C), dim3(kAgThreads), 0, s, a, (const E*)c.x,
                           (const E*)c.hist, (E*)c.hist_out, c.peak_q, (long)c.ldq);
        LDSP_HIP(hipGetLastError());
    }
    if (a.nt == 0) return;
    {
        LDSP_PROF(s, "k_agcbank_track");
        hipLaunchKernelGGL(k_agcbank_track, dim3((unsigned)c.C), dim3(kAgThreads), 0, s, t, c.target, c.level, c.tail,
                           c.edge, (const int32_t*)c.peak_q, c.gain_q, c.gains);
        LDSP_HIP(hipGetLastError());
    }
    if (a.ne == 0) return;
    {
        LDSP_PROF(s, "k_agcbank_apply");
        const unsigned ga = (unsigned)((a.ne + a.T - 1) / a.T);
        hipLaunchKernelGGL(k_agcbank_apply<CX>, dim3(ga, (unsigned)c.C), dim3(kAgThreads), 0, s, a, (const E*)c.x,
                           (const E*)c.hist, (const float*)c.gains, (long)c.ldg, (E*)c.y, (long)c.ldy);
        LDSP_HIP(hipGetLastError());
    }
}

} // namespace

int agcbank_tile(int B, int cplx)
{
    const int NG = kAgThreads / ag_lanes(B, cplx ? 2 : 4);
    return ((kAgTileSamples + B - 1) / B + NG - 1) / NG * NG;
}

void agcbank(const AgcbankCall& c, hipStream_t s)
{
    if (c.n == 0) return;
    LDSP_REQUIRE(c.C >= 1 && c.C <= kAgcbankMaxC, "agcbank: row count out of range");
    LDSP_REQUIRE(c.B >= kAgcbankMinB && c.B <= kAgcbankMaxB, "agcbank: block length out of range");
    LDSP_REQUIRE(c.H >= 0 && c.H <= kAgcMaxHang && c.d >= 0, "agcbank: bad parameters");
    LDSP_REQUIRE(c.n < ((size_t)1 << 36), "agcbank: call too long");
    const size_t B = (size_t)c.B, off = c.pend ? B : 0;
    LDSP_REQUIRE(c.ldx >= c.n && c.fill < 2 * B && c.fill >= off && (c.pend == 0 || c.pend == 1),
                 "agcbank: bad call geometry");
    LDSP_REQUIRE(c.nt == (c.fill + c.n - off) / B && c.ne == (c.pend + c.nt > 0 ? c.pend + c.nt - 1 : 0),
                 "agcbank: block counts do not match the call");
    LDSP_REQUIRE(c.ldq >= c.nt && c.ldg >= c.pend + c.nt + 1 && c.ldy >= c.ne * B,
                 "agcbank: output row stride below the call's blocks");
    const int V = c.cplx ? 2 : 4;
    AgArgs a;
    a.n = (long)c.n;
    a.ldx = (long)c.ldx;
    a.nt = (long)c.nt;
    a.ne = (long)c.ne;
    a.fill = (int)c.fill;
    a.carry = (int)(c.fill + c.n - c.ne * B);
    a.off = (int)off;
    a.B = c.B;
    a.G = ag_lanes(c.B, V);
    a.T = agcbank_tile(c.B, c.cplx);
    LDSP_REQUIRE(a.carry >= 0 && a.carry < 2 * c.B, "agcbank: bad call geometry");
    AgTrackArgs t;
    t.nt = a.nt;
    t.ldq = (long)c.ldq;
    t.ldg = (long)c.ldg;
    t.d = (long)c.d;
    t.H = c.H;
    t.pend = c.pend;
    t.Gmax = c.Gmax;
    if (c.cplx) launch<true>(c, a, t, s);
    else launch<false>(c, a, t, s);
}

} // namespace k
} // namespace ldsp
