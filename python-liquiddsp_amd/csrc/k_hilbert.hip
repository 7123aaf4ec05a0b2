// k_hilbert.hip -- firhilbf (liquid src/filter/src/firhilb.proto.c) for SSBDemod
// (reference src/demod.hpp:155-187) and HilbertTransform (src/utility.hpp:71-108).
// One Hilbert core serves the four operations.  Over z = history ++ this call's
// input, with M the semi-length and hq the 2M quadrature taps,
//   q[n] = sum_j hq[j] s[n - 4M + 1 + 2j]      (float32, acc = 0, then
//                                               acc = acc + hq[j] * s[..], j ascending)
//   C2R    s = im z, d = re z: lower[n] = d[n - 2M] + q[n], upper[n] = d[n - 2M] - q[n]
//   R2C    s = z:              y[n] = (z[n - 2M], q[n])
//   DECIM  y[k] = the R2C output at n = 2k + 1
//   INTERP y[2k] = im z[k - M], y[2k + 1] = sum_j hq[j] re z[k + 1 - 2M + j]
// A sum only ever touches samples of one parity, so a workgroup de-interleaves
// its tile into parity / component planes in LDS on the way in, and every sum
// is a 2M-tap unit-stride FIR over one plane:
//   FO[i] = s at odd  sample 2 (A0 - 2M + i) + 1     -> the even outputs' sums
//   FE[i] = s at even sample 2 (A0 - 2M + 1 + i)     -> the odd outputs' sums
//   DE / DO: the delayed component d at the same indices (C2R; the other ops
//   read the delayed sample from the planes they already have)
// for the tile's first output pair A0; output pair a of the tile is
//   q[2a] = sum_j hq[j] FO[a + j],  d[2a - 2M]     = DE[a + M - 1]
//   q[2a + 1] = sum_j hq[j] FE[a + j],  d[2a + 1 - 2M] = DO[a + M]
// (INTERP is the same at the low rate with FE = re, DE = im).  Each lane keeps
// kHilR = 4 consecutive sums of one plane in registers as a sliding window fed
// by one conflict-free 16-byte LDS read per four taps (2M + 3 plane reads per
// 4 * 2M multiply-adds); the taps are uniform (scalar loads).  The sums go back
// to LDS planes, and the tile is stored in output order with unit-stride stores.
// Workgroup 0 also writes the next call's history (the last H samples of z).
#include "kernels.hpp"
#include "ldsp_common.hpp"

namespace ldsp {
namespace k {

namespace {

constexpr int kHilR = 4;                              // sums per lane and plane
constexpr int kHilPairs = 256 * kHilR;                // output pairs per workgroup
constexpr int kHilPlane = kHilPairs + 2 * kHilbMaxM + 16;  // + the last lane's read-ahead (7); 16 mod 32
static_assert(kHilPlane % 32 == 16 && kHilPlane % 4 == 0, "plane rows: 16-byte aligned, half the banks apart");
static_assert(kHilPairs == kHilbTile / 2, "kernels.hpp states the tile");

template <typename T> __device__ __forceinline__ T hil_zero();
template <> __device__ __forceinline__ float hil_zero<float>() { return 0.0f; }
template <> __device__ __forceinline__ float2 hil_zero<float2>() { return make_float2(0.0f, 0.0f); }

// z[g]: history for g < 0 (H samples), the call's input for g < n, zero beyond
template <typename T>
__device__ __forceinline__ T hil_fetch(const T* __restrict__ x, const T* __restrict__ hist, long g, long n, int H)
{
    if (g < 0) return g + H >= 0 ? hist[g + H] : hil_zero<T>();
    return g < n ? x[g] : hil_zero<T>();
}

typedef float hil_f4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ hil_f4 hil_ld4(const float* p) { return *(const hil_f4*)__builtin_assume_aligned(p, 16); }

// acc[r] = sum_j hq[j] P[r + j], r < 4: the restatement's order within each sum
__device__ __forceinline__ void hil_fir4(const float* P, const float* __restrict__ hq, int M, float acc[kHilR])
{
    // the next four plane samples and taps are fetched one step ahead of their use
    // (hq carries kHilbTapPad readable floats after the taps, the planes 7 after the tile)
    // (native vector loads: one ds_read_b128 each, conflict-free at the lanes' 16-byte stride)
    hil_f4 w0 = hil_ld4(P), w1 = hil_ld4(P + 4);
    float h[4] = {hq[0], hq[1], hq[2], hq[3]};
#pragma unroll
    for (int r = 0; r < kHilR; r++) acc[r] = 0.0f;
    int j = 0;
    for (; j + 4 <= 2 * M; j += 4) {
        const float w[8] = {w0.x, w0.y, w0.z, w0.w, w1.x, w1.y, w1.z, w1.w};
        const float c[4] = {h[0], h[1], h[2], h[3]};
        w0 = w1;
        w1 = hil_ld4(P + j + 8);
#pragma unroll
        for (int t = 0; t < 4; t++) h[t] = hq[j + 4 + t];
#pragma unroll
        for (int t = 0; t < 4; t++) {
#pragma unroll
            for (int r = 0; r < kHilR; r++) acc[r] = acc[r] + c[t] * w[t + r];
        }
    }
    if (j < 2 * M) {                                  // 2M = 4i + 2: the last two taps
        const float w[5] = {w0.x, w0.y, w0.z, w0.w, w1.x};
#pragma unroll
        for (int t = 0; t < 2; t++) {
#pragma unroll
            for (int r = 0; r < kHilR; r++) acc[r] = acc[r] + h[t] * w[t + r];
        }
    }
}

template <int OP> struct HilIo;
template <> struct HilIo<kHilbC2R> { using In = float2; };
template <> struct HilIo<kHilbR2C> { using In = float; };
template <> struct HilIo<kHilbDecim> { using In = float; };
template <> struct HilIo<kHilbInterp> { using In = float2; };

// n: input samples of the call.  y0 / y1: C2R lower / upper (either may be
// null); the other ops write y0.
template <int OP>
__global__ void __launch_bounds__(256) k_hilbert(const typename HilIo<OP>::In* __restrict__ x,
                                                 const typename HilIo<OP>::In* __restrict__ hist,
                                                 typename HilIo<OP>::In* __restrict__ hist_out, long n,
                                                 const float* __restrict__ hq, int M, float* __restrict__ y0,
                                                 float* __restrict__ y1)
{
    using In = typename HilIo<OP>::In;
    constexpr bool kLow = OP == kHilbInterp;          // the sums run at the input rate
    constexpr bool kEven = OP == kHilbC2R || OP == kHilbR2C;   // the even outputs carry a sum too
    constexpr bool kDly = OP == kHilbC2R || OP == kHilbInterp; // the delayed component has planes of its own
    // kHilPlane and the Q rows are 16 mod 32 floats long, so a wave storing
    // alternate-parity outputs reads both rows of a pair without a bank conflict
    constexpr int kNF = kLow ? 1 : 2, kND = OP == kHilbC2R ? 2 : (kDly ? 1 : 0);
    __shared__ __attribute__((aligned(16))) float F[kNF][kHilPlane];
    __shared__ __attribute__((aligned(16))) float D[kND ? kND : 1][kND ? kHilPlane : 4];
    __shared__ __attribute__((aligned(16))) float Q[2][kHilPairs + 16];
    float* const FE = F[0];
    float* const FO = F[kNF - 1];
    float* const DE = D[0];
    float* const DO = D[kND == 2 ? 1 : 0];
    float* const QE = Q[0];
    float* const QO = Q[1];
    const int tid = threadIdx.x;
    const int H = kLow ? 2 * M - 1 : 4 * M - 1;
    const long A0 = (long)blockIdx.x * kHilPairs;     // first output pair of the tile
    const long pairs = kLow ? n : (OP == kHilbDecim ? n / 2 : (n + 1) / 2);
    const int cntp = (int)min((long)kHilPairs, pairs - A0);

    if (blockIdx.x == 0) {                            // the next call's history
        for (int j = tid; j < H; j += 256) {
            const long g = n - H + j;
            hist_out[j] = g < 0 ? hist[g + H] : x[g];
        }
    }
    // Sample g0 + u goes to the planes, u in [u0, lim):
    //   low rate: plane index u <-> sample A0 - 2M + 1 + u
    //   else:     u <-> sample 2 (A0 - 2M) + u; the first even sample lies before FE[0]
    constexpr int u0 = kLow ? 0 : 1;
    const int lim = kLow ? cntp + 2 * M - 1 : 2 * (cntp + 2 * M);
    const long g0 = kLow ? A0 - 2 * M + 1 : 2 * (A0 - 2 * M);
    auto put = [&](int u, In v) {
        if constexpr (kLow) {
            FE[u] = v.x;
            DE[u] = v.y;
        } else {
            const int p = u >> 1;
            if constexpr (OP == kHilbC2R) {
                if (u & 1) FO[p] = v.y, DO[p] = v.x;
                else FE[p - 1] = v.y, DE[p - 1] = v.x;
            } else {
                if (u & 1) FO[p] = v;
                else FE[p - 1] = v;
            }
        }
    };
    if (g0 + u0 >= 0 && g0 + lim <= n) {
        // an inner tile reads the input alone: all its loads are issued before the first plane store
        constexpr int kLd = ((kLow ? 1 : 2) * (kHilPairs + 2 * kHilbMaxM) + 255) / 256;
        const In* __restrict__ xb = x + g0;
        In v[kLd];
#pragma unroll
        for (int i = 0; i < kLd; i++) {
            const int u = u0 + tid + 256 * i;
            v[i] = hil_zero<In>();
            if (u < lim) v[i] = xb[u];
        }
#pragma unroll
        for (int i = 0; i < kLd; i++) {
            const int u = u0 + tid + 256 * i;
            if (u < lim) put(u, v[i]);
        }
    } else {
        for (int u = u0 + tid; u < lim; u += 256) put(u, hil_fetch<In>(x, hist, g0 + u, n, H));
    }
    __syncthreads();
    if (kHilR * tid < cntp) {
        float acc[kHilR];
        if constexpr (kEven) {
            hil_fir4(FO + kHilR * tid, hq, M, acc);
            *(float4*)(QE + kHilR * tid) = make_float4(acc[0], acc[1], acc[2], acc[3]);
        }
        hil_fir4(FE + kHilR * tid, hq, M, acc);
        *(float4*)(QO + kHilR * tid) = make_float4(acc[0], acc[1], acc[2], acc[3]);
    }
    __syncthreads();
    if constexpr (OP == kHilbDecim) {
        float2* y = (float2*)y0;
        for (int a = tid; a < cntp; a += 256) y[A0 + a] = make_float2(FO[a + M], QO[a]);
    } else {
        const long nout = kLow ? 2 * n : n;           // outputs of the call
        const int cnt = (int)min((long)(2 * kHilPairs), nout - 2 * A0);
        for (int u = tid; u < cnt; u += 256) {
            const int a = u >> 1;
            const long o = 2 * A0 + u;
            if constexpr (OP == kHilbC2R) {
                const float d = (u & 1) ? DO[a + M] : DE[a + M - 1];
                const float q = (u & 1) ? QO[a] : QE[a];
                if (y0) y0[o] = d + q;
                if (y1) y1[o] = d - q;
            } else if constexpr (OP == kHilbR2C) {
                const float d = (u & 1) ? FO[a + M] : FE[a + M - 1];
                const float q = (u & 1) ? QO[a] : QE[a];
                ((float2*)y0)[o] = make_float2(d, q);
            } else {
                y0[o] = (u & 1) ? QO[a] : DE[a + M - 1];
            }
        }
    }
}

template <int OP>
void hil_launch(const void* x, const void* hist, void* hist_out, size_t n, const float* hq, int M, void* y0, void* y1,
                hipStream_t s)
{
    using In = typename HilIo<OP>::In;
    const size_t pairs = OP == kHilbInterp ? n : (n + 1) / 2;
    const unsigned grid = (unsigned)((pairs + kHilPairs - 1) / kHilPairs);
    hipLaunchKernelGGL(k_hilbert<OP>, dim3(grid), dim3(256), 0, s, (const In*)x, (const In*)hist, (In*)hist_out,
                       (long)n, hq, M, (float*)y0, (float*)y1);
}

} // namespace

void hilbert(int op, const void* x, const void* hist, void* hist_out, size_t n, const float* hq, int M, void* y0,
             void* y1, hipStream_t s)
{
    if (n == 0) return;
    LDSP_REQUIRE(M >= 2 && M <= kHilbMaxM, "hilbert: semi-length out of range");
    LDSP_REQUIRE(n < ((size_t)1 << 41), "hilbert: call too long");
    switch (op) {
    case kHilbR2C: {
        LDSP_PROF(s, "k_hilbert_r2c");
        hil_launch<kHilbR2C>(x, hist, hist_out, n, hq, M, y0, y1, s);
        break;
    }
    case kHilbC2R: {
        LDSP_PROF(s, "k_hilbert_c2r");
        hil_launch<kHilbC2R>(x, hist, hist_out, n, hq, M, y0, y1, s);
        break;
    }
    case kHilbDecim: {
        LDSP_PROF(s, "k_hilbert_decim");
        hil_launch<kHilbDecim>(x, hist, hist_out, n, hq, M, y0, y1, s);
        break;
    }
    case kHilbInterp: {
        LDSP_PROF(s, "k_hilbert_interp");
        hil_launch<kHilbInterp>(x, hist, hist_out, n, hq, M, y0, y1, s);
        break;
    }
    default:
        throw Error(LDSP_EINVAL, "hilbert: unknown operation");
    }
    LDSP_HIP(hipGetLastError());
}

} // namespace k
} // namespace ldsp
