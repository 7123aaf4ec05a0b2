// fft_butterflies.hpp -- the register butterflies shared by the FFT kernels
// (k_firfft.hip: overlap-save FIR; k_chan.hip: the channelizer's M-point DFT).
// Complex values are (re, im) float2; every transform is the forward one
// (sign -1) in place with its outputs in natural order.  The inverse of R
// points is the forward transform read at (R - k) mod R.
#pragma once
#include <hip/hip_runtime.h>

namespace ldsp {
namespace k {
namespace {

__device__ __forceinline__ float2 cadd(float2 a, float2 b) { return make_float2(a.x + b.x, a.y + b.y); }
__device__ __forceinline__ float2 csub(float2 a, float2 b) { return make_float2(a.x - b.x, a.y - b.y); }
// a * w (complex), fused
__device__ __forceinline__ float2 cmul(float2 a, float2 w)
{
    return make_float2(fmaf(a.x, w.x, -a.y * w.y), fmaf(a.x, w.y, a.y * w.x));
}
// a * (-i)
__device__ __forceinline__ float2 mul_mi(float2 a) { return make_float2(a.y, -a.x); }

// forward 4-point DFT in place (sign -1)
__device__ __forceinline__ void dft4(float2& a0, float2& a1, float2& a2, float2& a3)
{
    const float2 t0 = cadd(a0, a2), t1 = csub(a0, a2);
    const float2 t2 = cadd(a1, a3), t3 = mul_mi(csub(a1, a3));
    a0 = cadd(t0, t2);
    a2 = csub(t0, t2);
    a1 = cadd(t1, t3);
    a3 = csub(t1, t3);
}

// forward 8-point DFT in place: v[k] = sum_r v[r] exp(-2 pi i r k / 8)
__device__ __forceinline__ void dft8(float2 (&v)[8])
{
    constexpr float r2 = 0.70710678118654752f;
    float2 e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
    float2 o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
    dft4(e0, e1, e2, e3);
    dft4(o0, o1, o2, o3);
    // W8^1 = (1 - i)/sqrt2, W8^2 = -i, W8^3 = (-1 - i)/sqrt2
    const float2 w1 = make_float2((o1.x + o1.y) * r2, (o1.y - o1.x) * r2);
    const float2 w2 = mul_mi(o2);
    const float2 w3 = make_float2((o3.y - o3.x) * r2, -(o3.x + o3.y) * r2);
    v[0] = cadd(e0, o0);
    v[4] = csub(e0, o0);
    v[1] = cadd(e1, w1);
    v[5] = csub(e1, w1);
    v[2] = cadd(e2, w2);
    v[6] = csub(e2, w2);
    v[3] = cadd(e3, w3);
    v[7] = csub(e3, w3);
}

__device__ __forceinline__ float2 cmulk(float2 a, float wr, float wi)
{
    return make_float2(fmaf(a.x, wr, -a.y * wi), fmaf(a.x, wi, a.y * wr));
}

// forward 16-point DFT (4 x 4): out[k + 4 m]
__device__ __forceinline__ void dft16(float2 (&v)[16])
{
    constexpr float c = 0.92387953251128674f, s = 0.38268343236508977f, r2 = 0.70710678118654752f;
#pragma unroll
    for (int j = 0; j < 4; j++) dft4(v[j], v[j + 4], v[j + 8], v[j + 12]);
    // b[j][k] = v[j + 4 k] *= W16^{jk}
    v[5] = cmulk(v[5], c, -s);                                   // j1 k1
    v[9] = make_float2((v[9].x + v[9].y) * r2, (v[9].y - v[9].x) * r2);   // j1 k2: W8
    v[13] = cmulk(v[13], s, -c);                                 // j1 k3
    v[6] = make_float2((v[6].x + v[6].y) * r2, (v[6].y - v[6].x) * r2);   // j2 k1: W8
    v[10] = mul_mi(v[10]);                                       // j2 k2: -i
    v[14] = make_float2((v[14].y - v[14].x) * r2, -(v[14].x + v[14].y) * r2);   // j2 k3: W16^6
    v[7] = cmulk(v[7], s, -c);                                   // j3 k1: W16^3
    v[11] = make_float2((v[11].y - v[11].x) * r2, -(v[11].x + v[11].y) * r2);   // j3 k2: W16^6
    v[15] = cmulk(v[15], -c, s);                                 // j3 k3: W16^9
    // DFT4 over j for each k: inputs v[4k + j]... (b[j][k] sits at v[j + 4k])
#pragma unroll
    for (int k = 0; k < 4; k++) dft4(v[4 * k], v[4 * k + 1], v[4 * k + 2], v[4 * k + 3]);
    // now v[4k + m] = X[k + 4m]; transpose to v[i] = X[i]
    float2 o[16];
#pragma unroll
    for (int k = 0; k < 4; k++)
#pragma unroll
        for (int m = 0; m < 4; m++) o[k + 4 * m] = v[4 * k + m];
#pragma unroll
    for (int i = 0; i < 16; i++) v[i] = o[i];
}

} // namespace
} // namespace k
} // namespace ldsp
