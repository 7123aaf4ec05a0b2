// chan_dft.hpp -- what the two filter-bank kernels share (k_chan.hip: analysis,
// k_synth.hip: synthesis): the split M = R1 R2 of the M-point inverse DFT and
// the inverse register transform.  The twiddle table exp(2 pi i j / M), j < M,
// is the host's (capi.cpp: bank_twiddles), computed in double and rounded once.
#pragma once
#include "fft_butterflies.hpp"

namespace ldsp {
namespace k {
namespace {

constexpr int chan_r2(int M) { return M <= 16 ? 1 : (M <= 64 ? 8 : 16); }

// inverse R-point DFT in place, natural order: the forward one read at (R - k) mod R
template <int R>
__device__ __forceinline__ void chan_idft(float2 (&v)[R])
{
    static_assert(R == 4 || R == 8 || R == 16, "register transforms: 4, 8, 16 points");
    if constexpr (R == 4) dft4(v[0], v[1], v[2], v[3]);
    else if constexpr (R == 8) dft8(v);
    else dft16(v);
#pragma unroll
    for (int k = 1; k < R / 2; k++) {
        const float2 t = v[k];
        v[k] = v[R - k];
        v[R - k] = t;
    }
}

} // namespace
} // namespace k
} // namespace ldsp
