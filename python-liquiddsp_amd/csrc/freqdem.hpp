// freqdem.hpp -- the FM discriminator of one sample pair, shared by k_freqdem
// (k_misc.hip) and the FMBank kernels (k_fmbank.hip) so that both give the same
// bits: freqdem_demodulate_block's
//   y = cargf(conjf(r') r) * ref,   ref = (float)(1 / (2 pi kf)),
// r' the sample before r.  The library is built with -ffp-contract=off, so the
// products and sums below round one by one wherever the function is inlined.
#pragma once
#include "ldsp_math.hpp"

namespace ldsp {

__device__ __forceinline__ float freqdem_disc(const float2 rp, const float2 r, const float ref)
{
    // conjf(r') * r with the C99 float complex product: (a + j b')(c + j d), b' = -b
    const float a = rp.x, bq = -rp.y;
    const float re = a * r.x - bq * r.y;
    const float im = a * r.y + bq * r.x;
    return lm_atan2f(im, re) * ref;
}

} // namespace ldsp
