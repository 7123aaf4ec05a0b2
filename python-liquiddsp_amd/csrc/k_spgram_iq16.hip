// k_spgram_iq16.hip -- k_spgram's kernels for int16 (I, Q) input (k::spgram_iq16),
// built from k_spgram.hip in a translation unit of their own: see there.
#define LDSP_SPGRAM_IQ16 1
#include "k_spgram.hip"
