"""Parameter sets of tests/test_gpu_dispatch_edges.py (and of the cases added to
tests/test_gpu_parity.py), with the kernel each is meant to reach.

Kept apart from the tests so that tests/test_dispatch_host.py can check every
choice of shape against the library's dispatch getters on a machine without a
GPU: the thresholds live in the library alone, and a set that stops reaching its
branch fails there, not silently.
"""
import numpy as np
import scipy.signal as sps

# ------------------------------------------------------------------ resampler
# (cplx, len, nfilter, kernel): branch tables of exactly 64 KiB (no room for the
# span beside them: k_resamp_direct) and of 80 KiB (k_resamp, the staged kernel)
RESAMP_SETS = [(False, 16, 512, "direct"), (True, 16, 256, "direct"),
               (False, 10, 1024, "staged"), (True, 10, 512, "staged")]
RESAMP_RATES = [0.024, 0.5, 1.7]       # decimating, near unity, interpolating
RESAMP_FC = 0.2
RESAMP_CUTS = [0, 1, 2, 41, 5000, 5001, 30_011]
# the default tile kernel on inputs off a 16-byte boundary: (cplx, offset in samples)
MISALIGNED = [(True, 1), (False, 1), (False, 2), (False, 3)]
MISALIGNED_RATES = [0.024, 1.7]


def resampler(ld, cplx, rate, m, nf, fc=RESAMP_FC):
    cls = ld.ComplexResampler if cplx else ld.RealResampler
    return cls(rate=np.float32(rate), len=m, Fc=np.float32(fc), As=60.0, nfilter=nf)


# ------------------------------------------------------------------ IIR, exact SOS cascades (k_iir_sect)
# cheby2 lowpass, Fc = 0.02: order -> sections L = ceil(order / 2); tiles of 1024
# samples up to 6 sections, 512 above
SECT_ORDERS = [1, 2, 5, 8, 16, 3, 4, 9, 10, 11, 12, 13, 14]
SECT_FC = 0.02


def sect_sections(order):
    return (order + 1) // 2


def sect_tile(order):
    return 1024 if sect_sections(order) <= 6 else 512


SECT_MANY_ORDERS = [12, 14]            # merged launches at L = 6 (T = 1024) and L = 7 (T = 512)

# ------------------------------------------------------------------ IIR, exact transfer functions (k_iir_seq<Z>)
# scipy butter(N, Wn) as float32 (b, a): nv = N + 1 coefficients -> size class
SEQ_TF = [(3, 0.3, 4), (4, 0.3, 17), (8, 0.4, 17), (12, 0.5, 17), (16, 0.5, 17)]
SEQ_CUTS = [0, 1, 63, 64, 65, 5000, 40_000]


def butter_tf(N, wn):
    b, a = sps.butter(N, wn)
    return np.float32(b), np.float32(a)


# ------------------------------------------------------------------ IIR, fast mode, D > 8 (iir_scan)
# bandpass cheby2 of order 5..8 (D = 2 * order) and wide Butterworths as
# transfer functions (D = N = 9..16; float32 direct form II stays stable: pole
# radius <= 0.91, |y| < 4 on unit Gaussian input)
SCAN_PROTO_ORDERS = [5, 6, 7, 8]
SCAN_PROTO = dict(filter_type="cheby2", band_type="bandpass", Fc=0.05, F0=0.2)
SCAN_TF_ORDERS = list(range(9, 17))
SCAN_TF_WN = 0.5
SCAN_CUTS = [0, 1, 63, 65, 65_535, 65_537, 200_000]
SCAN_AUTO_SIZES = [5000, 200_000]

# ------------------------------------------------------------------ IIR, speculative exact chunks
# (name, W, staged, size class): Butterworth lowpass of order 10 (5 sections) either
# side of the 64 KiB stage, and the one-pole filter of the smallest size class
SPEC_R = 0.985
SPEC_CASES = [("butter10_0.02", 8192, False, 17), ("butter10_0.04", 4096, True, 17), ("onepole", 8192, False, 2)]
SPEC_CUTS = [0, 100, 3000, 3001, 60_000]     # calls shorter than W, and one of > 200 chunks


def spec_filter(ld, name, cplx):
    if name == "onepole":
        b, a = np.float32([1 - SPEC_R]), np.float32([1, -SPEC_R])
        return (ld.CIIRFilter if cplx else ld.RIIRFilter)(b, a)
    fc = float(name.split("_")[1])
    return (ld.ComplexIIRFilter if cplx else ld.RealIIRFilter)(filter_type="butter", order=10, Fc=np.float32(fc))


def spec_oracle(ora, name, cplx):
    if name == "onepole":
        return ora.IIRFilter(tf=(np.float32([1 - SPEC_R]), np.float32([1, -SPEC_R])), cplx=cplx)
    fc = float(name.split("_")[1])
    return ora.IIRFilter(prototype=("butter", "lowpass", 1, 10, np.float32(fc), 0.3, 0.7, 60.0), cplx=cplx)


# ------------------------------------------------------------------ FIR
FIR_TAPS = [1, 2, 15, 16, 17, 51, 127, 255, 513,
            32, 47, 48, 49, 64, 65, 66, 129, 130, 194, 321, 385, 449, 514]
FIR_LONG = 4001                        # direct form with more than 64 KiB of dynamic LDS (complex)


def fir_window(L):
    """(N, P, M): window, overlap and hop an L-tap overlap-save filter would use."""
    P = -(-(L - 1) // 64) * 64
    N = 512 if P <= 128 else 1024
    return N, P, N - P


def fir_expected(L, cplx, mode):
    """The dispatch of a non-empty call: complex fast mode with 48 <= L <= 513 is the FFT."""
    if mode == "fast" and cplx and 48 <= L <= 513:
        N, P, _ = fir_window(L)
        return ("fft", N, P)
    return ("direct", 0, 0)


def fir_hop_cuts(L):
    """Calls that end exactly on a window, one short, one over, and calls shorter
    than the overlap (differences M - 1, M, M + 1, 1, P - 1, ...)."""
    _, P, M = fir_window(L)
    return sorted({0, M - 1, 2 * M - 1, 3 * M, 3 * M + 1, 3 * M + 1 + max(P - 1, 0), 10 * M})
