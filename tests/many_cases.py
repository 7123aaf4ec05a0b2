"""Parameter sets of tests/test_gpu_many_mixed.py (many-calls on channels that
differ), with the path each is meant to reach.

Kept apart from the tests, like dispatch_cases.py, so that
tests/test_many_host.py can check every set against the library's own decision
code (AGC._dispatch, AmpModem._dispatch, the IIR getters) on a machine without a
GPU: a set that stops reaching its branch fails there.
"""
import numpy as np

SIZES = (0, 200, 1100, 3000, 40_000, 70_001, 262_144, 300_007)     # every n of the mixed tests

# ------------------------------------------------------------------ AGC
# bandwidth -> (exact warm-up W, approximate warm-up Wa, first chunk-parallel n);
# a call is speculative once the object's history holds W + Wa + 256 samples
AGC_WARMUPS = {0.1: (256, 1024, 2048), 0.01: (500, 4000, 3575), 1e-3: (5000, 40_000, 30_950)}
AGC_SMALL_MIN = 320                      # below: the sequential loop
# (a) five channels; channel 1 locked at gain 2, channel 2 at scale 1 (the others
# 0.01), channel 4 with a 777-sample call of its own first
AGC_BW = [0.1, 0.01, 0.01, 1e-3, 0.01]
AGC_LOCKED, AGC_SCALE1, AGC_PRE, AGC_PRE_N = 1, 2, 4, 777
AGC_CALLS = [3000, 200, 40_000, 40_000]
# the path of every channel on every call, and which calls run from the history
# alone: the history holds min(hist_len, samples seen) = 0 / 3000 / 3200 / 43 200
# (+ 777 on channel 4) against 1536, 4756, 4756, 45 256, 4756
AGC_PATHS = [["par", "small", "small", "small", "small"],
             ["seq"] * 5,
             ["par"] * 5,
             ["par"] * 5]
AGC_SPEC = [[False] * 5,
            None,                                      # sequential calls: not applicable
            [True, False, False, False, False],
            [True, True, True, False, True]]
# afterwards: another bandwidth on channel 2 (its history restarts), reset() on
# channel 4 (its history stays), then two more calls
AGC_SETTER_CH, AGC_SETTER_BW, AGC_RESET_CH = 2, 0.03, 4
AGC_CALLS_AFTER = [40_000, 3000]
AGC_PATHS_AFTER = [["par"] * 5, ["par", "small", "par", "small", "small"]]
AGC_SPEC_AFTER = [[True, True, False, True, True], [True, None, True, None, None]]

# ------------------------------------------------------------------ AmpModem
# (b) dsb modems alternating carrier PLL and Costas loop
AMP_CARRIER = [True, False, True, False, True, False]
AMP_MOD = [0.5, 0.75, 0.3, 0.5, 0.75, 0.3]
AMP_CALLS = [1100, 3000, 40_000, 200]
# n -> (carrier path, Costas path): 1100 lies between the two thresholds
AMP_PATHS = {200: ("seq", "seq"), 1100: ("par", "seq"), 3000: ("par", "par"), 40_000: ("par", "par")}

# ------------------------------------------------------------------ IIR, fast mode (modal scan)
# complex cheby2 lowpass: (order, Fc, modes M, look-back J)
MODAL_FILTERS = [(8, 0.02, 4, 3), (8, 0.0075, 4, 7), (8, 0.004, 4, 13), (8, 0.002, 4, 28),
                 (4, 0.0075, 2, 7), (6, 0.0075, 3, 6)]
MODAL_M4 = [0, 1, 2, 3]                  # indices of the four-mode filters
MODAL_CALLS = [40_000, 262_144, 300_007]
# n -> (units, workgroups by look-back J): one-XCD mode (8 x units) while units <= 16 J
MODAL_GRIDS = {40_000: (20, {3: 160, 7: 160, 13: 160, 28: 160, 6: 160}),
               262_144: (128, {3: 128, 7: 128, 13: 1024, 28: 1024, 6: 128}),
               300_007: (147, {3: 147, 7: 147, 13: 1176, 28: 1176, 6: 147})}
# k_iir_modal launches of one execute_many over the six filters.  Equal grids
# merge within a mode count when the grid is a multiple of 8; sizeof(IirModalArgs)
# is 432, so a merged launch carries at most 8 objects (more than any group here).
#   40 000: M = 4 x 4 -> 1, M = 2 -> 1, M = 3 -> 1
#  262 144: M = 4: {J 3, 7} at 128 -> 1, {J 13, 28} at 1024 -> 1; M = 2 (J 7, 128) -> 1; M = 3 (J 6, 128) -> 1
#  300 007: M = 4: J 3 and J 7 at 147 alone -> 2, {J 13, 28} at 1176 -> 1; M = 2 -> 1; M = 3 -> 1
MODAL_LAUNCHES = {40_000: 3, 262_144: 4, 300_007: 5}

# exact SOS cascades (k_iir_sect: block size 2 x sections x 64, so the many-call
# splits by section count): cheby2 lowpass at Fc 0.02
SECT_ORDERS = [8, 8, 12, 14, 5]
SECT_FC = 0.02
SECT_LAUNCHES = 4                        # orders 8 + 8 merge; 12, 14 and 5 run alone

# speculative exact chunks: butter order 4 and ellip order 6 at Fc 0.05 (exact mode)
SPEC_PROTOS = [("butter", 4), ("ellip", 6)]
SPEC_FC = 0.05
ONEPOLE_R = [0.985, 0.9]                 # RIIRFilter one-poles beside the two de-emphasis filters
DEEMPH_RATES = [48000.0, 44100.0]
SPEC_CALLS = [3000, 70_001]

# ------------------------------------------------------------------ filter_resample_many
# (d) (Fc of the cheby2 order 8 filter, resampler rate); the last channel has
# made a 777-sample filter_resample of its own first
FRONT = [(0.0075, 0.024), (0.004, 0.1), (0.02, 0.5), (0.0075, 0.024)]
FRONT_PRE_CH, FRONT_PRE_N = 3, 777
FRONT_CALLS = [70_001, 2048 + 39, 262_144, 0]

# ------------------------------------------------------------------ cap splits
CAP_C = [1, 2, 9, 17]
CAP_N = 40_000


def ceil_div(a, b):
    return -(-a // b)


def modal_filter(ld, order, fc, cplx=True):
    cls = ld.ComplexIIRFilter if cplx else ld.RealIIRFilter
    return cls(filter_type="cheby2", order=order, Fc=np.float32(fc))


def modal_oracle(ora, order, fc, cplx=True):
    return ora.IIRFilter(prototype=("cheby2", "lowpass", 1, order, np.float32(fc), 0.3, 0.7, 60.0), cplx=cplx)


def resampler(ld, rate, cplx=True):
    cls = ld.ComplexResampler if cplx else ld.RealResampler
    return cls(rate=np.float32(rate), Fc=np.float32(min(rate, 0.4)))


def resampler_oracle(ora, rate, cplx=True):
    return ora.Resampler(np.float32(rate), m=20, fc=np.float32(min(rate, 0.4)), npfb=13, cplx=cplx)


def agc(ld, c):
    g = ld.AGC()
    g.bandwidth = AGC_BW[c]
    g.scale = 1.0 if c == AGC_SCALE1 else 0.01
    if c == AGC_LOCKED:
        g.gain = 2.0
        g.lock = True
    return g


def agc_oracle(ora, c):
    g = ora.AGC()
    g.bandwidth = np.float32(AGC_BW[c])
    g.scale = np.float32(1.0 if c == AGC_SCALE1 else 0.01)
    if c == AGC_LOCKED:
        g.gain = np.float32(2.0)
        g.lock(True)
    return g
