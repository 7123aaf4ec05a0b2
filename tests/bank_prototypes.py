"""User, asymmetric and short prototypes for the three 4-wave bank demodulators
(k_ambank.hip, k_stbank.hip, k_ssbbank.hip), shared by
tests/test_bank_prototypes_host.py (the cases can fail: reference alone, no device)
and tests/test_gpu_bank_prototypes.py (the kernels against the reference).

The (D, L) list names the path each entry is there for.  Two families of
float32 prototypes, seeded:
  tilted designs (L >= 180): the object's own designed prototype of that length
    times r^j with r^(L-1) = 1 / 64, divided in double by the double sum and
    rounded once: still a low-pass of unit DC gain, clearly asymmetric;
  short prototypes (L <= 60): random, see am_protos / st_protos / ssb_proto.
The float64 references are the Ref classes of test_gpu_ambank.py,
test_gpu_stereobank.py and test_gpu_ssbbank.py, fed the prototypes supplied here
(never the ones read back); StRef adds the sums of the StereoBank's arithmetic
scale.  row_taps is the header's integer-phase formula of the SSBBank's complex
taps (also used by tests/test_ssbbank_host.py)."""
import math
from types import SimpleNamespace

import numpy as np

import test_gpu_ambank as t_am
import test_gpu_ssbbank as t_sb
import test_gpu_stereobank as t_st

# (D, L) and the path of the 4-wave kernels each is there for
CASES = [(8, 1),                # no history, three idle waves
         (8, 2), (8, 3),        # fewer taps than waves, L < D
         (1, 4),                # one tap per wave, D = 1 without the magic division
         (32, 5),               # last wave idle although L > 4, largest D, L << D
         (8, 16), (8, 17),      # (L - 1) / D goes 1 -> 2, ROW parity flips
         (3, 32),               # parts of exactly 8, no remainder
         (5, 60),               # parts of 15, remainder 7
         (4, 180), (5, 224),    # long and even
         (32, 1024),            # even, parts of 256
         (2, 1025)]             # the longest, asymmetric
IDS = [f"{D}-{L}" for D, L in CASES]
# the cases as the host module judges them: each as it is, and LONGEST once more behind a lead that fills its window
VARIANTS = [(D, L, False) for D, L in CASES] + [(2, 1025, True)]
VIDS = IDS + ["2-1025-lead"]
AM_THR = (0.0, t_am.THR)                              # the two thresholds of test_gpu_ambank.py
# the SSBBank's band per tilted design: lo = 2 / (L - 1), the cut-off whose default length is L (or L + 1)
SSB_BAND = {(4, 180): (2 / 179, 0.1), (5, 224): (2 / 223, 0.09), (32, 1024): (1 / 512, 0.015), (2, 1025): (1 / 512, 0.225)}


def nrows(L):
    """3 rows for the short prototypes, 5 from L = 180 on: the generators add their zero, weak and noise rows."""
    return 5 if L >= 180 else 3


def tilted(L):
    return L >= 180


def tilt(p):
    """p[j] r^j with r^(L-1) = 1 / 64, divided in double by the double sum, rounded once."""
    p = np.asarray(p, np.float32).astype(np.float64)
    L = p.size
    t = p * (1.0 / 64.0) ** (np.arange(L, dtype=np.float64) / (L - 1))
    return (t / t.sum()).astype(np.float32)


def unit_l1(v):
    return (v / np.abs(v).sum()).astype(np.float32)


LONGEST = (2, 1025)             # its call of D (2 tile + 1) + 3 samples is shorter than its history


def samples(D, tile, L, lead=False):
    """The modules' own call length, D (2 tile + 1) + 3: two full tiles, a ragged third and a non-zero skip
    afterwards.  At LONGEST that is no longer than the history: no column's window lies inside the stream, and
    the taps j > nD meet zeros alone.  lead: whole tiles in front until the last three tiles' windows do."""
    K = D * (2 * tile + 1) + 3
    return K + D * tile * -(-(L - 1) // (D * tile)) if lead else K


def row_taps(p, lo, hi, words, sides):
    """g_c[j] = p[j] exp(2 pi i psi_c[j] / 2^33) with psi in Python integers, double, rounded once."""
    L = len(p)
    wm = int(np.rint(np.float64((lo + hi) / 2) * 4294967296.0))
    g = np.empty((len(words), L), np.complex64)
    for c, (w, s) in enumerate(zip(words, sides)):
        psi = np.array([(int(s) * wm * (2 * j - (L - 1)) + 2 * j * int(w)) % (1 << 33) for j in range(L)], dtype=np.int64)
        psi = np.where(psi >= 1 << 32, psi - (1 << 33), psi)               # signed: exact in double
        a = np.pi * (psi.astype(np.float64) / 4294967296.0)
        pd = np.asarray(p, np.float32).astype(np.float64)
        g[c] = ((pd * np.cos(a)).astype(np.float32) + 1j * (pd * np.sin(a)).astype(np.float32)).astype(np.complex64)
    return g


def steady(D, L, ncols):
    """Columns whose window holds no sample before the stream's start."""
    return np.arange(ncols) * D >= L - 1


def judged(D, L, ncols):
    """The columns on which a reversed prototype must show: the steady ones, or all where the call has none
    (LONGEST without lead)."""
    st = steady(D, L, ncols)
    return st if st.any() else np.ones(ncols, bool)


# ---------------------------------------------------------------- AMBank
def am_protos(ld, D, L):
    """(h, g): tilted designs at carrier = 4 / (L - 1) and the default audio cut-off, or g = u / sum u with u
    uniform in (0.5, 1) and h = g + e, e normal with sum |e| = 0.25."""
    if tilted(L):
        am = t_am.make(ld, 1, D, L, None, 4 / (L - 1))
        return tilt(am.taps), tilt(am.carrier_taps)
    rng = np.random.default_rng(7100 + 64 * D + L)
    u = rng.uniform(0.5, 1.0, L)
    g = u / u.sum()
    e = rng.standard_normal(L)
    return (g + 0.25 * e / np.abs(e).sum()).astype(np.float32), g.astype(np.float32)


def am_short_rows(seed, C, K, D):
    """complex64 [C][K] (read-only): x = A (1 + a(t)) exp(i (2 pi f0 t + phi)) + noise, A between 0.01 and 1, a(t)
    four tones in (0.02, 0.2) / D at an index of 0.3 to 0.5, |f0| <= 0.002, complex noise of deviation 0.01 A.
    With sum |d| = 0.25 and sum g = 1, |B| <= 0.25 * 1.5 A (1 + noise) < 0.5 A <= |Cr|: every steady column is
    within full scale by construction (am_row's band would need 2 / L of room)."""
    t = np.arange(K, dtype=np.float64)
    x = np.empty((C, K), np.complex128)
    for c in range(C):
        rng = np.random.default_rng(seed + 31 * c)
        A = 10.0 ** rng.uniform(-2.0, 0.0)
        index, f0 = rng.uniform(0.3, 0.5), rng.uniform(-0.002, 0.002)
        f, ph, w = rng.uniform(0.02, 0.2, 4) / D, rng.uniform(0.0, 1.0, 4), rng.uniform(0.3, 1.0, 4)
        w /= w.sum()
        a = index * (w[:, None] * np.sin(2 * np.pi * (f[:, None] * t[None, :] + ph[:, None]))).sum(axis=0)
        x[c] = A * (1.0 + a) * np.exp(2j * np.pi * (f0 * t + rng.uniform(0.0, 1.0)))
        x[c] += 0.01 * A * (rng.standard_normal(K) + 1j * rng.standard_normal(K)) / np.sqrt(2)
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x


_am, _st, _ssb = {}, {}, {}


def am_case(ld, D, L, lead=False):
    """Prototypes, input and the float64 references at the two thresholds, computed once and shared."""
    if (D, L, lead) not in _am:
        C = nrows(L)
        h, g = am_protos(ld, D, L)
        d = (h.astype(np.float64) - g.astype(np.float64)).astype(np.float32)
        K = samples(D, ld.AMBank(1, D, taps=h, carrier_taps=g).tile, L, lead)
        seed = 7200 + 64 * D + L
        if tilted(L):
            x, carried, _ = t_am.rows_for(seed, C, K, t_am.cutoff(D, None), 4 / (L - 1), L)
        else:
            x, carried = am_short_rows(seed, C, K, D), np.ones(C, bool)
        _am[(D, L, lead)] = dict(C=C, D=D, L=L, h=h, g=g, d=d, x=x, carried=carried,
                           make=lambda thr=0.0: ld.AMBank(C, D, taps=h, carrier_taps=g, threshold=thr),
                           ref=[t_am.Ref(g, d, D, x, thr) for thr in AM_THR])
    return _am[(D, L, lead)]


# ---------------------------------------------------------------- StereoBank
class StRef(t_st.Ref):
    """test_gpu_stereobank.Ref from supplied prototypes, with the arithmetic's scale per column:
    Ss = Sz = sum |h[j]| |u|, SP = sum |g[j]| |u|, and from dS = 2 Im(dz conj(P)^2) / m plus the phase error
    2 |dP| / |P| of the unit phasor conj(P)^2 / m,  scale = Ss + 2 Sz + 4 |z| SP / |P|;  Ss where m <= thr^2."""

    def __init__(self, h, g, word, D, x, thr):
        super().__init__(SimpleNamespace(taps=np.asarray(h, np.float32), pilot_taps=np.asarray(g, np.float32),
                                         pilot=word / 2.0 ** 32, word=word, decim=D), x, thr)
        u = np.abs(np.asarray(x).astype(np.float64))
        L, ncols = len(h), self.s.shape[1]
        t = np.arange(ncols, dtype=np.int64)[:, None] * D - np.arange(L, dtype=np.int64)[None, :]
        U = np.concatenate([np.zeros((u.shape[0], L - 1)), u], axis=1)[:, t + L - 1]
        self.Ss = U @ np.abs(np.asarray(h, np.float64))
        self.SP = U @ np.abs(np.asarray(g, np.float64))
        with np.errstate(divide="ignore", invalid="ignore"):
            self.scale = np.where(self.on, 3.0 * self.Ss + 4.0 * np.abs(self.z) * self.SP / np.abs(self.P), self.Ss)


def st_protos(ld, D, L):
    """(h, g): tilted designs, or h and g normal, each scaled to sum |.| = 1."""
    if tilted(L):
        sb = ld.StereoBank(1, t_st.PILOT, D, ntaps=L)
        return tilt(sb.taps), tilt(sb.pilot_taps)
    rng = np.random.default_rng(7300 + 64 * D + L)
    return unit_l1(rng.standard_normal(L)), unit_l1(rng.standard_normal(L))


def st_case(ld, D, L, lead=False):
    if (D, L, lead) not in _st:
        C = nrows(L)
        h, g = st_protos(ld, D, L)
        probe = ld.StereoBank(1, t_st.PILOT, D, taps=h, pilot_taps=g)
        x, pilot = t_st.rows_for(7400 + 64 * D + L, C, samples(D, probe.tile, L, lead))
        _st[(D, L, lead)] = dict(C=C, D=D, L=L, h=h, g=g, x=x, pilot=pilot, word=int(probe.word),
                           make=lambda: ld.StereoBank(C, t_st.PILOT, D, taps=h, pilot_taps=g),
                           ref=StRef(h, g, int(probe.word), D, x, t_st.THR))
    return _st[(D, L, lead)]


# ---------------------------------------------------------------- SSBBank
def ssb_proto(ld, D, L):
    """(p, lo, hi): the tilted design of the band SSB_BAND[(D, L)], or p normal with sum |p| = 1 at
    lo = 0.1 / D, hi = 0.4 / D."""
    if tilted(L):
        lo, hi = SSB_BAND[(D, L)]
        return tilt(ld.SSBBank(1, D, lo=lo, hi=hi, ntaps=L).taps), lo, hi
    rng = np.random.default_rng(7500 + 64 * D + L)
    return unit_l1(rng.standard_normal(L)), 0.1 / D, 0.4 / D


def ssb_case(ld, D, L, lead=False):
    """Prototype, band, BFOs, sidebands, input, g_c from the supplied p (integer-phase formula) and the object's
    words.  The reference is taken from the object's row_taps by the callers, as the existing tests do."""
    if (D, L, lead) not in _ssb:
        C = nrows(L)
        p, lo, hi = ssb_proto(ld, D, L)
        bfo, side = t_sb.lists_for(7600 + 64 * D + L, C)
        make = lambda: ld.SSBBank(C, D, lo=lo, hi=hi, bfo=bfo, sideband=[t_sb.NAMES[int(s)] for s in side], taps=p)  # noqa: E731
        probe = make()
        x, signal = t_sb.rows_for(7700 + 64 * D + L, C, samples(D, probe.tile, L, lead), lo, hi, bfo, side)
        _ssb[(D, L, lead)] = dict(C=C, D=D, L=L, p=p, lo=lo, hi=hi, bfo=bfo, side=side, x=x, signal=signal, make=make,
                            words=probe.words.copy(), g=row_taps(p, lo, hi, probe.words, side))
    return _ssb[(D, L, lead)]


def ncols_after(L, D):
    """The first column whose window has been inside the stream for a column: ceil(L / D) + 1."""
    return math.ceil(L / D) + 1
