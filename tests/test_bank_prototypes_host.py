"""The cases of tests/bank_prototypes.py can fail (CPU suite, no device): on the
float64 references alone,

  * reversal is visible: the reference computed from the reversed prototypes
    differs from the reference by at least 1e-4 of the row's maximum, 100 times the
    GPU gate, over the steady columns of every signal row (all columns where the
    call is shorter than the history, (2, 1025); that case is judged once more
    behind a lead that fills its window), so a table written
    with j where k = L - 1 - j belongs fails parity by two orders of magnitude
    (a condition on the cases, not a tolerance);
  * AMBank: no column lies on the threshold, every steady column of a carrier
    row is within full scale;
  * StereoBank: at most 1 % of a case's columns lie on the threshold; with the
    tilted designs the pilot rows are open in every column from ceil(L / D) on
    and the zero and noise rows in none, with the short prototypes at least one
    row has both open and closed columns;
  * SSBBank with an even L recovers m(nD - (L - 1) / 2), the half-sample delay,
    within the 2e-3 of test_recovery_and_rejection, and misses (L - 1) // 2 by
    orders of magnitude;
  * the supplied prototypes read back with their bits, band_taps as
    float(double(h) - double(g)), and the SSBBank's row_taps lie within one
    float32 step of the integer-phase formula.

Each test prints the figures it asserts on."""
import math

import numpy as np
import pytest

import bank_prototypes as bp
import test_gpu_ambank as t_am
import test_gpu_ssbbank as t_sb
import test_gpu_stereobank as t_st
from bank_prototypes import VARIANTS, VIDS
from test_ssbbank_host import ulps

VISIBLE = 100 * 1e-6                                  # 100 times the gate, of the row's maximum


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def moved(ref, rev, keep):
    """Per row: the largest difference over the columns kept, relative to the row's largest reference there."""
    top = np.max(np.where(keep, np.abs(ref), 0.0), axis=1)
    return np.max(np.where(keep, np.abs(ref - rev), 0.0), axis=1) / np.where(top > 0, top, 1.0)


# ---------------------------------------------------------------- AMBank
@pytest.mark.parametrize("D,L,lead", VARIANTS, ids=VIDS)
def test_ambank_case(ld, D, L, lead):
    cs = bp.am_case(ld, D, L, lead)
    am = cs["make"]()
    assert (am.ntaps, am.decim, am.nchan) == (L, D, cs["C"])
    assert (bits(am.taps) == bits(cs["h"])).all() and (bits(am.carrier_taps) == bits(cs["g"])).all()
    assert (bits(am.band_taps) == bits(cs["d"])).all()
    assert cs["x"].shape == (cs["C"], bp.samples(D, am.tile, L, lead))
    if L > 1:
        assert not np.array_equal(cs["g"], cs["g"][::-1]) and not np.array_equal(cs["d"], cs["d"][::-1])
    for thr, ref in zip(bp.AM_THR, cs["ref"]):
        assert not ref.edge.any(), int(ref.edge.sum())
        st = ref.steady[0]
        full = ~ref.beyond[cs["carried"]][:, st]
        assert ref.on[cs["carried"]][:, st].all()
        assert st.any() or (D, L) == bp.LONGEST and not lead
        line = f"AMBank D={D} L={L} thr={thr:g}: {int(full.sum())} of {full.size} steady columns of the carrier rows within full scale"
        if L > 1:
            rev = t_am.Ref(cs["g"][::-1], cs["d"][::-1], D, cs["x"], thr)
            mv = moved(ref.y, rev.y, bp.judged(D, L, ref.y.shape[1])[None, :])[cs["carried"]]
            line += f", reversed differs by {mv.min():.3g} .. {mv.max():.3g} of the row maximum"
            assert mv.min() >= VISIBLE, mv
        print(line)
        assert full.all()


# ---------------------------------------------------------------- StereoBank
@pytest.mark.parametrize("D,L,lead", VARIANTS, ids=VIDS)
def test_stereobank_case(ld, D, L, lead):
    cs = bp.st_case(ld, D, L, lead)
    sb, ref, pilot = cs["make"](), cs["ref"], cs["pilot"]
    assert (sb.decim, sb.nchan, sb.word) == (D, cs["C"], cs["word"]) and len(sb.taps) == L
    assert (bits(sb.taps) == bits(cs["h"])).all() and (bits(sb.pilot_taps) == bits(cs["g"])).all()
    assert cs["x"].shape == (cs["C"], bp.samples(D, sb.tile, L, lead))
    assert ref.edge.sum() <= 0.01 * ref.edge.size, int(ref.edge.sum())
    share = ref.on.mean(axis=1)
    line = f"StereoBank D={D} L={L}: {int(ref.edge.sum())} columns on the threshold, open share per row " + \
        " ".join(f"{100 * v:.0f}%" for v in share)
    if bp.tilted(L):
        n0 = math.ceil(L / D)
        assert ref.on[pilot][:, n0:].all() and not ref.on[~pilot].any()
    else:
        assert ((share > 0) & (share < 1)).any(), share
    if L > 1:
        assert not np.array_equal(cs["h"], cs["h"][::-1]) and not np.array_equal(cs["g"], cs["g"][::-1])
        rev = bp.StRef(cs["h"][::-1], cs["g"][::-1], cs["word"], D, cs["x"], t_st.THR)
        keep = bp.judged(D, L, ref.s.shape[1])[None, :]
        mv = np.minimum(moved(ref.left, rev.left, keep), moved(ref.right, rev.right, keep))[pilot]
        line += f", reversed differs by {mv.min():.3g} .. {mv.max():.3g} of the pilot rows' maximum"
        assert mv.min() >= VISIBLE, mv
    print(line)


# ---------------------------------------------------------------- SSBBank
@pytest.mark.parametrize("D,L,lead", VARIANTS, ids=VIDS)
def test_ssbbank_case(ld, D, L, lead):
    cs = bp.ssb_case(ld, D, L, lead)
    sb = cs["make"]()
    assert (sb.ntaps, sb.decim, sb.nchan, sb.lo, sb.hi) == (L, D, cs["C"], cs["lo"], cs["hi"])
    assert (bits(sb.taps) == bits(cs["p"])).all() and (sb.words == cs["words"]).all()
    assert cs["x"].shape == (cs["C"], bp.samples(D, sb.tile, L, lead))
    off = ulps(sb.row_taps, cs["g"])
    assert off.max() <= 1, int(off.max())
    line = f"SSBBank D={D} L={L}: row_taps worst {int(off.max())} float32 step of the integer-phase formula"
    if L > 1:
        assert not np.array_equal(cs["p"], cs["p"][::-1])
        side = cs["side"]
        ref = t_sb.Ref(cs["g"], cs["words"], D, cs["x"])
        rev = t_sb.Ref(bp.row_taps(cs["p"][::-1], cs["lo"], cs["hi"], cs["words"], side), cs["words"], D, cs["x"])
        keep = bp.judged(D, L, ref.y.shape[1])[None, :]
        mv = moved(ref.y, rev.y, keep)[cs["signal"]]
        line += f", reversed differs by {mv.min():.3g} .. {mv.max():.3g} of the signal rows' maximum"
        assert mv.min() >= VISIBLE, mv
    print(line)


@pytest.mark.parametrize("D,L,lo,hi", [(2, 80, 0.025, 0.225), (4, 200, 0.01, 0.1), (1, 34, 0.0625, 0.4)])
def test_ssbbank_even_length_delays_by_half_a_sample(ld, D, L, lo, hi):
    """The symmetric designed prototype of an even length: on clean unit-sum tones, after ceil(L / D) + 1
    columns, the float64 definition is m(nD - (L - 1) / 2) within 2e-3 (the bound of
    test_recovery_and_rejection); a tap phase counted in whole samples, (L - 1) // 2, would miss by 0.1 and more."""
    C = 3
    bfo, side = np.array([0.0, 0.123456789, -0.3141592653589793]), np.array([1, -1, 1])
    sb = t_sb.make(ld, (C, D, L, lo, hi), bfo, side)
    assert sb.ntaps == L and np.array_equal(sb.taps, sb.taps[::-1])
    n0 = bp.ncols_after(L, D)
    K = D * (n0 + 2 * sb.tile + 1) + 3
    bfo_w = sb.words.astype(np.int64).astype(np.int32).astype(np.float64) / 4294967296.0
    rows, mods = [], []
    for c in range(C):
        f, ph, w, m = t_sb.tones(np.random.default_rng(3000 + 31 * c), 2 * lo, hi - lo)
        rows.append(t_sb.ssb_row(K, bfo_w[c], side[c], 1.0, f, ph, w))
        mods.append(m)
    ref = t_sb.Ref(sb.row_taps, sb.words, D, np.stack(rows).astype(np.complex64))
    n = np.arange(ref.y.shape[1], dtype=np.float64) * D
    for c, m in enumerate(mods):
        half = np.max(np.abs(ref.y[c, n0:] - m(n - (L - 1) / 2)[n0:]))
        whole = np.max(np.abs(ref.y[c, n0:] - m(n - (L - 1) // 2)[n0:]))
        print(f"D={D} L={L} bfo {bfo[c]:+.3f} {t_sb.NAMES[side[c]]}: {half:.3g} at (L - 1) / 2, {whole:.3g} at (L - 1) // 2")
        assert half <= 2e-3, (c, float(half))
        assert whole >= 10 * 2e-3, (c, float(whole))
