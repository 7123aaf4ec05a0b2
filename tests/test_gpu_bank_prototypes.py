"""AMBank, StereoBank and SSBBank on the GPU with user, asymmetric and short
prototypes (tests/bank_prototypes.py): the convention h[j] x[nD - j] of the
tables indexed by k = L - 1 - j, idle waves (L < 4), no history (L = 1), a
history shorter than a skip (L - 1 < D), parts without a remainder and with the
longest one, both parities of ROW and even L, none of which the designed
symmetric odd prototypes of the objects' own modules can see.  That the cases
can fail -- a reversed table differs by 100 gates and more -- is asserted on
the references alone in tests/test_bank_prototypes_host.py.

(a) Parity with the float64 definition from the supplied prototypes.  Tilted
designs keep each object's documented gate: AMBank 1e-6 absolute within full
scale and 1e-6 of ref.scale beyond it, StereoBank 1e-6 of the row maximum outside
ref.edge, SSBBank gate_rows.  Short prototypes are not selective, so |P| or the
output can be small against the sums that form it; they are held to 1e-6 of the
arithmetic's own scale per column: AMBank ref.scale, SSBBank ref.scale for every
row, StereoBank Ss + 2 Sz + 4 |z| SP / |P| (StRef), Ss where the column is mono.
For L <= 60 the worst-case rounding of 32 partial sums and the trees lies below
1e-6 of that scale: a miss is a finding.
(b) Ten ragged calls give the bits of one call.
The longest case, (2, 1025), runs once more behind a lead that fills its
window (test_longest_prototype_behind_a_lead).
(c) An object created from the designed object's read-back prototypes returns
the designed object's bits.
Two identities independent of the references: a unit-sample prototype makes
the StereoBank (no pilot taps) and the SSBBank (BFO 0) return the input sample
nD - j0, for the SSBBank through its one complex tap, bit for bit.

Measured on an MI355X (profiles/bank_prototypes_gpu.txt), worst figure per case
against the gate of 1e-6; short prototypes against the arithmetic's scale,
tilted designs (from L = 180) against each object's own gate: AMBank absolute
within full scale at thr = 0, StereoBank the worse of left and right against the
row maximum, SSBBank the signal rows against the row maximum:

    (D, L)       AMBank     StereoBank   SSBBank
    (8, 1)       1.4e-16    3.7e-16      1.1e-7
    (8, 2)       5.7e-8     7.5e-8       1.5e-7
    (8, 3)       1.6e-8     7.8e-8       7.7e-8
    (1, 4)       3.9e-8     7.7e-8       6.6e-8
    (32, 5)      2.5e-8     8.9e-8       7.0e-8
    (8, 16)      5.2e-8     5.4e-8       4.5e-8
    (8, 17)      1.6e-8     6.9e-8       4.9e-8
    (3, 32)      3.0e-8     5.0e-8       1.2e-7
    (5, 60)      1.3e-8     8.6e-8       5.9e-8
    (4, 180)     3.5e-7     1.6e-7       7.5e-8
    (5, 224)     4.0e-7     1.5e-7       1.2e-7
    (32, 1024)   5.7e-7     1.8e-7       1.1e-7
    (2, 1025)    7.9e-7     4.5e-7       6.1e-8
    behind lead  6.8e-7     1.4e-7       1.3e-7

Beyond full scale the tilted AMBank cases reach |y| = 2.6e6 at thr = 0; over all
columns the error against ref.scale is the figure above, so the columns beyond
full scale are no worse; the carrier level is within 9.5e-8 and
the pilot level within 1.6e-7 of the definition's.  No column lay on a
threshold.  With one tap the float32 sums are exact, hence the 1e-16.
"""
from types import SimpleNamespace

import numpy as np
import pytest

import bank_prototypes as bp
import test_gpu_ambank as t_am
import test_gpu_ssbbank as t_sb
import test_gpu_stereobank as t_st
from bank_prototypes import CASES, IDS
from test_ssbbank_host import ulps

pytestmark = pytest.mark.gpu

GATE = 1e-6


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


_runs = {}


def run(kind, ld, D, L):
    """One call per object and case, computed once and shared by the parity and the cut tests."""
    key = (kind, D, L)
    if key not in _runs:
        if kind == "am":
            cs = bp.am_case(ld, D, L)
            objs = [cs["make"](thr) for thr in bp.AM_THR]
            _runs[key] = dict(cs, y=[o(cs["x"]) for o in objs], level=[o.carrier_level.copy() for o in objs],
                              skip=objs[0].skip)
        elif kind == "st":
            cs = bp.st_case(ld, D, L)
            sb = cs["make"]()
            _runs[key] = dict(cs, y=sb(cs["x"]), level=sb.pilot_level.copy(), skip=sb.skip)
        else:
            cs = bp.ssb_case(ld, D, L)
            sb = cs["make"]()
            assert ulps(sb.row_taps, cs["g"]).max() <= 1
            _runs[key] = dict(cs, y=sb(cs["x"]), skip=sb.skip, ref=t_sb.Ref(sb.row_taps, sb.words, D, cs["x"]))
    return _runs[key]


def ragged(make, x, D, axis):
    """The object fed x in the modules' ten ragged calls; skip and every call's shape as the schedule says."""
    cut = make()
    lens = t_am.ragged_cuts(np.random.default_rng(40 + D), x.shape[1], D)
    assert len(lens) == 10
    parts, at = [], 0
    for n in lens:
        skip = cut.skip
        assert skip == (-at) % D
        p = cut(x[:, at:at + n])
        assert p.shape[axis] == ((-(-(n - skip) // D)) if n > skip else 0) and p.shape[0] == x.shape[0]
        parts.append(p)
        at += n
    assert any(0 < n < D and p.shape[axis] == 0 for n, p in zip(lens, parts)) or D <= 2
    return cut, np.concatenate(parts, axis=axis)


# ---------------------------------------------------------------- AMBank
@pytest.mark.parametrize("D,L", CASES, ids=IDS)
def test_ambank_parity_with_definition(ld, D, L):
    r = run("am", ld, D, L)
    C, K = r["C"], r["x"].shape[1]
    assert r["skip"] == (-K) % D
    for thr, y, ref, level in zip(bp.AM_THR, r["y"], r["ref"], r["level"]):
        assert y.dtype == np.float32 and y.shape == (C, -(-K // D)) == ref.y.shape
        assert np.isfinite(y).all()
        assert not ref.edge.any()
        err = np.abs(y.astype(np.float64) - ref.y)
        full = ~ref.beyond
        assert full[r["carried"]][:, ref.steady[0]].all()
        over = err / ref.scale
        print(f"AMBank D={D} L={L} thr={thr:g}: worst absolute {err[full].max():.3g} within full scale, "
              f"{over.max():.3g} of the arithmetic's scale over all columns (|y| up to {np.abs(ref.y).max():.3g})")
        assert over.max() <= GATE, (thr, float(over.max()))                # ref.scale is 1 within full scale
        if bp.tilted(L):
            assert err[full].max() <= GATE, (thr, float(err[full].max()))
            assert (bits(y[1]) == 0).all()                                 # the zero row: +0.0
        Cl = np.abs(ref.Cr[:, -1])
        lerr = np.abs(level - Cl) / np.maximum(Cl, 0.01)
        print(f"  carrier level worst {lerr.max():.3g}")
        assert level.dtype == np.float32 and lerr.max() <= 1e-6
    assert (bits(r["level"][0]) == bits(r["level"][1])).all()


@pytest.mark.parametrize("D,L", CASES, ids=IDS)
def test_ambank_cuts_give_the_same_bits(ld, D, L):
    r = run("am", ld, D, L)
    cut, y = ragged(r["make"], r["x"], D, 1)
    assert (bits(y) == bits(r["y"][0])).all()
    assert (bits(cut.carrier_level) == bits(r["level"][0])).all()


# ---------------------------------------------------------------- StereoBank
@pytest.mark.parametrize("D,L", CASES, ids=IDS)
def test_stereobank_parity_with_definition(ld, D, L):
    r = run("st", ld, D, L)
    C, K, y, ref = r["C"], r["x"].shape[1], r["y"], r["ref"]
    assert y.dtype == np.float32 and y.shape == (C, 2, -(-K // D)) and r["skip"] == (-K) % D
    assert np.isfinite(y).all()
    assert ref.edge.sum() <= 0.01 * ref.edge.size
    if bp.tilted(L):
        el, er = t_st.worst(y[:, 0], ref.left, ~ref.edge), t_st.worst(y[:, 1], ref.right, ~ref.edge)
        print(f"StereoBank D={D} L={L}: left worst {el.max():.3g}, right worst {er.max():.3g} of the row maximum, "
              f"{int(ref.edge.sum())} columns left out")
        assert el.max() <= GATE and er.max() <= GATE, (float(el.max()), float(er.max()))
    else:
        keep = ~ref.edge & (ref.scale > 0)
        el = np.where(keep, np.abs(y[:, 0] - ref.left), 0.0) / np.where(keep, ref.scale, 1.0)
        er = np.where(keep, np.abs(y[:, 1] - ref.right), 0.0) / np.where(keep, ref.scale, 1.0)
        print(f"StereoBank D={D} L={L}: left worst {el.max():.3g}, right worst {er.max():.3g} of the arithmetic's scale, "
              f"{int(ref.edge.sum())} columns left out, {int(ref.on.sum())} of {ref.on.size} columns in stereo")
        assert el.max() <= GATE and er.max() <= GATE, (float(el.max()), float(er.max()))
        assert (ref.scale[[0, 2]] > 0).all()                               # an all-zero window: the zero row's alone
    assert (bits(y[1]) == 0).all()                                         # the zero row: +0.0
    Pl = np.abs(ref.P[:, -1])
    lerr = np.abs(r["level"] - Pl) / np.maximum(Pl, t_st.AP / 2)
    print(f"  pilot level worst {lerr.max():.3g}")
    assert r["level"].dtype == np.float32 and lerr.max() <= 1e-5


@pytest.mark.parametrize("D,L", CASES, ids=IDS)
def test_stereobank_cuts_give_the_same_bits(ld, D, L):
    r = run("st", ld, D, L)
    cut, y = ragged(r["make"], r["x"], D, 2)
    assert (bits(y) == bits(r["y"])).all()
    assert (bits(cut.pilot_level) == bits(r["level"])).all()


# ---------------------------------------------------------------- SSBBank
@pytest.mark.parametrize("D,L", CASES, ids=IDS)
def test_ssbbank_parity_with_definition(ld, D, L):
    r = run("ssb", ld, D, L)
    C, K, y, ref = r["C"], r["x"].shape[1], r["y"], r["ref"]
    assert y.dtype == np.float32 and y.shape == (C, -(-K // D)) == ref.y.shape and r["skip"] == (-K) % D
    assert np.isfinite(y).all()
    if bp.tilted(L):
        rel, res = t_sb.gate_rows(y, ref, r["signal"])
        print(f"SSBBank D={D} L={L}: signal rows worst {rel:.3g} of the row maximum, residue rows worst {res:.3g} "
              f"of the arithmetic's scale")
        assert rel <= GATE and res <= GATE, (rel, res)
        assert (bits(y[1]) == 0).all()                                     # the zero row: +0.0
    else:
        assert (ref.scale > 0).all()
        over = np.abs(y.astype(np.float64) - ref.y) / ref.scale
        print(f"SSBBank D={D} L={L}: worst {over.max():.3g} of the arithmetic's scale per column")
        assert over.max() <= GATE, float(over.max())


@pytest.mark.parametrize("D,L", CASES, ids=IDS)
def test_ssbbank_cuts_give_the_same_bits(ld, D, L):
    r = run("ssb", ld, D, L)
    _, y = ragged(r["make"], r["x"], D, 1)
    assert (bits(y) == bits(r["y"])).all()


# ---------------------------------------------------------------- the longest prototype with its window filled
@pytest.mark.parametrize("kind", ["am", "st", "ssb"])
def test_longest_prototype_behind_a_lead(ld, kind):
    """(D, L) = (2, 1025): the call of D (2 tile + 1) + 3 samples is shorter than the history, so in the case above
    the taps j > nD meet zeros alone.  Here whole tiles are put in front and the columns whose window lies
    inside the stream are held to the tilted designs' gates, so every tap meets a sample.  The start-up columns
    before them are not judged: at L = 1025 the AMBank's carrier estimate passes through cancellation there
    (|Cr| 50 times below sum |g[j] x| at |B| <= |Cr|), where no float32 evaluation meets the flat 1e-6 (measured
    1.39e-6 in two columns, 1.4e-8 of the arithmetic's scale; a numpy float32 restatement of the kernel's
    order of operations gives the same figure to the last digit)."""
    D, L = bp.LONGEST
    if kind == "am":
        cs = bp.am_case(ld, D, L, lead=True)
        st = cs["ref"][0].steady[0]
        assert st.sum() >= 2 * 64 + 1
        for thr, ref in zip(bp.AM_THR, cs["ref"]):
            y = cs["make"](thr)(cs["x"])
            err = np.abs(y.astype(np.float64) - ref.y)[:, st]
            full = ~ref.beyond[:, st]
            assert full[cs["carried"]].all() and not ref.edge.any()
            over = err / ref.scale[:, st]
            print(f"AMBank D={D} L={L} thr={thr:g} behind a lead: worst absolute {err[full].max():.3g} within full scale, "
                  f"{over.max():.3g} of the arithmetic's scale")
            assert err[full].max() <= GATE and over.max() <= GATE
    elif kind == "st":
        cs = bp.st_case(ld, D, L, lead=True)
        ref, y = cs["ref"], cs["make"]()(cs["x"])
        keep = ~ref.edge & bp.steady(D, L, y.shape[2])[None, :]
        assert ref.on[cs["pilot"]][:, keep[0]].all()
        el, er = t_st.worst(y[:, 0], ref.left, keep), t_st.worst(y[:, 1], ref.right, keep)
        print(f"StereoBank D={D} L={L} behind a lead: left worst {el.max():.3g}, right worst {er.max():.3g} of the row maximum")
        assert el.max() <= GATE and er.max() <= GATE
    else:
        cs = bp.ssb_case(ld, D, L, lead=True)
        sb = cs["make"]()
        y = sb(cs["x"])
        ref = t_sb.Ref(sb.row_taps, sb.words, D, cs["x"])
        st = bp.steady(D, L, y.shape[1])
        rel, res = t_sb.gate_rows(y[:, st], SimpleNamespace(y=ref.y[:, st], scale=ref.scale[:, st]), cs["signal"])
        print(f"SSBBank D={D} L={L} behind a lead: signal rows worst {rel:.3g} of the row maximum, residue rows worst "
              f"{res:.3g} of the arithmetic's scale")
        assert rel <= GATE and res <= GATE


# ---------------------------------------------------------------- (c) create_taps against create
def test_ambank_from_read_back_prototypes(ld):
    shape = (3, 5, 251, None, 0.016)
    a = t_am.make(ld, *shape)
    b = ld.AMBank(3, 5, taps=a.taps, carrier_taps=a.carrier_taps)
    x, _, _ = t_am.rows_for(8100, 3, 5 * (2 * a.tile + 1) + 3, t_am.cutoff(5, None), 0.016, 251)
    assert (bits(b.band_taps) == bits(a.band_taps)).all()
    assert (bits(b(x)) == bits(a(x))).all() and (bits(b.carrier_level) == bits(a.carrier_level)).all()


def test_stereobank_from_read_back_prototypes(ld):
    a = ld.StereoBank(3, t_st.PILOT, 5)
    b = ld.StereoBank(3, t_st.PILOT, 5, taps=a.taps, pilot_taps=a.pilot_taps)
    x, _ = t_st.rows_for(8200, 3, 5 * (2 * a.tile + 1) + 3)
    assert (bits(b(x)) == bits(a(x))).all() and (bits(b.pilot_level) == bits(a.pilot_level)).all()


def test_ssbbank_from_read_back_prototypes(ld):
    shape = (3, 2, 81, 0.025, 0.225)
    bfo, side = np.array([0.0, 0.123456789, -0.3141592653589793]), np.array([1, -1, 1])
    a = t_sb.make(ld, shape, bfo, side)
    b = ld.SSBBank(3, 2, lo=0.025, hi=0.225, bfo=bfo, sideband=[t_sb.NAMES[int(s)] for s in side], taps=a.taps)
    x, _ = t_sb.rows_for(8300, 3, 2 * (2 * a.tile + 1) + 3, 0.025, 0.225, bfo, side)
    assert (bits(b.row_taps) == bits(a.row_taps)).all()
    assert (bits(b(x)) == bits(a(x))).all()


# ---------------------------------------------------------------- identities
J0 = [0, 1, 7, 8, 16]


def delayed(u, D, j0, ncols):
    """u[:, nD - j0] over n < ncols, +0.0 before the stream's start."""
    at = np.arange(ncols) * D - j0
    return np.where(at[None, :] >= 0, u[:, np.maximum(at, 0)], np.zeros((), u.dtype))


@pytest.mark.parametrize("j0", J0)
def test_stereobank_unit_sample_returns_the_input(ld, j0):
    """taps = delta[j - j0], pilot_taps = 0: m = 0 is not above thr^2, so left = right = s, and s is one
    fmaf(1, u, +0) plus exact zeros: y[c, 0] == y[c, 1] == u[c, nD - j0] bit for bit (an all-zero pilot prototype
    is accepted at creation)."""
    D, L, C = 8, 17, 2
    h = np.zeros(L, np.float32)
    h[j0] = 1.0
    sb = ld.StereoBank(C, t_st.PILOT, D, taps=h, pilot_taps=np.zeros(L, np.float32))
    u = np.random.default_rng(8400 + j0).standard_normal((C, D * (2 * sb.tile + 1) + 3)).astype(np.float32)
    assert (u != 0).all()                             # no negative zero
    y = sb(u)
    want = delayed(u, D, j0, y.shape[2])
    assert (bits(y[:, 0]) == bits(want)).all() and (bits(y[:, 1]) == bits(want)).all()
    assert (sb.pilot_level == 0).all()


@pytest.mark.parametrize("j0", J0)
def test_ssbbank_unit_sample_returns_one_complex_product(ld, j0):
    """taps = delta[j - j0], bfo = 0, both sidebands: the rotation is exactly 1, so
    y = fl(fl(gr x_re) - fl(gi x_im)) with (gr, gi) = row_taps[c, j0], bit for bit."""
    D, L, C = 8, 17, 2
    p = np.zeros(L, np.float32)
    p[j0] = 1.0
    sb = ld.SSBBank(C, D, lo=0.1 / D, hi=0.4 / D, bfo=0.0, sideband=["usb", "lsb"], taps=p)
    assert (sb.words == 0).all()
    g = sb.row_taps
    assert (np.delete(g, j0, axis=1) == 0).all() and (np.abs(g[:, j0]) > 0.99).all()
    rng = np.random.default_rng(8500 + j0)
    x = (rng.standard_normal((C, D * (2 * sb.tile + 1) + 3)) + 1j * rng.standard_normal((C, D * (2 * sb.tile + 1) + 3)))
    x = x.astype(np.complex64)
    assert (x.real != 0).all() and (x.imag != 0).all()
    y = sb(x)
    xd = delayed(x, D, j0, y.shape[1])
    gr, gi = g[:, j0].real.astype(np.float32)[:, None], g[:, j0].imag.astype(np.float32)[:, None]
    want = (gr * xd.real.astype(np.float32)).astype(np.float32) - (gi * xd.imag.astype(np.float32)).astype(np.float32)
    assert want.dtype == np.float32
    assert (bits(y) == bits(want + np.float32(0.0))).all()
