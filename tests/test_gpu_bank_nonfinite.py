"""One non-finite sample stays where the definition puts it.  For each bank
object two fresh objects run over the same finite input, fed as two calls; in
the second run one sample (row r, position t0 in the kernel's second tile, off
the tile's edges) is NaN or +inf in both of its components.  The calls are cut a
few columns after t0, so the bad sample also passes through the history pair.

0 * NaN is NaN, so the outputs whose bits differ from the clean run's are the
exact read footprint of the kernel, which a tolerance of 1e-6 of the row maximum
cannot see.  Compared bitwise against the clean run:

  * every other row is identical in every output and read-back;
  * in row r (in every row of Channelizer and Downconverter, whose one input
    stream feeds all rows, and there the same columns in every row) the columns
    before the footprint are identical, and for the FIR-class objects the
    columns after it too, in the same call and in the next;
  * somewhere inside the footprint the bits differ (the sample was read);
  * recursive parts (AudioBank with de-emphasis, SquelchBank's level, the
    Spectrogram's psd) may stay non-finite from the footprint on, and reset()
    (clear() for the psd) followed by the clean input gives the clean bits again;
  * no output of the clean run is non-finite, and the float64 definition of the
    clean input, from each object's own test module, is finite.

The footprint is the definition's, from the object's own taps, decim and skip:
Downconverter, StereoBank, FMBank columns n with 0 <= nD - t0 < L (FMBank for
t0 and t0 + 1, through conj(x[t-1]) x[t]); AudioBank without de-emphasis the
outputs whose 2 len window ends at j_k with j_k - 2 len < t0 <= j_k; Spectrogram
the transforms whose W samples contain t0 and the rows that average them.  Two
kernels multiply zero-padded taps by staged samples past the definition's
footprint (k_chan.hip and k_synth.hip keep ceil(L / M) taps per branch and
ceil(L / D) per output residue, zero past L), so their bound is the padded one:

  * Channelizer: columns n with 0 <= nD - t0 < ceil(L / M) M   (definition: < L);
  * Synthesizer: outputs t with n0 D <= t < (n0 + ceil(L / D)) D for a bad
    sample in column n0                                      (definition: < n0 D + L).

int16 IQ input has no non-finite value: from_bytes is not covered here."""
import numpy as np
import pytest

import test_gpu_audiobank as t_ab
import test_gpu_channelizer as t_ch
import test_gpu_downconverter as t_dc
import test_gpu_fmbank as t_fm
import test_gpu_spectrogram as t_sp
import test_gpu_squelchbank as t_sq
import test_gpu_stereobank as t_st
import test_gpu_synthesizer as t_sy
from conftest import cgauss

pytestmark = pytest.mark.gpu

VALUES = pytest.mark.parametrize("value", [np.nan, np.inf], ids=["nan", "inf"])
ROW = 5                                               # the bad row: not the first, not the last, a noise row


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view({1: np.uint8, 2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def col_same(a, b):
    """bool[rows, cols]: a and b carry the same bits (over any axes between the first and the last)."""
    assert a.shape == b.shape and a.dtype == b.dtype, (a.shape, b.shape)
    e = bits(a) == bits(b)
    if e.ndim == 1:
        e = e[None, :]
    while e.ndim > 2:
        e = e.all(axis=1)
    return e


def poisoned(x, at, value):
    bad = np.array(x)
    bad[at] = complex(value, value) if np.iscomplexobj(bad) else value
    return bad


def contained(clean, bad, dirty, row=None, recursive=False, what=""):
    """dirty: bool[cols], the footprint.  With a row: every other row identical, the rest on
    that row alone; without: on every row, and the same columns differ in every row."""
    assert clean.dtype.kind not in "fc" or np.isfinite(clean).all(), what
    e = col_same(clean, bad)
    assert dirty.shape == (e.shape[1],) and dirty.any(), what
    keep = np.arange(dirty.size) < np.flatnonzero(dirty)[0] if recursive else ~dirty
    if row is not None:
        others = np.delete(e, row, axis=0)
        assert others.all(), (what, "another row changed", np.argwhere(~others)[:4].tolist())
        e = e[row:row + 1]
    else:
        assert (e == e[0]).all(), (what, "the rows differ in different columns")
    assert e[:, keep].all(), (what, "outside the footprint", np.flatnonzero(~e.all(axis=0) & keep)[:8].tolist())
    assert not e[:, dirty].all(), (what, "the bad sample was not read")
    off = np.flatnonzero(~e.all(axis=0))
    print(f"{what}: columns {off[0]} .. {off[-1]} differ, footprint {np.flatnonzero(dirty)[0]} .. {np.flatnonzero(dirty)[-1]}")


def two_calls(obj, x, cut, call=None):
    """The outputs of obj over x[..., :cut] and x[..., cut:], each a tuple of arrays."""
    call = call or (lambda o, p: (o(p),))
    return [call(obj, np.ascontiguousarray(p)) for p in (x[..., :cut], x[..., cut:])]


def joined(parts, i, axis=-1):
    return np.concatenate([p[i] for p in parts], axis=axis)


def decim_layout(F, D, span):
    """t0 in the second tile's middle, the cut two columns after it, a length of two tiles, a
    column and a ragged tail that also leaves the footprint behind."""
    t0 = D * (F + F // 2) + 1
    return t0, t0 + 2 * D + 1, max(D * (2 * F + 1) + 3, t0 + span + 3 * D + 3)


# ---------------------------------------------------------------- Channelizer, Downconverter: one stream, every row
@VALUES
@pytest.mark.parametrize("M,m,D", [(16, 6, 16), (8, 6, 4)])
def test_channelizer(ld, value, M, m, D):
    """The footprint is the padded one, ceil(L / M) M samples: k_chan.hip sums ceil(L / M) taps per
    branch, the taps zero past L, so the columns with L <= nD - t0 < ceil(L / M) M multiply a zero
    tap by the bad sample.  Every row sees it, in the same columns."""
    mk = lambda: ld.Channelizer(M, D, m=m)
    ch = mk()
    L = len(ch.taps)
    PM = -(-L // M) * M
    t0, cut, N = decim_layout(ch.tile, D, PM)
    x = cgauss(np.random.default_rng(100 + M), N)
    assert np.isfinite(t_ch.definition(x, ch.taps, ch.scale, M, D, -(-N // D))).all()
    clean, bad = two_calls(mk(), x, cut), two_calls(mk(), poisoned(x, t0, value), cut)
    lag = np.arange(-(-N // D)) * D - t0
    assert cut - t0 < L and ((lag >= L) & (lag < PM)).any() and (lag >= PM).sum() >= 3
    contained(joined(clean, 0), joined(bad, 0), (lag >= 0) & (lag < PM), what=f"Channelizer M={M} D={D} L={L} padded {PM}")


@VALUES
@pytest.mark.parametrize("C,D,m", [(3, 5, 6), (16, 64, 6)])
def test_downconverter(ld, value, C, D, m):
    f = t_dc.freqs_for(np.random.default_rng(200 + C), C)
    mk = lambda: ld.Downconverter(f, D, m=m)
    dc = mk()
    L = len(dc.taps)
    t0, cut, N = decim_layout(dc.tile, D, L)
    x = cgauss(np.random.default_rng(210 + D), N)
    assert np.isfinite(t_dc.definition(x, dc.taps, dc.scale, dc.words, D)).all()
    clean, bad = two_calls(mk(), x, cut), two_calls(mk(), poisoned(x, t0, value), cut)
    lag = np.arange(-(-N // D)) * D - t0
    assert cut - t0 < L and (lag >= L).sum() >= 3
    contained(joined(clean, 0), joined(bad, 0), (lag >= 0) & (lag < L), what=f"Downconverter C={C} D={D} L={L}")


# ---------------------------------------------------------------- Synthesizer: input rows, one output stream
@VALUES
@pytest.mark.parametrize("M,m,D", [(16, 6, 8), (16, 6, 16)])
def test_synthesizer(ld, value, M, m, D):
    """A bad sample in row ROW, column n0.  The footprint is the padded one, the D outputs of each
    of the ceil(L / D) columns from n0 on: k_synth.hip sums ceil(L / D) taps per output residue,
    the taps zero past L."""
    mk = lambda: ld.Synthesizer(M, D, m=m)
    sy = mk()
    F, L = sy.tile, len(sy.taps)
    Q = -(-L // D)
    n0 = F + F // 2 + 1
    K = max(2 * F + 1 + Q, n0 + Q + 5)
    y = t_sy.cgauss2(np.random.default_rng(300 + D), M, K)
    assert np.isfinite(t_sy.definition(y, sy.taps, sy.scale, M, D)).all()
    clean, bad = two_calls(mk(), y, n0 + 2), two_calls(mk(), poisoned(y, (ROW, n0), value), n0 + 2)
    t = np.arange(K * D)
    assert 2 < Q and ((t >= n0 * D + L) & (t < (n0 + Q) * D)).any()
    contained(joined(clean, 0), joined(bad, 0), (t >= n0 * D) & (t < (n0 + Q) * D),
              what=f"Synthesizer M={M} D={D} L={L} padded {Q * D}")


# ---------------------------------------------------------------- FMBank
@VALUES
@pytest.mark.parametrize("D,m", [(8, 6), (1, 0)])
def test_fmbank(ld, ora, value, D, m):
    """One workgroup per row and tile (k_fmbank.hip), 16 rows.  d[t0] and d[t0 + 1] read the bad sample."""
    C = 16
    mk = (lambda: ld.FMBank(C, t_fm.KF, D, m=m)) if m else (lambda: ld.FMBank(C, t_fm.KF))
    fb = mk()
    L = max(len(fb.taps), 1)                         # the discriminator alone: y = d
    t0, cut, K = decim_layout(fb.tile, D, L + 1)
    x = t_fm.rows_for(400 + D, C, K)
    d = t_fm.disc(ora, x)
    assert np.isfinite(d).all() and (not m or np.isfinite(t_fm.definition(d, fb.taps, fb.scale, D)).all())
    clean, bad = two_calls(mk(), x, cut), two_calls(mk(), poisoned(x, (ROW, t0), value), cut)
    lag = np.arange(-(-K // D)) * D - t0
    assert (lag >= L + 1).sum() >= 3
    contained(joined(clean, 0), joined(bad, 0), (lag >= 0) & (lag < L + 1), row=ROW, what=f"FMBank D={D} L={L}")


# ---------------------------------------------------------------- AudioBank
def audio_case(ld, sr, pcm16=False):
    C, rate, m, npfb = 16, 0.192, 20, 13
    mk = lambda: ld.AudioBank(C, rate, m, nfilter=npfb, deemphasis=sr, pcm16=pcm16)
    ab = mk()
    T = ab.tile
    t0 = int((T + T // 2) / rate) + 1
    K = max(t_ab.samples_for(ab), t0 + 2 * m + 40)
    x = t_ab.rows_for(500, C, K)
    j, _ = t_ab.schedule(ab.step, 0, ab.nfilter, K)
    assert np.isfinite(t_ab.definition(ab, x)).all()
    assert T < np.searchsorted(j, t0) < 2 * T and (j - 2 * m >= t0).sum() >= 3
    return mk, x, t0, t0 + 7, j, m


@VALUES
def test_audiobank_without_deemphasis(ld, value):
    """FIR-class: the outputs whose window of 2 len samples, ending at j_k, holds t0."""
    mk, x, t0, cut, j, m = audio_case(ld, None)
    clean, bad = two_calls(mk(), x, cut), two_calls(mk(), poisoned(x, (ROW, t0), value), cut)
    contained(joined(clean, 0), joined(bad, 0), (j >= t0) & (j - 2 * m < t0), row=ROW, what="AudioBank, no de-emphasis")


@VALUES
@pytest.mark.parametrize("pcm16", [False, True], ids=["float", "pcm16"])
def test_audiobank_with_deemphasis(ld, value, pcm16):
    """Recursive: row ROW may stay non-finite from the first window that holds t0 (what a NaN
    rounds to in the PCM row is not specified); the rows before it and the other rows are
    identical, and reset() leaves no poisoned state behind."""
    mk, x, t0, cut, j, m = audio_case(ld, 250e3, pcm16)
    obj = mk()
    clean, bad = two_calls(mk(), x, cut), two_calls(obj, poisoned(x, (ROW, t0), value), cut)
    contained(joined(clean, 0), joined(bad, 0), j >= t0, row=ROW, recursive=True, what=f"AudioBank, de-emphasis, pcm16={pcm16}")
    obj.reset()
    again = obj(np.ascontiguousarray(x[:, :cut]))
    assert col_same(again, clean[0][0]).all()


# ---------------------------------------------------------------- SquelchBank
@VALUES
@pytest.mark.parametrize("C,B,alpha,timeout,row", [(16, 1024, 1.0, 2, ROW), (256, 64, 0.25, 1, 100)])
def test_squelchbank(ld, value, C, B, alpha, timeout, row):
    """k_sqbank_fsm steps the rows one lane per row, so the rows of a bank share its waves: 16
    rows in one wave, 256 in four.  The level is recursive: row `row` may stay non-finite from
    the bad sample's block on; the blocks before it and every other row, state included, are
    identical, and reset() leaves no poisoned state behind."""
    mk = lambda: t_sq.make(ld, C, B, alpha, timeout)
    T = mk().tile
    x, level, _ = t_sq.case(T, C, B, alpha, timeout)
    assert np.isfinite(level).all()
    b0 = T + T // 2
    t0 = b0 * B + B // 2 + 1
    cut = t0 + 5                                      # inside the block: the bad sample is carried to the next call
    nb = level.shape[1]
    assert T < b0 < 2 * T and nb > b0 + 2

    def call(o, p):
        y = o(p)
        return y, o.status, o.level

    obj = mk()
    clean, bad = two_calls(mk(), x, cut, call), two_calls(obj, poisoned(x, (row, t0), value), cut, call)
    blocks = np.arange(nb) >= b0
    what = f"SquelchBank C={C} B={B}"
    contained(joined(clean, 0), joined(bad, 0), np.repeat(blocks, B), row=row, recursive=True, what=what + " gate")
    contained(joined(clean, 2), joined(bad, 2), blocks, row=row, recursive=True, what=what + " level")
    st = col_same(joined(clean, 1), joined(bad, 1))
    assert np.delete(st, row, axis=0).all() and st[row, :b0].all()
    ref = mk()
    two_calls(ref, x, cut, call)
    for got, want in zip(obj.state, ref.state):
        assert (bits(np.delete(got, row)) == bits(np.delete(want, row))).all()
    obj.reset()
    again = call(obj, np.ascontiguousarray(x[:, :cut]))
    assert all(col_same(a, c).all() for a, c in zip(again, clean[0]))
    assert all((bits(g) == bits(w)).all() for g, w in zip(obj.state, mk_state(mk, x, cut, call)))


def mk_state(mk, x, cut, call):
    o = mk()
    call(o, np.ascontiguousarray(x[:, :cut]))
    return o.state


# ---------------------------------------------------------------- StereoBank
@VALUES
def test_stereobank(ld, value):
    """One workgroup per row and tile (k_stbank.hip), 16 rows.  The pilot level is that of the
    call's last column: inside the footprint after the first call, past it after the second."""
    C, D, L = 16, 4, 181
    mk = lambda: ld.StereoBank(C, t_st.PILOT, D, ntaps=L)
    sb = mk()
    t0, cut, K = decim_layout(sb.tile, D, L)
    x, _ = t_st.rows_for(600, C, K)
    ref = t_st.Ref(sb, x, t_st.THR)
    assert np.isfinite(ref.left).all() and np.isfinite(ref.right).all()
    assert not ref.edge.any()                         # no column on the threshold's edge (test_gpu_stereobank.py)

    def call(o, p):
        y = o(p)
        return y, o.pilot_level, o.stereo

    clean, bad = two_calls(mk(), x, cut, call), two_calls(mk(), poisoned(x, (ROW, t0), value), cut, call)
    lag = np.arange(-(-K // D)) * D - t0
    assert cut - t0 < L and (lag >= L).sum() >= 3
    contained(joined(clean, 0), joined(bad, 0), (lag >= 0) & (lag < L), row=ROW, what=f"StereoBank D={D} L={L}")
    for i in (1, 2):                                  # pilot_level, stereo
        first = bits(clean[0][i]) == bits(bad[0][i])
        assert np.delete(first, ROW).all()
        assert (bits(clean[1][i]) == bits(bad[1][i])).all()
    assert not (bits(clean[0][1]) == bits(bad[0][1]))[ROW]


# ---------------------------------------------------------------- Spectrogram
@VALUES
@pytest.mark.parametrize("N,W,d,A,window", [(1024, 300, 7, 3, "hann"), (1024, 1024, 64, 24, "hamming")])
def test_spectrogram(ld, value, N, W, d, A, window):
    """The rows are FIR-class: the transforms whose W samples hold t0, and the rows that average
    them.  The psd is recursive: it may stay non-finite; clear() once the bad sample has left the
    history and the unfinished row gives the bits of a clean object cleared at the same place,
    and reset() the clean run's first call."""
    mk = lambda: t_sp.make(ld, N, W, d, A, window)
    F = mk().tile
    t0 = d * (F + F // 2) + 1
    cut = t0 + 2 * d + 1
    n = max(t_sp.base_len(F, d, A), t0 + W + 3 * d * A + 3)
    x = t_sp.signal(700 + N + d, n + d * (A + 1) + 2, N)
    more, x = x[n:], x[:n]
    assert np.isfinite(t_sp.definition(x, mk().window, N, d, 0, n // d)).all()

    def call(o, p):
        return (o(p),)

    a, b = mk(), mk()
    clean, bad = two_calls(a, x, cut, call), two_calls(b, poisoned(x, t0, value), cut, call)
    s = np.arange(n // d)
    hit = ((s + 1) * d - W <= t0) & (t0 <= (s + 1) * d - 1)            # the transforms that read t0
    rows = np.zeros(n // d // A, bool)
    rows[np.unique(s[hit] // A)[np.unique(s[hit] // A) < rows.size]] = True
    assert cut - t0 < W and rows.any() and not rows[-3:].any() and not hit[-(A + 1):].any()
    got_c, got_b = joined(clean, 0, axis=0), joined(bad, 0, axis=0)
    contained(got_c.T, got_b.T, rows, what=f"Spectrogram N={N} W={W} d={d} A={A}")   # [bins, rows]: every bin alike
    assert np.isfinite(a.psd).all() and a.num_transforms == b.num_transforms == n // d
    assert not (bits(a.psd) == bits(b.psd)).all()
    for o in (a, b):
        o.clear()
    ra, rb = a(more), b(more)
    assert ra.shape[0] >= 1 and col_same(ra, rb).all()
    assert a.num_transforms == b.num_transforms > 0 and (bits(a.psd) == bits(b.psd)).all()
    c = mk()
    first = c(np.ascontiguousarray(x[:cut]))
    b.reset()
    assert col_same(b(np.ascontiguousarray(x[:cut])), first).all() and (bits(b.psd) == bits(c.psd)).all()
