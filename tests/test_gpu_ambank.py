"""AMBank on the GPU: the feed-forward coherent AM demodulator over bank rows
(k_ambank.hip) against its definition (include/ldsp.h),

    d[j]     = (float)((double)h[j] - (double)g[j])
    B[c][n]  = sum_{j<L} d[j] x[c][nD-j]
    Cr[c][n] = sum_{j<L} g[j] x[c][nD-j]
    m = |Cr|^2,  y[c][n] = m > thr^2 ? Re(B conj(Cr)) / m : 0

evaluated here in float64 from the object's own float32 taps, carrier_taps and
band_taps.  Rows are seeded AM, x = A (1 + a(t)) exp(i (2 pi f0 t + phi)) + noise:
A between 0.01 and 1, a(t) four tones between 1.5 carrier + |f0| and
audio - 2 / L - |f0| at a modulation index of 0.3 to 0.8, |f0| <= 0.4 carrier,
complex noise of deviation up to 0.03 A.  Wherever C >= 4, row 1 is 0
throughout, row 2 has index 0.05 and row 3 is noise of deviation 0.005 without a
carrier.  Sizes come from the kernel's tile (F output columns per workgroup):
one call of D (2F + 1) + 3 samples per row is two full tiles, a ragged third
and a non-zero skip afterwards.

The gate of the parity test is 1e-6 absolute (y = 1 is 100 % modulation): the
project's gate for FIR-class kernels taken against the scale of
the arithmetic, the carrier, and not against the modulation depth, which can be
arbitrarily small.  It holds flat for every column within full scale,
|B| <= |Cr|: all columns of a row with a carrier once its window lies inside the
stream.  Beyond full scale -- the first columns of a stream, whose window is
mostly the zeros before its start and whose carrier estimate is a few edge taps
(|y| reaches 1e6 there, where float32 values are 0.25 apart), and the noise row
at a threshold of 0 -- no float32 evaluation can meet a flat 1e-6, and the same
1e-6 is taken against the scale of y's own arithmetic, from
dy = dB / Cr - B dCr / Cr^2 with |dB| <= 1e-6 sum |d[j] x| and
|dCr| <= 1e-6 sum |g[j] x|:  |dy| <= 1e-6 (SB / |Cr| + |B| SC / |Cr|^2).
The figure relative to the row's maximum is printed for the rows of index
>= 0.3.  Columns whose reference m lies within 1e-4 (relative) of
thr^2 could fall on either side of the float32 comparison; the test asserts
that there is none.  Streams cut into calls, banks of other sizes and row
orders, inputs read in place, a threshold set between calls, reset() and a
host-memory call must give the same bits."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GATE = 1e-6
THR = 1e-3                                            # the threshold of the second parity run
# (C, D, L, audio, carrier): carrier = 4 / (L - 1), the cut-off whose default length is L; audio None: 0.5 / D (0.45 at D = 1)
SHAPES = [(1, 1, 33, None, 0.125), (3, 5, 251, None, 0.016), (16, 4, 181, None, 4 / 180), (5, 8, 363, None, 4 / 362),
          (256, 3, 65, 0.3, 0.0625), (2, 32, 1025, None, 4 / 1024)]
IDS = [f"{s[0]}-{s[1]}-{s[2]}" for s in SHAPES]


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(ld, C, D, L, audio, carrier, **kw):
    return ld.AMBank(C, D, audio=audio, carrier=carrier, ntaps=L, **kw)


def cutoff(D, audio):
    return audio or (0.45 if D == 1 else 0.5 / D)


def am_row(seed, K, audio, carrier, L, index=None, A=None, sigma=None, f0=None):
    """One row in complex128 over t = 0 .. K - 1 and its modulation a(t) as a function of t."""
    rng = np.random.default_rng(seed)
    A = 10.0 ** rng.uniform(-2.0, 0.0) if A is None else A
    index = rng.uniform(0.3, 0.8) if index is None else index
    f0 = rng.uniform(-0.4, 0.4) * carrier if f0 is None else f0
    sigma = rng.uniform(0.0, 0.03) if sigma is None else sigma
    lo, hi = 1.5 * carrier + abs(f0), audio - 2.0 / L - abs(f0)
    assert lo < hi, (lo, hi)
    f = rng.uniform(lo, hi, 4)
    ph = rng.uniform(0.0, 1.0, 4)
    w = rng.uniform(0.3, 1.0, 4)
    w /= w.sum()

    def a(t):
        return index * (w[:, None] * np.sin(2 * np.pi * (f[:, None] * t[None, :] + ph[:, None]))).sum(axis=0)

    t = np.arange(K, dtype=np.float64)
    x = A * (1.0 + a(t)) * np.exp(2j * np.pi * (f0 * t + rng.uniform(0.0, 1.0)))
    if sigma > 0:
        x = x + sigma * A * (rng.standard_normal(K) + 1j * rng.standard_normal(K)) / np.sqrt(2)
    return x, a, index


def rows_for(seed, C, K, audio, carrier, L):
    """complex64 [C][K] (read-only), the rows that carry a carrier, and the rows of index >= 0.3."""
    rows = [am_row(seed + 31 * c, K, audio, carrier, L) for c in range(C)]
    x = np.stack([r[0] for r in rows])
    am, deep = np.ones(C, bool), np.ones(C, bool)
    if C >= 4:
        x[1] = 0
        x[2] = am_row(seed + 5, K, audio, carrier, L, index=0.05)[0]
        rng = np.random.default_rng(seed + 7)
        x[3] = 0.005 * (rng.standard_normal(K) + 1j * rng.standard_normal(K)) / np.sqrt(2)
        am[[1, 3]] = False
        deep[[1, 2, 3]] = False
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x, am, deep


class Ref:
    """The definition in float64 over complex64 rows x fed from t = 0, one threshold."""

    def __init__(self, g, d, D, x, thr):
        x = np.asarray(x).astype(np.complex128)
        g, d = np.asarray(g).astype(np.float64), np.asarray(d).astype(np.float64)
        L, K = g.size, x.shape[1]
        ncols = -(-K // D)
        t = np.arange(ncols, dtype=np.int64)[:, None] * D - np.arange(L, dtype=np.int64)[None, :]    # [ncols][L]
        xp = np.concatenate([np.zeros((x.shape[0], L - 1), np.complex128), x], axis=1)              # xp[:, t + L - 1] = x[:, t]
        self.B = np.empty((x.shape[0], ncols), np.complex128)
        self.Cr = np.empty((x.shape[0], ncols), np.complex128)
        SB, SC = np.empty(self.B.shape), np.empty(self.B.shape)               # sum |d[j]| |x|, sum |g[j]| |x|
        for c in range(x.shape[0]):                   # row by row: [ncols][L] at a time
            U = xp[c][t + L - 1]
            self.B[c], self.Cr[c] = U @ d, U @ g
            SB[c], SC[c] = np.abs(U) @ np.abs(d), np.abs(U) @ np.abs(g)
        self.m = np.abs(self.Cr) ** 2
        thr2 = float(np.float32(thr) * np.float32(thr))
        self.on = self.m > thr2
        # either side in float32; at thr = 0 the comparison is m > 0, and m = 0 comes from an all-zero window alone,
        # which is 0 in float32 as well
        self.edge = (np.abs(self.m - thr2) <= 1e-4 * thr2) & (self.m > 0)
        with np.errstate(divide="ignore", invalid="ignore"):
            self.y = np.where(self.on, np.real(self.B * np.conj(self.Cr)) / self.m, 0.0)
            # beyond full scale: |B| > |Cr|, more than 100 % (see the module's docstring); the scale of y's
            # arithmetic there, from dy = dB / Cr - B dCr / Cr^2 with |dB| <= gate SB and |dCr| <= gate SC
            aB, aC = np.abs(self.B), np.abs(self.Cr)
            self.beyond = self.on & (aB > aC)
            self.scale = np.where(self.beyond, SB / aC + aB * SC / aC ** 2, 1.0)
        self.steady = np.broadcast_to(np.arange(ncols) * D >= L - 1, self.y.shape)   # the window holds no sample before 0


_cases = {}


def case(ld, shape):
    """One call per shape at each of the two thresholds, computed once and shared."""
    if shape not in _cases:
        C, D, L, audio, carrier = shape
        am0 = make(ld, *shape)
        K = D * (2 * am0.tile + 1) + 3
        x, carried, deep = rows_for(2000 + 7 * C + D, C, K, cutoff(D, audio), carrier, L)
        y0 = am0(x)
        lv0 = am0.carrier_level.copy()
        am1 = make(ld, *shape, threshold=THR)
        y1 = am1(x)
        refs = [Ref(am0.carrier_taps, am0.band_taps, D, x, thr) for thr in (0.0, THR)]
        _cases[shape] = dict(am=am0, x=x, carried=carried, deep=deep, y=[y0, y1], ref=refs, level=lv0,
                             level1=am1.carrier_level.copy(), present1=am1.carrier_present.copy(),
                             present0=am0.carrier_present.copy(), skip=am0.skip)
    return _cases[shape]


# ---------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_parity_with_definition(ld, shape):
    C, D, L, audio, carrier = shape
    cs = case(ld, shape)
    K = cs["x"].shape[1]
    assert cs["am"].ntaps == L and cs["skip"] == (-3) % D
    for thr, y, ref in zip((0.0, THR), cs["y"], cs["ref"]):
        assert y.dtype == np.float32 and y.shape == (C, -(-K // D))
        assert np.isfinite(y).all()
        assert not ref.edge.any(), int(ref.edge.sum())                     # no column is left out
        err = np.abs(y.astype(np.float64) - ref.y)
        full = ~ref.beyond                            # within full scale: the flat gate
        # every column of a row with a carrier whose window lies inside the stream is within full scale
        assert full[cs["carried"]][:, ref.steady[0]].all()
        top = np.max(np.where(full, np.abs(ref.y), 0.0), axis=1)
        rel = (np.max(np.where(full, err, 0.0), axis=1) / np.where(top > 0, top, 1.0))[cs["deep"]]
        over = err / ref.scale
        print(f"C={C} D={D} L={L} F={cs['am'].tile} thr={thr:g}: worst absolute {err[full].max():.3g} over the "
              f"{int(full.sum())} of {full.size} columns within full scale, relative to the row maximum there, index >= 0.3: "
              f"{rel.max():.3g}; beyond full scale (|y| up to {np.abs(ref.y).max():.3g}) worst {err[~full].max() if (~full).any() else 0:.3g} "
              f"absolute, {over[~full].max() if (~full).any() else 0:.3g} of the arithmetic's scale")
        assert err[full].max() <= GATE, (thr, float(err[full].max()))
        assert over.max() <= GATE, (thr, float(over.max()))


# ---------------------------------------------------------------- 2. zero and weak rows
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_zero_and_weak_rows(ld, shape):
    C, D, L, audio, carrier = shape
    cs = case(ld, shape)
    ref = cs["ref"][0]
    if C >= 4:
        for y in cs["y"]:
            assert (bits(y[1]) == 0).all()                                 # the zero row: +0.0, no NaN
    Cl = np.abs(ref.Cr[:, -1])
    for level in (cs["level"], cs["level1"]):
        assert level.dtype == np.float32 and level.shape == (C,)
        err = np.abs(level - Cl) / np.maximum(Cl, 0.01)
        print(f"C={C} D={D}: carrier level worst {err.max():.3g}, AM rows |Cr| {Cl[cs['carried']].min():.4f} .. "
              f"{Cl[cs['carried']].max():.4f}")
        assert err.max() <= 1e-6
    assert (bits(cs["level"]) == bits(cs["level1"])).all()                 # the level does not depend on the threshold
    assert cs["present1"].dtype == bool and cs["present1"][cs["carried"]].all()
    assert (Cl[cs["carried"]] >= 0.005).all()
    if C >= 4:
        assert not cs["present1"][1] and not cs["present0"][1] and cs["level"][1] == 0
    assert (cs["present0"] == (cs["level"] > 0)).all()


# ---------------------------------------------------------------- 3. recovery
def clean_rows(K, audio, carrier, L, offsets, A):
    rows = [am_row(3000 + 31 * i, K, audio, carrier, L, index=0.5, A=A, sigma=0.0, f0=f * carrier)
            for i, f in enumerate(offsets)]
    return np.stack([r[0] for r in rows]).astype(np.complex64), [r[1] for r in rows]


@pytest.mark.parametrize("C,D,L,audio,carrier,offsets", [(3, 5, 251, 0.1, 0.016, (0.0, 0.4, -0.4)),
                                                         (2, 4, 1001, 0.125, 0.004, (0.4, -0.4)),
                                                         (2, 4, 1001, 0.125, 0.004, (0.0, 0.4))])
def test_recovery(ld, C, D, L, audio, carrier, offsets):
    """Clean AM at index 0.5: after ceil(L / D) + 1 columns y is a(t - (L - 1) / 2) within 2e-3 (the float64
    definition measures 1.1e-4 to 5.5e-4), and the same stream at A = 1 and A = 0.01 gives outputs within 1e-6."""
    am = make(ld, C, D, L, audio, carrier)
    assert am.ntaps == L
    n0 = -(-L // D) + 1
    K = D * (n0 + 2 * am.tile + 1) + 3
    x1, mods = clean_rows(K, audio, carrier, L, offsets, 1.0)
    x2, _ = clean_rows(K, audio, carrier, L, offsets, 0.01)
    y1 = am(x1)
    am.reset()
    y2 = am(x2)
    tn = np.arange(y1.shape[1], dtype=np.float64) * D - (L - 1) / 2
    for c, a in enumerate(mods):
        want = a(tn)
        err = np.max(np.abs(y1[c, n0:] - want[n0:]))
        print(f"D={D} L={L} offset {offsets[c]:+.1f} carrier: recovery {err:.3g}, A = 1 against A = 0.01 "
              f"{np.max(np.abs(y1[c, n0:] - y2[c, n0:])):.3g}")
        assert np.max(np.abs(want[n0:])) > 0.3
        assert err <= 2e-3, (c, float(err))
    assert np.max(np.abs(y1[:, n0:].astype(np.float64) - y2[:, n0:])) <= 1e-6
    assert am.carrier_present.all()


# ---------------------------------------------------------------- 4. the same bits
def ragged_cuts(rng, K, D):
    """Ten call lengths that add up to K: 0, lengths below D (some below skip) and ragged ones."""
    lens = [0, 1, max(D - 2, 0), D, 0, D + 1] + [int(v) for v in rng.integers(0, 3 * D + 2, 3)]
    assert sum(lens) < K
    return lens + [K - sum(lens)]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_cuts_give_the_same_bits(ld, shape):
    C, D, L, audio, carrier = shape
    cs = case(ld, shape)
    x, y = cs["x"], cs["y"][0]
    cut = make(ld, *shape)
    lens = ragged_cuts(np.random.default_rng(40 + D), x.shape[1], D)
    assert len(lens) == 10
    parts, at = [], 0
    for n in lens:
        skip = cut.skip
        p = cut(x[:, at:at + n])
        assert p.shape == (C, (-(-(n - skip) // D)) if n > skip else 0)
        parts.append(p)
        at += n
    assert any(0 < n < D and p.shape[1] == 0 for n, p in zip(lens, parts)) or D <= 2
    assert (bits(np.concatenate(parts, axis=1)) == bits(y)).all()
    assert (bits(cut.carrier_level) == bits(cs["level"])).all()


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[4]], ids=[IDS[1], IDS[2], IDS[4]])
def test_rows_do_not_depend_on_the_bank(ld, shape):
    """A row's bits in a bank of 1, in a bank of another size with the rows in another order, and reversed."""
    C, D, L, audio, carrier = shape
    cs = case(ld, shape)
    x, y = cs["x"], cs["y"][0]
    for c in (0, C - 1):
        assert (bits(make(ld, 1, D, L, audio, carrier)(x[c:c + 1])) == bits(y[c:c + 1])).all()
    assert (bits(make(ld, *shape)(np.ascontiguousarray(x[::-1]))) == bits(y[::-1])).all()
    C2 = C + 3 if C < 100 else 7
    order = np.random.default_rng(C).permutation(max(C, C2))[:C2] % C
    assert (bits(make(ld, C2, D, L, audio, carrier)(np.ascontiguousarray(x[order]))) == bits(y[order])).all()


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_device_views_are_read_in_place(ld, shape):
    """A column slice of a wider device tensor whose rows start 8 bytes off a 16-byte boundary; a numpy call
    against a device call."""
    import torch
    C, D, L, audio, carrier = shape
    cs = case(ld, shape)
    x, y = cs["x"], cs["y"][0]
    K = x.shape[1]
    ldw = (K + 11) // 2 * 2
    wide = torch.full((C, ldw), float("nan"), dtype=torch.complex64, device="cuda")
    view = wide[:, 1:1 + K]
    view.copy_(torch.from_numpy(np.array(x)))
    assert view.data_ptr() % 16 == 8 and (ldw * 8) % 16 == 0 and not view.is_contiguous()
    yd = make(ld, *shape)(view)
    assert yd.is_cuda and yd.dtype == torch.float32 and tuple(yd.shape) == y.shape
    assert (bits(yd.cpu().numpy()) == bits(y)).all()                       # y came from a numpy call
    dense = make(ld, *shape)(torch.from_numpy(np.array(x)).cuda())
    assert (bits(dense.cpu().numpy()) == bits(y)).all()


def test_channelizer_output_and_audiobank_in_place(ld):
    """au(am(ch(x))): a Channelizer output and a row range of it read in place on the device, the AMBank's
    output read in place by an AudioBank, against the same calls through host memory."""
    import torch
    from conftest import cgauss
    C, D, N = 16, 4, 8 * (4 * (2 * 64 + 1) + 3)
    z = ld.Channelizer(C, 8)(torch.from_numpy(cgauss(np.random.default_rng(70), N)).cuda())
    assert z.is_cuda and z.shape[0] == C and z.is_contiguous()
    kw = dict(audio=0.125, carrier=4 / 180, ntaps=181)
    host = ld.AMBank(C, D, **kw)(z.cpu().numpy())
    yd = ld.AMBank(C, D, **kw)(z)
    assert yd.is_cuda and (bits(yd.cpu().numpy()) == bits(host)).all()
    part = ld.AMBank(5, D, **kw)(z[4:9])              # a row range
    assert (bits(part.cpu().numpy()) == bits(host[4:9])).all()
    cols = ld.AMBank(C, D, **kw)                      # a column range, twice
    a, b = cols(z[:, :203]), cols(z[:, 203:])
    assert not z[:, 203:].is_contiguous()
    assert (bits(torch.cat([a, b], dim=1).cpu().numpy()) == bits(host)).all()
    au_d = ld.AudioBank(C, 0.96, deemphasis=None)(yd)
    au_h = ld.AudioBank(C, 0.96, deemphasis=None)(host)
    assert au_d.is_cuda and au_d.shape[0] == C and au_d.shape[1] > 0
    assert (bits(au_d.cpu().numpy()) == bits(au_h)).all()
    au_r = ld.AudioBank(5, 0.96, deemphasis=None)(yd[4:9])
    assert (bits(au_r.cpu().numpy()) == bits(au_h[4:9])).all()


def test_set_threshold_between_calls(ld):
    """The columns after a set_threshold are those of a bank created with the new value and fed the
    same stream: the threshold touches no state."""
    shape = SHAPES[1]
    C, D, L, audio, carrier = shape
    cs = case(ld, shape)
    x, y = cs["x"], cs["y"][0]
    cut = 3 * D * 20 + 2
    a = make(ld, *shape)
    b = make(ld, *shape, threshold=2.0)               # above every carrier: silence
    assert a.threshold == 0.0 and b.threshold == 2.0
    ya0, yb0 = a(x[:, :cut]), b(x[:, :cut])
    assert (bits(ya0) == bits(y[:, :ya0.shape[1]])).all()
    assert (bits(yb0) == 0).all() and not b.carrier_present.any() and a.carrier_present.all()
    a.threshold = 2.0
    assert a.threshold == 2.0
    ya1, yb1 = a(x[:, cut:]), b(x[:, cut:])
    assert (bits(ya1) == bits(yb1)).all() and (bits(ya1) == 0).all()
    assert not a.carrier_present.any() and (bits(a.carrier_level) == bits(b.carrier_level)).all()
    assert (bits(a.carrier_level) == bits(cs["level"])).all()
    b.threshold = 0.0                                 # and back
    assert b.carrier_present.all()
    with pytest.raises(ValueError):
        a.threshold = -0.5


def test_reset(ld):
    shape = SHAPES[1]
    C, D, L, audio, carrier = shape
    cs = case(ld, shape)
    x, y = cs["x"], cs["y"][0]
    again = make(ld, *shape)
    again(x[:, :137])
    assert again.skip == (-137) % D and again.carrier_level[0] > 0
    again.reset()
    assert again.skip == 0 and (again.carrier_level == 0).all() and not again.carrier_present.any()
    assert (bits(again(x)) == bits(y)).all()
    assert (bits(again.carrier_level) == bits(cs["level"])).all()


# ---------------------------------------------------------------- 5. behind a squelch
def test_squelched_blocks_are_silent(ld):
    """am(sq(x)): row 0 is AM throughout, row 1 falls to -60 dB after 40 blocks and the SquelchBank closes it,
    row 2 is closed throughout.  Every column whose L-sample window lies wholly in zeroed samples is +0.0."""
    C, D, L, B = 3, 4, 181, 64
    audio, carrier = 0.125, 4 / 180
    K = 100 * B + 7
    x = np.stack([am_row(5000 + c, K, audio, carrier, L, A=0.5, sigma=0.01)[0] for c in range(C)])
    rng = np.random.default_rng(5005)
    quiet = 1e-3 * (rng.standard_normal((2, K)) + 1j * rng.standard_normal((2, K))) / np.sqrt(2)
    x[1, 40 * B:] = quiet[0, 40 * B:]
    x[2] = quiet[1]
    z = ld.SquelchBank(C, B, -20.0, 0.5, 2)(x.astype(np.complex64))
    assert z.shape == (C, 100 * B)
    zero = z == 0
    assert not zero[0, 10 * B:].any() and zero[2, 10 * B:].all() and not zero[1, 10 * B:40 * B].any() and zero[1, 60 * B:].all()
    am = make(ld, C, D, L, audio, carrier)
    y = am(z)
    before = np.concatenate([np.zeros((C, 1), np.int64), np.cumsum(zero, axis=1)], axis=1)   # zeroed samples before sample i
    n = np.arange(y.shape[1]) * D                     # the window of column n: samples nD - L + 1 .. nD, zeros before 0
    first = np.maximum(n - L + 1, 0)
    silent = (before[:, n + 1] - before[:, first]) == (n + 1 - first)[None, :]
    assert silent[2, 20 * B // D:].all() and silent[1].sum() > 30 * B // D and not silent[0, 20 * B // D:].any()
    assert (bits(y)[silent] == 0).all()
    assert (y[~silent] != 0).mean() > 0.99
    assert not am.carrier_present[1:].any() and am.carrier_present[0]
