"""SSBBank on the GPU: the tuned single-sideband demodulator over bank rows
(k_ssbbank.hip) against its definition (include/ldsp.h),

    S[c][n]  = sum_{j<L} g_c[j] x[c][nD-j]
    rot_c(n) = exp(-2 pi i ((((nD) mod 2^32) w_c) mod 2^32) / 2^32)
    y[c][n]  = Re(rot_c(n) S[c][n])

evaluated here in float64 from the object's own row_taps (complex64) and words,
the phase in exact integer arithmetic.  Rows are seeded single sideband,
x = A sum_k w_k exp(i s (2 pi f_k t + phi_k)) exp(2 pi i bfo t) + noise: A between
0.01 and 1, four tones f_k between 2 lo and hi - lo on the row's sideband s,
complex noise of deviation 0.01 A, the BFO drawn from [-0.5, 0.5) (row 0's is
exactly 0), the sidebands alternating.  Wherever C >= 4, row 1 is 0 throughout,
row 2 carries its tones on the opposite sideband only and row 3 is noise only.
Sizes come from the kernel's tile (F output columns per workgroup): one call of
D (2F + 1) + 3 samples per row is two full tiles, a ragged third and a non-zero
skip afterwards.

The gate of the parity test is the project's gate for FIR-class kernels, as in
test_gpu_downconverter.py: max |y - ref| / max |ref| <= 1e-6 per signal row.
The output of rows 2 and 3 is the residue of rejected content, and no float32
sum meets a gate against its own size; for them
|y - ref| <= 1e-6 max_n sum_j |g_c[j]| |x[nD - j]|, the arithmetic's scale.  The
zero row is +0.0 in every column.

Two properties of the definition follow from As = 60 dB (the float64
definition measures 5.1e-4 and 2.8e-4 at worst): on clean unit-sum tones, after
ceil(L / D) + 1 columns, y is within 2e-3 of m(nD - (L - 1) / 2), and with the
tones on the other sideband, from 0.2 lo upward, |y| <= 1e-3.

Streams cut into calls, banks of other sizes and row orders, inputs read in
place, reset(), a host-memory call, a retune between calls and a stream
position beyond 2^32 must give the same bits or, for the last, the same gate."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GATE = 1e-6
# (C, D, L, lo, hi)
SHAPES = [(1, 1, 33, 0.0625, 0.4), (3, 2, 81, 0.025, 0.225), (16, 4, 201, 0.01, 0.1), (5, 5, 501, 0.004, 0.1),
          (256, 3, 65, 1 / 32, 0.16), (2, 32, 1025, 1 / 512, 0.015)]
IDS = [f"{s[0]}-{s[1]}-{s[2]}" for s in SHAPES]
NAMES = {1: "usb", -1: "lsb"}


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def make(ld, shape, bfo, side, C=None):
    C_, D, L, lo, hi = shape
    return ld.SSBBank(C_ if C is None else C, D, lo=lo, hi=hi, bfo=bfo, sideband=[NAMES[int(s)] for s in side], ntaps=L)


def tones(rng, f_lo, f_hi, n=4):
    """n unit-sum tones: frequencies, phases (turns), weights; and m(t) = sum w cos(2 pi (f t + ph))."""
    f, ph, w = rng.uniform(f_lo, f_hi, n), rng.uniform(0.0, 1.0, n), rng.uniform(0.3, 1.0, n)
    w /= w.sum()

    def m(t):
        return (w[:, None] * np.cos(2 * np.pi * (f[:, None] * t[None, :] + ph[:, None]))).sum(axis=0)

    return f, ph, w, m


def ssb_row(K, bfo, s, A, f, ph, w, t0=0):
    """A (m(t) + i s m^(t)) exp(2 pi i bfo t) over t = t0 .. t0 + K - 1, complex128."""
    t = np.arange(K, dtype=np.float64) + float(t0 % (1 << 20))            # the tones' phases are arbitrary anyway
    tb = (np.arange(K, dtype=np.int64) + int(t0)).astype(np.float64)      # t < 2^53: exact
    a = (w[:, None] * np.exp(1j * s * 2 * np.pi * (f[:, None] * t[None, :] + ph[:, None]))).sum(axis=0)
    return A * a * np.exp(2j * np.pi * np.mod(bfo * tb, 1.0))


def lists_for(seed, C):
    rng = np.random.default_rng(seed)
    bfo = rng.uniform(-0.5, 0.5, C)
    bfo[0] = 0.0
    side = np.where(np.arange(C) % 2 == 0, 1, -1)
    return bfo, side


def rows_for(seed, C, K, lo, hi, bfo, side):
    """complex64 [C][K] (read-only) and the rows that carry a signal on their own sideband."""
    x = np.empty((C, K), np.complex128)
    signal = np.ones(C, bool)
    for c in range(C):
        rng = np.random.default_rng(seed + 31 * c)
        A = 10.0 ** rng.uniform(-2.0, 0.0)
        f, ph, w, _ = tones(rng, 2 * lo, hi - lo)
        s = side[c]
        noise = 0.01 * A * (rng.standard_normal(K) + 1j * rng.standard_normal(K)) / np.sqrt(2)
        if C >= 4 and c == 1:
            x[c] = 0
        elif C >= 4 and c == 2:
            x[c] = ssb_row(K, bfo[c], -s, A, f, ph, w) + noise
        elif C >= 4 and c == 3:
            x[c] = noise
        else:
            x[c] = ssb_row(K, bfo[c], s, A, f, ph, w) + noise
    if C >= 4:
        signal[[1, 2, 3]] = False
    x = x.astype(np.complex64)
    x.setflags(write=False)
    return x, signal


class Ref:
    """The definition in float64 over complex64 rows x fed from stream position T (zeros before it)."""

    def __init__(self, g, words, D, x, T=0):
        x = np.asarray(x).astype(np.complex128)
        g = np.asarray(g).astype(np.complex128)
        C, K = x.shape
        L = g.shape[1]
        n = np.arange(-(-T // D), -(-(T + K) // D), dtype=np.int64)       # absolute column indices
        at = (n * D - T)[:, None] - np.arange(L, dtype=np.int64)[None, :]  # [ncols][L], >= -(L - 1)
        xp = np.concatenate([np.zeros((C, L - 1), np.complex128), x], axis=1)
        low = ((n * D) & 0xFFFFFFFF).astype(np.uint64)
        self.y = np.empty((C, n.size))
        self.scale = np.empty((C, n.size))
        for c in range(C):                            # row by row: [ncols][L] at a time
            U = xp[c][at + L - 1]
            S = U @ g[c]
            ph = (low * np.uint64(words[c])) & np.uint64(0xFFFFFFFF)       # exact: both factors below 2^32
            rot = np.exp(-2j * np.pi * (ph.astype(np.float64) / 4294967296.0))
            self.y[c] = np.real(rot * S)
            self.scale[c] = np.abs(U) @ np.abs(g[c])


def gate_rows(y, ref, signal):
    """Worst figure of the signal rows (against the row's largest output) and of the others (against the
    arithmetic's scale); both must be <= GATE."""
    err = np.abs(y.astype(np.float64) - ref.y)
    rel = err[signal].max(axis=1) / np.abs(ref.y[signal]).max(axis=1) if signal.any() else np.zeros(1)
    rest = ~signal & (ref.scale.max(axis=1) > 0)
    res = err[rest].max(axis=1) / ref.scale[rest].max(axis=1) if rest.any() else np.zeros(1)
    return float(rel.max()), float(res.max())


_cases = {}


def case(ld, shape):
    """One call per shape, computed once and shared."""
    if shape not in _cases:
        C, D, L, lo, hi = shape
        bfo, side = lists_for(900 + C + D, C)
        sb = make(ld, shape, bfo, side)
        K = D * (2 * sb.tile + 1) + 3
        x, signal = rows_for(2000 + 7 * C + D, C, K, lo, hi, bfo, side)
        y = sb(x)
        _cases[shape] = dict(sb=sb, x=x, bfo=bfo, side=side, signal=signal, y=y, skip=sb.skip,
                             ref=Ref(sb.row_taps, sb.words, D, x))
    return _cases[shape]


# ---------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_parity_with_definition(ld, shape):
    C, D, L, lo, hi = shape
    cs = case(ld, shape)
    y, ref, K = cs["y"], cs["ref"], cs["x"].shape[1]
    assert cs["sb"].ntaps == L and cs["skip"] == (-3) % D and cs["sb"].words[0] == 0
    assert y.dtype == np.float32 and y.shape == (C, -(-K // D)) == ref.y.shape
    assert np.isfinite(y).all()
    rel, res = gate_rows(y, ref, cs["signal"])
    print(f"C={C} D={D} L={L} F={cs['sb'].tile}: signal rows worst {rel:.3g} of the row maximum, "
          f"residue rows worst {res:.3g} of the arithmetic's scale")
    assert rel <= GATE and res <= GATE, (rel, res)
    if C >= 4:
        assert (bits(y[1]) == 0).all()                # the zero row: +0.0
        top = np.abs(ref.y).max(axis=1)
        print(f"  opposite-sideband row {top[2]:.3g}, noise row {top[3]:.3g}, signal rows {top[cs['signal']].min():.3g} "
              f".. {top[cs['signal']].max():.3g}")


# ---------------------------------------------------------------- 2. properties of the definition
@pytest.mark.parametrize("C,D,L,lo,hi", [(3, 2, 81, 0.025, 0.225), (2, 4, 1001, 0.002, 0.06)])
def test_recovery_and_rejection(ld, C, D, L, lo, hi):
    """Clean unit-sum tones: after ceil(L / D) + 1 columns y is m(nD - (L - 1) / 2) within 2e-3; the same
    kind of tones on the other sideband, from 0.2 lo upward, give |y| <= 1e-3."""
    shape = (C, D, L, lo, hi)
    bfo, side = np.array([0.0, 0.3, -0.05])[:C], np.array([1, -1, -1])[:C]
    sb = make(ld, shape, bfo, side)
    assert sb.ntaps == L
    n0 = -(-L // D) + 1
    K = D * (n0 + 2 * sb.tile + 1) + 3
    bfo_w = sb.words.astype(np.int64).astype(np.int32).astype(np.float64) / 4294967296.0   # the BFOs the words stand for
    on, off, mods = [], [], []
    for c in range(C):
        rng = np.random.default_rng(3000 + 31 * c)
        f, ph, w, m = tones(rng, 2 * lo, hi - lo)
        on.append(ssb_row(K, bfo_w[c], side[c], 1.0, f, ph, w))
        mods.append(m)
        f, ph, w, _ = tones(rng, 0.2 * lo, hi - lo)
        off.append(ssb_row(K, bfo_w[c], -side[c], 1.0, f, ph, w))
    y_on = sb(np.stack(on).astype(np.complex64))
    sb.reset()
    y_off = sb(np.stack(off).astype(np.complex64))
    tn = np.arange(y_on.shape[1], dtype=np.float64) * D - (L - 1) / 2
    for c, m in enumerate(mods):
        want = m(tn)
        err = np.max(np.abs(y_on[c, n0:] - want[n0:]))
        leak = np.max(np.abs(y_off[c, n0:]))
        print(f"D={D} L={L} bfo {bfo[c]:+.2f} {NAMES[side[c]]}: recovery {err:.3g}, other sideband {leak:.3g}")
        assert np.max(np.abs(want[n0:])) > 0.3
        assert err <= 2e-3, (c, float(err))
        assert leak <= 1e-3, (c, float(leak))


# ---------------------------------------------------------------- 3. the same bits
def ragged_cuts(rng, K, D):
    """Ten call lengths that add up to K: 0, lengths below D (some below skip) and ragged ones."""
    lens = [0, 1, max(D - 2, 0), D, 0, D + 1] + [int(v) for v in rng.integers(0, 3 * D + 2, 3)]
    assert sum(lens) < K
    return lens + [K - sum(lens)]


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_cuts_give_the_same_bits(ld, shape):
    C, D, L, lo, hi = shape
    cs = case(ld, shape)
    x, y = cs["x"], cs["y"]
    cut = make(ld, shape, cs["bfo"], cs["side"])
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


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2], SHAPES[4]], ids=[IDS[1], IDS[2], IDS[4]])
def test_rows_do_not_depend_on_the_bank(ld, shape):
    """A row's bits in a bank of 1, in a bank of another size with the rows in another order, and reversed."""
    C, D, L, lo, hi = shape
    cs = case(ld, shape)
    x, y, bfo, side = cs["x"], cs["y"], cs["bfo"], cs["side"]
    for c in (0, C - 1):
        assert (bits(make(ld, shape, bfo[c:c + 1], side[c:c + 1], C=1)(x[c:c + 1])) == bits(y[c:c + 1])).all()
    assert (bits(make(ld, shape, bfo[::-1], side[::-1])(np.ascontiguousarray(x[::-1]))) == bits(y[::-1])).all()
    C2 = C + 3 if C < 100 else 7
    order = np.random.default_rng(C).permutation(max(C, C2))[:C2] % C
    got = make(ld, shape, bfo[order], side[order], C=C2)(np.ascontiguousarray(x[order]))
    assert (bits(got) == bits(y[order])).all()


@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[3]], ids=[IDS[1], IDS[3]])
def test_device_views_are_read_in_place(ld, shape):
    """A column slice of a wider device tensor whose rows start 8 bytes off a 16-byte boundary; a numpy call
    against a device call."""
    import torch
    C, D, L, lo, hi = shape
    cs = case(ld, shape)
    x, y = cs["x"], cs["y"]
    K = x.shape[1]
    ldw = (K + 11) // 2 * 2
    wide = torch.full((C, ldw), float("nan"), dtype=torch.complex64, device="cuda")
    view = wide[:, 1:1 + K]
    view.copy_(torch.from_numpy(np.array(x)))
    assert view.data_ptr() % 16 == 8 and (ldw * 8) % 16 == 0 and not view.is_contiguous()
    yd = make(ld, shape, cs["bfo"], cs["side"])(view)
    assert yd.is_cuda and yd.dtype == torch.float32 and tuple(yd.shape) == y.shape
    assert (bits(yd.cpu().numpy()) == bits(y)).all()                       # y came from a numpy call
    dense = make(ld, shape, cs["bfo"], cs["side"])(torch.from_numpy(np.array(x)).cuda())
    assert (bits(dense.cpu().numpy()) == bits(y)).all()


def test_channelizer_output_and_audiobank_in_place(ld):
    """au(ssb(ch(x))): a Channelizer output and a row range of it read in place on the device, the SSBBank's
    output read in place by an AudioBank, against the same calls through host memory."""
    import torch
    from conftest import cgauss
    C, D, N = 16, 4, 8 * (4 * (2 * 64 + 1) + 3)
    z = ld.Channelizer(C, 8)(torch.from_numpy(cgauss(np.random.default_rng(70), N)).cuda())
    assert z.is_cuda and z.shape[0] == C and z.is_contiguous()
    bfo, side = lists_for(71, C)
    shape = (C, D, 201, 0.01, 0.1)
    host = make(ld, shape, bfo, side)(z.cpu().numpy())
    assert np.abs(host).max() > 0
    yd = make(ld, shape, bfo, side)(z)
    assert yd.is_cuda and (bits(yd.cpu().numpy()) == bits(host)).all()
    part = make(ld, shape, bfo[4:9], side[4:9], C=5)(z[4:9])               # a row range
    assert (bits(part.cpu().numpy()) == bits(host[4:9])).all()
    cols = make(ld, shape, bfo, side)                 # a column range, twice
    a, b = cols(z[:, :203]), cols(z[:, 203:])
    assert not z[:, 203:].is_contiguous()
    assert (bits(torch.cat([a, b], dim=1).cpu().numpy()) == bits(host)).all()
    both = make(ld, shape, bfo[4:9], side[4:9], C=5)  # a row and a column range at once
    a, b = both(z[4:9, :203]), both(z[4:9, 203:])
    assert (bits(torch.cat([a, b], dim=1).cpu().numpy()) == bits(host[4:9])).all()
    au_d = ld.AudioBank(C, 0.96, deemphasis=None)(yd)
    au_h = ld.AudioBank(C, 0.96, deemphasis=None)(host)
    assert au_d.is_cuda and au_d.shape[0] == C and au_d.shape[1] > 0
    assert (bits(au_d.cpu().numpy()) == bits(au_h)).all()
    au_r = ld.AudioBank(5, 0.96, deemphasis=None)(yd[4:9])
    assert (bits(au_r.cpu().numpy()) == bits(au_h[4:9])).all()


def test_reset(ld):
    shape = SHAPES[1]
    C, D, L, lo, hi = shape
    cs = case(ld, shape)
    x, y = cs["x"], cs["y"]
    again = make(ld, shape, cs["bfo"], cs["side"])
    again(x[:, :137])
    assert again.skip == (-137) % D
    again.reset()
    assert again.skip == 0
    assert (bits(again(x)) == bits(y)).all()


# ---------------------------------------------------------------- 4. retuning between calls
@pytest.mark.parametrize("shape", [SHAPES[1], SHAPES[2]], ids=[IDS[1], IDS[2]])
def test_retune_between_calls(ld, shape):
    """bfo and sideband set between two calls: the second call's columns are, bitwise, those of a bank created
    with the new lists and fed the whole stream (the history is raw input)."""
    C, D, L, lo, hi = shape
    cs = case(ld, shape)
    x = cs["x"]
    bfo2, side2 = lists_for(77 + C, C)
    bfo2[0], side2 = 0.123456789, -cs["side"]
    assert not np.array_equal(bfo2, cs["bfo"])
    cut = D * 40 + 1
    a = make(ld, shape, cs["bfo"], cs["side"])
    y0 = a(x[:, :cut])
    assert (bits(y0) == bits(cs["y"][:, :y0.shape[1]])).all()
    a.bfo = bfo2
    a.sideband = [NAMES[int(s)] for s in side2]
    y1 = a(x[:, cut:])
    fresh = make(ld, shape, bfo2, side2)
    whole = fresh(x)
    assert y0.shape[1] + y1.shape[1] == whole.shape[1]
    assert (bits(y1) == bits(whole[:, y0.shape[1]:])).all()
    assert (bits(a.row_taps) == bits(fresh.row_taps)).all() and (a.words == fresh.words).all()
    signal = cs["signal"] | (np.arange(C) == 2)       # with the sidebands swapped, row 2 is the signal row
    diff = bits(y1) != bits(cs["y"][:, y0.shape[1]:])
    assert diff[signal].mean() > 0.9                  # and the retune did change the output


# ---------------------------------------------------------------- 5. the phase beyond 2^32
@pytest.mark.parametrize("where", ["wrap", "far"])
def test_phase_at_large_stream_positions(ld, where):
    """_seek(T) at T = 2^32 - D (F + 1) - 1 (the sample index passes 2^32 inside the call's second tile) and at
    T = 3 2^32 + 5, BFOs off every coarse grid: parity at the parity test's gate, which a rotation from a
    truncated or rounded column index or word would miss."""
    shape = SHAPES[1]
    C, D, L, lo, hi = shape
    bfo, side = np.array([0.0, 0.123456789, -0.3141592653589793]), np.array([1, -1, 1])
    sb = make(ld, shape, bfo, side)
    F = sb.tile
    T = (1 << 32) - D * (F + 1) - 1 if where == "wrap" else 3 * (1 << 32) + 5
    K = D * (2 * F + 1) + 3
    bfo_w = sb.words.astype(np.int64).astype(np.int32).astype(np.float64) / 4294967296.0
    rows = []
    for c in range(C):
        rng = np.random.default_rng(4000 + c)
        f, ph, w, _ = tones(rng, 2 * lo, hi - lo)
        rows.append(ssb_row(K, bfo_w[c], side[c], 0.5, f, ph, w, t0=T))
    x = np.stack(rows).astype(np.complex64)
    sb._seek(T)
    assert sb.skip == (-T) % D
    y = sb(x)
    ref = Ref(sb.row_taps, sb.words, D, x, T=T)
    assert y.shape == ref.y.shape
    rel, _ = gate_rows(y, ref, np.ones(C, bool))
    first = Ref(sb.row_taps, sb.words, D, x, T=T % D)                      # the same rows at the stream's start
    away = np.abs(first.y - ref.y).max(axis=1) / np.abs(ref.y).max(axis=1)
    print(f"T={T}: worst {rel:.3g} of the row maximum; the rotation of position T mod D would be off by {away[1:].max():.3g}")
    assert rel <= GATE
    assert away[1:].min() > 1e-3                      # the position matters for every row with a BFO
    sb.reset()
    assert sb.skip == 0
