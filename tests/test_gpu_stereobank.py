"""StereoBank on the GPU: the feed-forward FM stereo decoder over bank rows
(k_stbank.hip) against its definition (include/ldsp.h),

    s[c][n] = sum_{j<L} h[j] u[c][nD-j]
    z[c][n] = sum_{j<L} h[j] u[c][nD-j] exp(-2 pi i (((nD-j) 2w) mod 2^32) / 2^32)
    P[c][n] = sum_{j<L} g[j] u[c][nD-j] exp(-2 pi i (((nD-j)  w) mod 2^32) / 2^32)
    m = |P|^2,  S = m > thr^2 ? 2 Im(z conj(P)^2) / m : 0,  left = s + S,  right = s - S

evaluated here in float64 with the rotations the kernel leaves out, from the
object's own taps, pilot_taps and pilot word.  Rows are seeded multiplexes
0.45 (l + r) + 0.45 (l - r) sin 2 theta + 0.1 sin theta + noise with a different
pilot phase and ppm offset per row; where there is room row 1 is 0 throughout
and row 2 is noise without a pilot.  Sizes come from the kernel's tile (F output
columns per workgroup): one call of D (2F + 1) + 3 samples per row is two full
tiles, a one-column tile and a ragged tail.  The gate of 1e-6 per row is the
project's gate for FIR-class kernels.  Columns whose reference m
lies within 1e-4 (relative) of thr^2 may fall on either side of the float32
comparison and are left out, at most 1 % of a case's columns.  Streams cut into
calls, banks of other sizes and row orders, inputs read in place, a threshold
set between calls and reset() must give the same bits.

The phase near 2^32 has no test: the kernel applies no rotation, so nothing in
it depends on the stream position beyond skip (ldsp.h), and no seek hook exists."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GATE = 1e-6
PILOT = 0.076                                        # 19 kHz at 250 kHz
AP = 0.1                                             # the pilot's amplitude
THR = 0.01                                           # the default threshold
SHAPES = [(1, 1, 33), (3, 5, None), (16, 4, 181), (5, 8, 363), (128, 3, 65), (2, 32, 1025)]   # (C, D, L)


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def tones(rng, count):
    """A sum of `count` tones up to 14 kHz (0.056 cycles per sample) of peak at most 1, as a function of t."""
    f = rng.uniform(0.0004, 0.056, count)
    ph = rng.uniform(0.0, 1.0, count)
    a = rng.uniform(0.3, 1.0, count)
    a /= a.sum()
    return lambda t: (a[:, None] * np.sin(2 * np.pi * (f[:, None] * t[None, :] + ph[:, None]))).sum(axis=0)


def multiplex(seed, K, sigma):
    """One row in float64 over t = 0 .. K - 1, and its (l, r) as a function of t: 4 + 3 audio tones,
    a pilot up to 50 ppm off nominal at an arbitrary phase, white noise of deviation sigma."""
    rng = np.random.default_rng(seed)
    left, right = tones(rng, 4), tones(rng, 3)

    def lr(t):
        return left(t), right(t)

    t = np.arange(K, dtype=np.float64)
    l, r = lr(t)
    theta = 2 * np.pi * (PILOT * (1.0 + rng.uniform(-50e-6, 50e-6)) * t + rng.uniform(0.0, 1.0))
    u = 0.45 * (l + r) + 0.45 * (l - r) * np.sin(2 * theta) + AP * np.sin(theta)
    if sigma > 0:
        u = u + sigma * rng.standard_normal(K)
    return u, lr


def rows_for(seed, C, K, sigma=0.05):
    """float32 [C][K]: seeded multiplexes; where there is room row 1 is 0 throughout and row 2 noise
    of sigma 0.005 without a pilot.  Also the rows that carry a pilot."""
    x = np.stack([multiplex(seed + 31 * c, K, sigma * (0.2 + 0.8 * ((c * 7) % 5) / 4.0))[0] for c in range(C)])
    pilot = np.ones(C, bool)
    if C >= 2:
        x[1] = 0
        pilot[1] = False
    if C >= 3:
        x[2] = 0.005 * np.random.default_rng(seed + 5).standard_normal(K)
        pilot[2] = False
    return x.astype(np.float32), pilot


class Ref:
    """The definition in float64 over float32 rows x fed from t = T0 = 0, one threshold."""

    def __init__(self, sb, x, thr):
        x = np.asarray(x).astype(np.float64)
        h, g = sb.taps.astype(np.float64), sb.pilot_taps.astype(np.float64)
        w = int(round(sb.pilot * 2.0 ** 32))
        assert w == sb.word and w / 2.0 ** 32 == sb.pilot
        D, L, K = sb.decim, h.size, x.shape[1]
        ncols = -(-K // D)
        t = np.arange(ncols, dtype=np.int64)[:, None] * D - np.arange(L, dtype=np.int64)[None, :]   # [ncols][L]
        xp = np.concatenate([np.zeros((x.shape[0], L - 1)), x], axis=1)       # xp[:, t + L - 1] = x[:, t]
        U = xp[:, t + L - 1]                                                  # [C][ncols][L], 0 where t < 0
        ez = np.exp(-2j * np.pi * (np.mod(t * (2 * w), 2 ** 32) / 2.0 ** 32))
        ep = np.exp(-2j * np.pi * (np.mod(t * w, 2 ** 32) / 2.0 ** 32))
        self.s = np.einsum("cnl,l->cn", U, h)
        self.z = np.einsum("cnl,nl->cn", U, h[None, :] * ez)
        self.P = np.einsum("cnl,nl->cn", U, g[None, :] * ep)
        self.m = np.abs(self.P) ** 2
        thr2 = float(np.float32(thr) * np.float32(thr))
        self.on = self.m > thr2
        self.edge = np.abs(self.m - thr2) <= 1e-4 * thr2                      # either side in float32
        with np.errstate(divide="ignore", invalid="ignore"):
            S = np.where(self.on, 2.0 * np.imag(self.z * np.conj(self.P) ** 2) / self.m, 0.0)
        self.left, self.right = self.s + S, self.s - S


def worst(y, ref, keep):
    """Per-row max-norm error relative to the row maximum, over the columns kept."""
    den = np.max(np.abs(ref), axis=1)
    err = np.where(keep, np.abs(y - ref), 0.0)
    return np.max(err, axis=1) / np.where(den > 0, den, 1.0)


_cases = {}


def case(ld, C, D, L):
    """One call per shape, computed once and shared: (bank, x, pilot rows, y, reference)."""
    key = (C, D, L)
    if key not in _cases:
        sb = ld.StereoBank(C, PILOT, D, ntaps=L)
        K = D * (2 * sb.tile + 1) + 3
        x, pilot = rows_for(2000 + 7 * C + D, C, K)
        y = sb(x)
        level, stereo = sb.pilot_level.copy(), sb.stereo.copy()
        _cases[key] = (sb, x, pilot, y, Ref(sb, x, THR), level, stereo)
    return _cases[key]


# ---------------------------------------------------------------- 1. the definition
@pytest.mark.parametrize("C,D,L", SHAPES)
def test_parity_with_definition(ld, C, D, L):
    sb, x, pilot, y, ref, _, _ = case(ld, C, D, L)
    K = x.shape[1]
    assert y.dtype == np.float32 and y.shape == (C, 2, -(-K // D))
    assert len(sb.taps) == len(sb.pilot_taps) == (L or 225)
    assert np.isfinite(y).all()
    assert ref.edge.sum() <= 0.01 * ref.edge.size, int(ref.edge.sum())
    if C >= 3:
        assert np.abs(ref.P[2]).max() < THR / 2
    el, er = worst(y[:, 0], ref.left, ~ref.edge), worst(y[:, 1], ref.right, ~ref.edge)
    print(f"C={C} D={D} L={len(sb.taps)} F={sb.tile}: left worst row {int(np.argmax(el))} {el.max():.3g}, "
          f"right worst row {int(np.argmax(er))} {er.max():.3g}, {int(ref.edge.sum())} columns left out")
    assert el.max() <= GATE, (int(np.argmax(el)), float(el.max()))
    assert er.max() <= GATE, (int(np.argmax(er)), float(er.max()))


# ---------------------------------------------------------------- 2. the mono fallback
@pytest.mark.parametrize("C,D,L", SHAPES)
def test_mono_fallback_and_pilot_level(ld, C, D, L):
    sb, x, pilot, y, ref, level, stereo = case(ld, C, D, L)
    for c in np.flatnonzero(~pilot):
        assert not ref.on[c].any()
        assert (bits(y[c, 0]) == bits(y[c, 1])).all(), c                 # left and right: the same bits,
        assert worst(y[c:c + 1, 0], ref.s[c:c + 1], True)[0] <= GATE, c  # the definition's s
    if C >= 2:
        assert (bits(y[1]) == 0).all()                                   # the zero row: +0.0, no NaN
    # |P| of the last column: float32 sums of a_p / 2 = 0.05 at most; 1e-5 of that or of |P|
    Pl = np.abs(ref.P[:, -1])
    assert level.dtype == np.float32 and level.shape == (C,)
    err = np.abs(level - Pl) / np.maximum(Pl, AP / 2)
    print(f"C={C} D={D}: pilot level worst {err.max():.3g}, pilot rows |P| {Pl[pilot].min():.4f} .. {Pl[pilot].max():.4f}")
    assert err.max() <= 1e-5
    assert (np.abs(Pl - THR) > 1e-3 * THR).all()                         # no row sits on the threshold
    assert (stereo == (Pl > THR)).all()
    assert not stereo[~pilot].any()
    if (L or 225) >= 181:                                                # a prototype long enough to see the pilot alone
        assert stereo[pilot].all()


# ---------------------------------------------------------------- 3. separation
def test_separation(ld):
    """A clean multiplex: after ceil(L / D) + 1 columns left is 0.9 l and right 0.9 r, delayed by
    (L - 1) / 2 samples, within 2e-3 of the row maximum; the float64 definition measures 5e-4."""
    C, D = 3, 5
    sb = ld.StereoBank(C, PILOT, D)
    L = len(sb.taps)
    assert L == 225
    K = D * (2 * sb.tile + 1) + 3
    rows = [multiplex(3000 + 31 * c, K, 0.0) for c in range(C)]
    y = sb(np.stack([u for u, _ in rows]).astype(np.float32))
    n0 = -(-L // D) + 1
    tn = np.arange(y.shape[2], dtype=np.float64) * D - (L - 1) / 2
    for c, (_, lr) in enumerate(rows):
        l, r = lr(tn)
        for name, got, want in (("left", y[c, 0], 0.9 * l), ("right", y[c, 1], 0.9 * r)):
            err = np.max(np.abs(got[n0:] - want[n0:])) / np.max(np.abs(want[n0:]))
            print(f"row {c} {name}: {err:.3g}")
            assert err <= 2e-3, (c, name, float(err))
    assert sb.stereo.all()


# ---------------------------------------------------------------- 4. the same bits
def ragged_cuts(rng, K, D):
    """Ten call lengths that add up to K: 0, lengths below D (some below skip) and ragged ones."""
    lens = [0, 1, max(D - 2, 0), D, 0, D + 1] + [int(v) for v in rng.integers(0, 3 * D + 2, 3)]
    assert sum(lens) < K
    return lens + [K - sum(lens)]


@pytest.mark.parametrize("C,D,L", SHAPES)
def test_cuts_give_the_same_bits(ld, C, D, L):
    sb, x, pilot, y, ref, level, _ = case(ld, C, D, L)
    cut = ld.StereoBank(C, PILOT, D, ntaps=L)
    lens = ragged_cuts(np.random.default_rng(40 + D), x.shape[1], D)
    assert len(lens) == 10
    parts, at = [], 0
    for n in lens:
        skip = cut.skip
        p = cut(x[:, at:at + n])
        assert p.shape == (C, 2, (-(-(n - skip) // D)) if n > skip else 0)
        parts.append(p)
        at += n
    assert any(0 < n < D and p.shape[2] == 0 for n, p in zip(lens, parts)) or D <= 2
    assert (bits(np.concatenate(parts, axis=2)) == bits(y)).all()
    assert (bits(cut.pilot_level) == bits(level)).all()


@pytest.mark.parametrize("C,D,L", [(3, 5, None), (16, 4, 181), (128, 3, 65)])
def test_rows_do_not_depend_on_the_bank(ld, C, D, L):
    """A bank of another size, the rows in another order."""
    sb, x, pilot, y, ref, _, _ = case(ld, C, D, L)
    C2 = C + 3 if C < 100 else 7
    order = np.random.default_rng(C).permutation(max(C, C2))[:C2] % C
    other = ld.StereoBank(C2, PILOT, D, ntaps=L)
    y2 = other(np.ascontiguousarray(x[order]))
    assert (bits(y2) == bits(y[order])).all()


@pytest.mark.parametrize("C,D,L", [(3, 5, None), (5, 8, 363)])
def test_device_views_are_read_in_place(ld, C, D, L):
    """A column slice of a wider device tensor whose rows start 4 bytes off a 16-byte boundary."""
    import torch
    sb, x, pilot, y, ref, _, _ = case(ld, C, D, L)
    K = x.shape[1]
    ldw = (K + 11) // 4 * 4
    wide = torch.full((C, ldw), float("nan"), dtype=torch.float32, device="cuda")
    view = wide[:, 1:1 + K]
    view.copy_(torch.from_numpy(x))
    assert view.data_ptr() % 16 == 4 and (ldw * 4) % 16 == 0 and not view.is_contiguous()
    dev = ld.StereoBank(C, PILOT, D, ntaps=L)
    yd = dev(view)
    assert yd.is_cuda and yd.dtype == torch.float32 and tuple(yd.shape) == y.shape
    assert (bits(yd.cpu().numpy()) == bits(y)).all()
    assert (bits(yd.reshape(2 * C, -1).cpu().numpy()) == bits(y.reshape(2 * C, -1))).all()   # the AudioBank's view


def test_fmbank_output_is_read_in_place(ld):
    """au(st(fm(x))): an FMBank(C, kf, 1) output, and a column slice of it, on the device."""
    import torch
    from conftest import cgauss
    C, D, K = 4, 5, 5 * 131 + 2
    x = np.stack([cgauss(np.random.default_rng(70 + c), K) for c in range(C)])
    mpx = ld.FMBank(C, 0.3)(torch.from_numpy(x).cuda())
    assert mpx.is_cuda and tuple(mpx.shape) == (C, K)
    host = ld.StereoBank(C, PILOT, D)(mpx.cpu().numpy())
    dev = ld.StereoBank(C, PILOT, D)
    assert (bits(dev(mpx).cpu().numpy()) == bits(host)).all()
    cut = ld.StereoBank(C, PILOT, D)
    a, b = cut(mpx[:, :203]), cut(mpx[:, 203:])
    assert (bits(torch.cat([a, b], dim=2).cpu().numpy()) == bits(host)).all()
    au = ld.AudioBank(2 * C, 0.96, deemphasis=50e3)(dev(mpx).reshape(2 * C, -1))
    assert au.is_cuda and au.shape[0] == 2 * C


def test_set_threshold_between_calls(ld):
    """The columns after a set_threshold are those of a bank created with the new value and fed the
    same stream: the threshold touches no state."""
    C, D = 3, 5
    sb, x, pilot, y, ref, _, _ = case(ld, C, D, None)
    K = x.shape[1]
    cut = 3 * D * 20 + 2
    a = ld.StereoBank(C, PILOT, D)
    b = ld.StereoBank(C, PILOT, D, threshold=0.2)     # above every pilot: mono
    assert a.threshold == np.float32(0.01) and b.threshold == np.float32(0.2)
    ya0, yb0 = a(x[:, :cut]), b(x[:, :cut])
    assert (bits(ya0) == bits(y[:, :, :ya0.shape[2]])).all()
    assert (bits(yb0[:, 0]) == bits(yb0[:, 1])).all() and not b.stereo.any()
    a.threshold = 0.2
    assert a.threshold == np.float32(0.2)
    ya1, yb1 = a(x[:, cut:]), b(x[:, cut:])
    assert (bits(ya1) == bits(yb1)).all()
    assert not a.stereo.any() and (bits(a.pilot_level) == bits(b.pilot_level)).all()
    b.threshold = 0.01                                # and back
    assert b.stereo[0]
    with pytest.raises(ValueError):
        a.threshold = -0.5


def test_reset(ld):
    C, D = 3, 5
    sb, x, pilot, y, ref, level, _ = case(ld, C, D, None)
    again = ld.StereoBank(C, PILOT, D)
    again(x[:, :137])
    assert again.skip == (-137) % D and again.pilot_level[0] > 0
    again.reset()
    assert again.skip == 0 and (again.pilot_level == 0).all() and not again.stereo.any()
    assert (bits(again(x)) == bits(y)).all()
    assert (bits(again.pilot_level) == bits(level)).all()
