"""SquelchBank on the GPU: the per-row level and squelch gate over bank rows
(k_sqbank.hip) against its definition (include/ldsp.h),

    p[c][b] = (1/B) sum_{i<B} |x[c][bB + i]|^2
    s[c][b] = s[c][b-1] + alpha (p[c][b] - s[c][b-1]),  s[c][-1] = 0      (float64)
    level[c][b] = (float) s[c][b];   hi = level[c][b] > thr[c]            (float32)
    status[c][b] = liquid's agc squelch step from status[c][b-1] with hi, once per block
    y[c][bB + i] = status in {RISE, SIGNALHI, FALL, SIGNALLO} ? x[c][bB + i] : +0.0

restated here in numpy float64.  Rows are seeded noise at a -40 dB floor (a
different seed per row) plus constant-frequency tone bursts at 0 dB whose edges
fall on block boundaries; from five rows up one row is 0 throughout and one is
always above the threshold of -10 dB.  The bursts are laid out by a script of
"tone on until the level is above the threshold and k blocks more" / "tone off
until it is below and k blocks more" items (the level's inertia depends on the
bandwidth, so fixed block counts would not steer every shape through the
states), plus fixed runs: a one-block burst, a long burst, a one-block gap, gaps
shorter and longer than the timeout.  Rows start the script at three different
places so that the shortest calls (9 blocks of 4096) still see every state, and
repeat it to the end of the call.  What the tests need of these inputs -- every
code 1 .. 6, the edges FALL -> SIGNALHI and SIGNALLO -> SIGNALHI, the float64
level at least 1e-3 (relative) away from the threshold at every block -- is
asserted on the reference alone before anything is compared.  With timeout = 1
the step function leaves SIGNALLO for TIMEOUT at once, so SIGNALLO -> SIGNALHI
cannot occur and is asked for only where timeout >= 2.

Sizes come from the kernel's tile (T blocks per workgroup): one call of
B (2T + 1) + 3 samples per row is two full tiles, a one-block tile and a carried
tail.  The level gate of 1e-6 per row is the project's gate for this class of
kernel; status and the gated rows are compared exactly."""
import functools

import numpy as np
import pytest

from conftest import cgauss

pytestmark = pytest.mark.gpu

GATE = 1e-6
MARGIN = 1e-3
DB = -10.0
KF = 0.25
SHAPES = [(1, 16, 0.5, 3), (3, 100, 0.25, 4), (16, 1024, 1.0, 2), (256, 64, 0.25, 1), (5, 4096, 0.125, 2)]
ENABLED, RISE, SIGNALHI, FALL, SIGNALLO, TIMEOUT = 1, 2, 3, 4, 5, 6


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype != np.uint8 else a


def lin(dB):
    return np.array([np.float32(10.0 ** (float(v) / 10)) for v in np.atleast_1d(dB)], np.float32)


# ---------------------------------------------------------------- the inputs
def script(timeout):
    return [("burst", 0), ("gap", 0), ("burst", 0), ("gap", 1), ("burst", 0), ("gap", timeout + 1),
            ("on", 1), ("off", 1), ("on", 6), ("off", 1), ("burst", 1), ("gap", max(timeout - 1, 1)),
            ("burst", 0), ("gap", timeout + 2)]


def tone_blocks(nb, alpha, timeout, start, thr=10.0 ** (DB / 10), clear=0.02):
    """on[b] for nb blocks: the script from item `start` on, repeated.  The level that steers it is
    the nominal one (tone power 1, floor 1e-4); the noise moves a block's power by a few 1e-3 of
    it, so an item whose nominal level comes within `clear` of the threshold is put off by one
    more block of what came before it, until it stays clear."""
    def walk(s, run):
        near = 1.0
        for v in run:
            s += alpha * ((1.0001 if v else 1e-4) - s)
            near = min(near, abs(s - thr) / thr)
        return s, near

    def item(kind, k, s):
        if kind in ("on", "off"):
            return [kind == "on"] * k
        run, want = [], kind == "burst"
        while True:                                  # until the level has crossed, then k blocks more
            run.append(want)
            s, _ = walk(s, [want])
            if (s > thr) == want:
                return run + [want] * k

    items, on, s, i = script(timeout), [], 0.0, start
    while len(on) < nb:
        kind, k = items[i % len(items)]
        i += 1
        for extra in range(8):
            before = [on[-1] if on else False] * extra
            run = before + item(kind, k, walk(s, before)[0])
            after, near = walk(s, run)
            if near >= clear:
                break
        else:
            raise AssertionError("no clear layout")
        s = after
        on += run
    return np.array(on[:nb], bool)


def roles(C):
    """Row c is 'zero', 'high' (always above) or a burst row; the first two from five rows up."""
    r = ["burst"] * C
    if C >= 5:
        r[1], r[3] = "zero", "high"
    return r


@functools.lru_cache(maxsize=None)
def rows_for(C, B, alpha, timeout, nb, tail=3, seed=0):
    """(x, on): complex64 [C, nb B + tail], read-only, and the burst layout [C, nb]."""
    K = nb * B + tail
    x = np.empty((C, K), np.complex64)
    on = np.zeros((C, nb), bool)
    t = np.arange(K)
    nburst = 0
    for c, role in enumerate(roles(C)):
        if role == "zero":
            x[c] = 0
            continue
        if role == "high":
            on[c] = True
        else:
            on[c] = tone_blocks(nb, alpha, timeout, 2 * (nburst % 3))
            nburst += 1
        gate = np.concatenate([np.repeat(on[c], B), np.full(tail, on[c, -1])])
        f = 0.0371 + 0.0113 * (c % 17)
        tone = np.exp(2j * np.pi * ((f * t) % 1.0))
        x[c] = (cgauss(np.random.default_rng(9000 + seed + 17 * c), K, 1e-2).astype(np.complex128) + gate * tone)
    x.setflags(write=False)
    on.setflags(write=False)
    return x, on


# ---------------------------------------------------------------- the definition in numpy
def step_modes(mode, timer, hi, timeout):
    """agc_squelch_update_mode over rows: mode and timer are updated in place."""
    m = mode.copy()
    mode[m == ENABLED] = np.where(hi[m == ENABLED], RISE, ENABLED)
    up = (m == RISE) | (m == SIGNALHI)
    mode[up] = np.where(hi[up], SIGNALHI, FALL)
    f = m == FALL
    mode[f] = np.where(hi[f], SIGNALHI, SIGNALLO)
    timer[f] = timeout
    lo = m == SIGNALLO
    timer[lo] -= 1
    mode[lo] = np.where(timer[lo] == 0, TIMEOUT, np.where(hi[lo], SIGNALHI, SIGNALLO))
    mode[m == TIMEOUT] = ENABLED


def status_of(level32, thr32, timeout, mode=None, timer=None):
    """The state machine over float32 levels [C, nb] compared in float32."""
    C, nb = level32.shape
    mode = np.full(C, ENABLED) if mode is None else mode.copy()
    timer = np.zeros(C, np.int64) if timer is None else timer.copy()
    st = np.empty((C, nb), np.uint8)
    hi = level32 > np.asarray(thr32, np.float32).reshape(-1, 1)
    for b in range(nb):
        step_modes(mode, timer, hi[:, b], timeout)
        st[:, b] = mode
    return st


def definition(x, B, alpha, timeout, thr32):
    """(level float64 [C, nb], status uint8 [C, nb]) of a stream from reset."""
    C, K = x.shape
    nb = K // B
    xb = x[:, :nb * B]
    p = (xb.real.astype(np.float64) ** 2 + xb.imag.astype(np.float64) ** 2).reshape(C, nb, B).sum(axis=2) / B
    level = np.empty((C, nb))
    s = np.zeros(C)
    for b in range(nb):
        s = s + alpha * (p[:, b] - s)
        level[:, b] = s
    return level, status_of(level.astype(np.float32), thr32, timeout)


def is_open(st):
    return (st >= RISE) & (st <= SIGNALLO)


def gated(x, st, B):
    nb = st.shape[1]
    return np.where(np.repeat(is_open(st), B, axis=1), x[:, :nb * B], np.complex64(0))


def has_edge(st, a, b):
    return bool(((st[:, :-1] == a) & (st[:, 1:] == b)).any())


def check_inputs(level, st, thr32, timeout, burst):
    """What the comparisons need of the inputs, on the reference alone."""
    thr = np.asarray(thr32, np.float64).reshape(-1, 1)
    margin = np.abs(level - thr) / thr
    assert margin.min() >= MARGIN, float(margin.min())
    sb = st[burst]
    assert set(np.unique(sb)) == {1, 2, 3, 4, 5, 6}, np.unique(sb)
    assert has_edge(sb, FALL, SIGNALHI)
    assert has_edge(sb, SIGNALLO, SIGNALHI) == (timeout >= 2)     # unreachable with timeout = 1 (module docstring)


@functools.lru_cache(maxsize=None)
def case(ld_tile, C, B, alpha, timeout):
    """The single-call input of a shape, its reference and the burst rows; checked once."""
    nb = 2 * ld_tile + 1
    x, on = rows_for(C, B, alpha, timeout, nb)
    thr = lin([DB] * C)
    level, st = definition(x, B, alpha, timeout, thr)
    burst = np.array([r == "burst" for r in roles(C)])
    check_inputs(level, st, thr, timeout, burst)
    for a in (level, st):
        a.setflags(write=False)
    return x, level, st


def make(ld, C, B, alpha, timeout, threshold=DB):
    return ld.SquelchBank(C, B, threshold, alpha, timeout)


def per_row_err(y, ref):
    den = np.max(np.abs(ref), axis=1)
    return np.max(np.abs(y.astype(np.float64) - ref), axis=1) / np.where(den > 0, den, 1.0)


def test_inputs_cover_the_states():
    """The layout itself, without a device result: the five runs the issue names are in the script."""
    for C, B, alpha, timeout in SHAPES:
        on = tone_blocks(400, alpha, timeout, 0)
        runs = np.diff(np.flatnonzero(np.diff(np.concatenate([[~on[0]], on, [~on[-1]]]).astype(np.int8))))
        burst_runs, gap_runs = runs[0::2], runs[1::2]
        assert 1 in burst_runs and burst_runs.max() >= 6 and 1 in gap_runs
        assert gap_runs.max() > timeout


# ---------------------------------------------------------------- 1. level, 2. status
@pytest.mark.parametrize("C,B,alpha,timeout", SHAPES)
def test_level_and_status(ld, C, B, alpha, timeout):
    sq = make(ld, C, B, alpha, timeout)
    x, level, st = case(sq.tile, C, B, alpha, timeout)
    nb = level.shape[1]
    got_st, got_lv = sq.measure(x)
    assert got_st.dtype == np.uint8 and got_lv.dtype == np.float32 and got_st.shape == got_lv.shape == (C, nb)
    assert sq.fill == 3 and sq.status is got_st and sq.level is got_lv
    err = per_row_err(got_lv, level)
    print(f"C={C} B={B} alpha={alpha} T={sq.tile}: level worst row {int(np.argmax(err))} {err.max():.3g}")
    assert err.max() <= GATE, (int(np.argmax(err)), float(err.max()))
    # status is an exact function of the level returned and the thresholds compared against
    assert (got_st == status_of(got_lv, sq.threshold_linear, timeout)).all()
    assert (got_st == st).all()
    mode, timer, s = sq.state
    assert (mode == st[:, -1]).all() and (s.astype(np.float32) == got_lv[:, -1]).all()


# ---------------------------------------------------------------- 3. the gate
@pytest.mark.parametrize("C,B,alpha,timeout", SHAPES)
def test_gate_exact(ld, C, B, alpha, timeout):
    sq = make(ld, C, B, alpha, timeout)
    x, level, st = case(sq.tile, C, B, alpha, timeout)
    y = sq(x)
    assert y.dtype == np.complex64 and y.shape == (C, st.shape[1] * B)
    assert (sq.status == st).all()
    assert (bits(y) == bits(gated(x, st, B))).all()           # open: the input's bits; closed: +0.0


# ---------------------------------------------------------------- 4. cuts
@pytest.mark.parametrize("C,B,alpha,timeout", SHAPES)
def test_streaming_is_bitwise_invariant(ld, C, B, alpha, timeout):
    sq = make(ld, C, B, alpha, timeout)
    T = sq.tile
    lens = [0, 1, B - 1, B, B + 1, T * B - 1, 0, T * B, T * B + 1]
    nb = (sum(lens) + 2 * B + 3) // B
    x, _ = rows_for(C, B, alpha, timeout, nb, tail=7)
    K = x.shape[1]
    lens.append(K - sum(lens))
    whole = sq(x)
    w_st, w_lv = sq.status, sq.level
    assert whole.shape == (C, nb * B) and w_st.shape == (C, nb) and sq.fill == 7
    for parity in (0, 1):                            # measure and __call__ alternated, both ways round
        sq.reset()
        assert sq.fill == 0
        at = done = 0
        sts, lvs = [], []
        for i, n in enumerate(lens):
            want = sq.num_outputs(n)
            assert want == (at + n) // B - at // B
            part = x[:, at:at + n]
            if i % 2 == parity:
                st, lv = sq.measure(part)
            else:
                y = sq(part)
                st, lv = sq.status, sq.level
                assert y.shape == (C, want * B)
                assert (bits(y) == bits(whole[:, done * B:(done + want) * B])).all(), (parity, i)
            assert st.shape == lv.shape == (C, want), (n, st.shape, want)
            sts.append(st)
            lvs.append(lv)
            at += n
            done += want
            assert sq.fill == at % B
        assert (np.concatenate(sts, axis=1) == w_st).all()
        assert (bits(np.concatenate(lvs, axis=1)) == bits(w_lv)).all()


# ---------------------------------------------------------------- 5. rows are independent
def three(sq, x):
    y = sq(x)
    return y, sq.status, sq.level


def same_rows(got, want, rows_got, rows_want):
    for g, w in zip(got, want):
        g = g.cpu().numpy() if hasattr(g, "cpu") else g
        assert (bits(g[rows_got]) == bits(w[rows_want])).all()


def test_rows_are_independent(ld):
    C, B, alpha, timeout = 16, 1024, 1.0, 2
    sq = make(ld, C, B, alpha, timeout)
    x, level, st = case(sq.tile, C, B, alpha, timeout)
    want = three(sq, x)
    for r in (0, 1, 2, 3, 7, 15):
        same_rows(three(make(ld, 1, B, alpha, timeout), x[r:r + 1]), want, [0], [r])
        same_rows(three(make(ld, r + 1, B, alpha, timeout), x[r::-1]), want, [0], [r])   # rows r .. 0: r first
    same_rows(three(make(ld, C, B, alpha, timeout), x[::-1]), want, slice(None, None, -1), slice(None))
    same_rows(three(make(ld, 1, B, alpha, timeout), x[5]), want, [0], [5])            # 1-D when nchan is 1


def test_inputs_read_in_place(ld):
    import torch
    C, B, alpha, timeout = 3, 100, 0.25, 4
    sq = make(ld, C, B, alpha, timeout)
    x, level, st = case(sq.tile, C, B, alpha, timeout)
    K = x.shape[1]
    want = three(sq, x)
    # a column slice of a wider tensor: row stride above K, rows that start 8 bytes off a 16-byte boundary
    pad = rows_for(C, B, alpha, timeout, 1, tail=0, seed=500)[0]
    wide = torch.from_numpy(np.concatenate([pad[:, :7], x, pad[:, :5]], axis=1)).to("cuda:0")
    view = wide[:, 7:7 + K]
    assert view.stride() == (K + 12, 1) and not view.is_contiguous()
    sq.reset()
    got = three(sq, view)
    assert all(g.is_cuda for g in got)                        # device in, device out: all three
    assert got[0].dtype == torch.complex64 and got[1].dtype == torch.uint8 and got[2].dtype == torch.float32
    same_rows(got, want, slice(None), slice(None))
    sq.reset()
    st_d, lv_d = sq.measure(view.contiguous())
    assert st_d.is_cuda and lv_d.is_cuda
    same_rows((st_d, lv_d), want[1:], slice(None), slice(None))
    # a non-unit column stride is refused and leaves the state as it was
    sq.reset()
    with pytest.raises(ValueError):
        sq(wide[:, ::2][:, :K // 2])
    assert sq.fill == 0
    same_rows(three(sq, view), want, slice(None), slice(None))


def test_rows_of_a_channelizer_output_in_place(ld):
    import torch
    ch = ld.Channelizer(16, 8)
    n = 8 * 3000
    xs = cgauss(np.random.default_rng(5300), n, 0.05)
    xs[n // 3:2 * n // 3] += np.exp(2j * np.pi * ((3 / 16 + 0.004) * np.arange(n // 3))).astype(np.complex64) * 2
    rows = ch(torch.from_numpy(xs).to("cuda:0"))
    K = rows.shape[1]
    sl = rows[2:7]                                            # the tone's channel among them
    assert sl.data_ptr() != rows.data_ptr() and sl.stride(1) == 1
    a = three(make(ld, 5, 64, 0.5, 2), sl)
    b = three(make(ld, 5, 64, 0.5, 2), sl.clone())
    c = three(make(ld, 5, 64, 0.5, 2), sl.cpu().numpy())
    assert tuple(a[0].shape) == (5, K // 64 * 64) and a[0].is_cuda
    same_rows(a, [t.cpu().numpy() for t in b], slice(None), slice(None))
    same_rows(a, c, slice(None), slice(None))
    assert len(np.unique(c[1])) > 1                           # the squelch did open and close


# ---------------------------------------------------------------- 6. thresholds
def test_per_row_thresholds_and_the_setter(ld):
    C, B, alpha, timeout = 3, 100, 0.25, 4
    tile = make(ld, C, B, alpha, timeout).tile
    x, level, _ = case(tile, C, B, alpha, timeout)
    nb = level.shape[1]
    dB = np.array([-10.0, -3.5, -13.25])
    thr = lin(dB)
    assert (np.abs(level - thr[:, None].astype(np.float64)) / thr[:, None] >= MARGIN).all()
    sq = make(ld, C, B, alpha, timeout, dB)
    assert (bits(sq.threshold_linear) == bits(thr)).all()
    st, lv = sq.measure(x)
    assert (st == status_of(level.astype(np.float32), thr, timeout)).all()
    assert (st == status_of(lv, sq.threshold_linear, timeout)).all()
    assert not (st == case(tile, C, B, alpha, timeout)[2]).all()               # the thresholds do matter

    # a setter between two calls: the states change from the next block on, the level does not
    half = (nb // 2) * B + 5                                  # the second call starts inside a block
    sq = make(ld, C, B, alpha, timeout)
    st0, lv0 = sq.measure(x[:, :half])
    before = sq.state
    sq.threshold = dB
    after = sq.state
    assert all((a == b).all() for a, b in zip(before, after))                  # the setter touches no state
    st1, lv1 = sq.measure(x[:, half:])
    assert (bits(np.concatenate([lv0, lv1], axis=1)) == bits(lv)).all()
    n0 = st0.shape[1]
    base = lin([DB] * C)
    assert (st0 == status_of(lv0, base, timeout)).all()
    mode, timer = st0[:, -1].astype(np.int64), before[1].astype(np.int64)
    assert (st1 == status_of(lv1, thr, timeout, mode, timer)).all()
    assert not (st1 == status_of(lv[:, n0:], base, timeout, mode, timer)).all()

    # reset keeps the thresholds and restores the initial state: the first run's bits again
    sq.reset()
    assert (sq.threshold == dB).all()
    st2, lv2 = sq.measure(x)
    assert (st2 == st).all() and (bits(lv2) == bits(lv)).all()


# ---------------------------------------------------------------- 7. the receiver
@pytest.mark.parametrize("C,B,alpha,timeout", [(3, 100, 0.25, 4), (16, 1024, 1.0, 2)])
def test_squelched_discriminator(ld, C, B, alpha, timeout):
    sq = make(ld, C, B, alpha, timeout)
    x, level, st = case(sq.tile, C, B, alpha, timeout)
    nb = st.shape[1]
    plain = ld.FMBank(C, KF)(np.ascontiguousarray(x[:, :nb * B]))
    got = ld.FMBank(C, KF)(sq(x))
    assert got.shape == plain.shape == (C, nb * B)
    opn = np.repeat(is_open(st), B, axis=1)
    first = np.ones_like(opn)                                 # the first sample of a run of open or closed blocks
    first[:, 1:] = opn[:, 1:] != opn[:, :-1]
    closed, opened = ~opn & ~first, opn & ~first
    assert closed.any() and opened.any()
    assert (got[closed] == 0).all()                           # exactly 0
    assert (bits(got)[opened] == bits(plain)[opened]).all()
