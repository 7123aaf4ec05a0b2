"""AGCBank on the GPU against its definition (include/ldsp.h; tests/agcbank_model.py is the
numpy form).  Per case one uncut device call is the shared result: its peak_q against the
float64 definition (+-2 units: the device's double log2 against numpy's), its gain_q exactly
the numpy integer recurrence over the peak_q returned, its output within 1e-6 * target of the
float64 definition evaluated from the gain_q returned, and max |y| <= target (1 + 1e-6).  Then
steady tones, a long decay across every partition and pass of the track kernel, the same bits
from ragged calls, other banks, unaligned slices, an SSBBank output read in place and host
calls, containment of zeros and non-finite samples, and call order across streams.

Tolerances.  1e-6 is the project's parity gate.  The float32 evaluation of gamma and the
product round three times (g, gamma, the product: about 6e-8 each); the ceiling adds the
two-unit peak allowance (2 * 2^-24 octave = 8e-8)."""
import functools

import numpy as np
import pytest

import agcbank_model as M
from test_gpu_bank_streams import compare, fill, row_steps, streams  # noqa: F401  (fill, streams: fixtures)

pytestmark = pytest.mark.gpu

CASES = [(1, 16, 0, 0.5), (3, 100, 2, 0.25), (16, 256, 4, 0.1), (256, 64, 1, 3.0), (5, 4096, 3, 0.5)]
KINDS = [False, True]
IDS = [f"C{c}-B{b}-H{h}-d{d}" for c, b, h, d in CASES]
MAX_GAIN = 60.0


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


def targets_for(C):
    """One value for most banks, one per row for the three-row case."""
    return [-12.0, -6.0, -20.0] if C == 3 else -12.0


def target_lin(C):
    return (10.0 ** (np.atleast_1d(np.asarray(targets_for(C), np.float64)) / 20.0)).reshape(-1, 1)


def rows_for(seed, C, B, cplx, nblocks=40, extra=3):
    """A tone under an envelope that jumps between 1e-3 and 0.7 in mid-block, plus noise at 1e-5."""
    rng = np.random.default_rng(seed)
    n = B * nblocks + extra
    t = np.arange(n)
    x = np.empty((C, n), np.complex128)
    for c in range(C):
        env = np.empty(n)
        at, loud = 0, (c % 2 == 0)
        jumps = sorted(rng.choice(np.arange(1, nblocks), size=min(6, nblocks - 1), replace=False))
        for j in list(jumps) + [None]:
            end = n if j is None else j * B + B // 2 + int(rng.integers(-3, 4))
            env[at:end] = 0.7 if loud else 1e-3
            at, loud = end, not loud
        f, ph = rng.uniform(0.01, 0.2), rng.uniform(0, 1)
        x[c] = env * np.exp(2j * np.pi * (f * t + ph)) + 1e-5 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))
    return x.astype(np.complex64) if cplx else np.ascontiguousarray(x.real.astype(np.float32))


def make(ld, C, B, H, decay, cplx, target=None, max_gain=MAX_GAIN):
    return ld.AGCBank(C, B, targets_for(C) if target is None else target, max_gain, H, decay, cplx)


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()         # a copy: the shared inputs are read-only


def run(ag, x):
    """One call: (y, peak_q, gain_q) as numpy arrays."""
    y = ag(x)
    pq, gq = ag.peak_q, ag.gain_q
    return tuple(v.cpu().numpy() if hasattr(v, "is_cuda") else np.asarray(v) for v in (y, pq, gq))


def pieces(ag, xs):
    """The stream in calls: the concatenated (y, peak_q, gain_q)."""
    outs = [run(ag, x) for x in xs]
    return tuple(np.concatenate([o[i] for o in outs], axis=1) for i in range(3))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def same(got, want, what):
    for g, w, name in zip(got, want, ("y", "peak_q", "gain_q")):
        assert g.shape == w.shape and g.dtype == w.dtype, (what, name, g.shape, w.shape, g.dtype, w.dtype)
        assert np.array_equal(bits(g), bits(w)), (what, name)


@functools.lru_cache(maxsize=None)
def uncut(case, cplx):
    """The case's input and the result of one device call on a fresh bank; shared and left unchanged."""
    import liquiddsp as ld
    import torch
    C, B, H, decay = case
    x = rows_for(1000 + C + B, C, B, cplx)
    y, pq, gq = run(make(ld, C, B, H, decay, cplx), dev(torch, x))
    for a in (x, y, pq, gq):
        a.setflags(write=False)
    assert y.shape == (C, 39 * B) and pq.shape == gq.shape == (C, 40) and pq.dtype == gq.dtype == np.int32
    assert y.dtype == x.dtype
    return x, y, pq, gq


def amp(v):
    return np.abs(v)


# ---------------------------------------------------------------- the definition
@pytest.mark.parametrize("cplx", KINDS, ids=["real", "complex"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_peak(ld, torch, case, cplx):
    C, B, H, decay = case
    x, y, pq, gq = uncut(case, cplx)
    want = M.quantise(M.block_peaks(x, B))
    off = np.abs(pq.astype(np.int64) - want)
    print(f"peak_q: worst {int(off.max())} units, {int((off != 0).sum())} of {off.size} blocks differ")
    assert off.max() <= 2


@pytest.mark.parametrize("cplx", KINDS, ids=["real", "complex"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_tracker_exact(ld, torch, case, cplx):
    C, B, H, decay = case
    x, y, pq, gq = uncut(case, cplx)
    T = [M.units(t) for t in np.atleast_1d(targets_for(C))]
    want = M.gain_q(M.track_serial(pq, H, M.units(decay)), T, M.units(MAX_GAIN))
    assert np.array_equal(gq.astype(np.int64), want), int(np.argmax(gq != want))
    assert (np.diff(gq.astype(np.int64), axis=1) != 0).any()             # the gain moves


@pytest.mark.parametrize("cplx", KINDS, ids=["real", "complex"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_output_and_ceiling(ld, torch, case, cplx):
    C, B, H, decay = case
    x, y, pq, gq = uncut(case, cplx)
    tl = target_lin(C)
    want = M.apply(x, gq, B)
    err = (amp(y.astype(want.dtype) - want) / tl).max()
    top = (amp(y.astype(want.dtype)) / tl).max()
    print(f"output: worst |y - definition| = {err:.3g} of target; max |y| / target = 1 + {top - 1:.3g}")
    assert err <= 1e-6
    assert top <= 1 + 1e-6
    assert top > 0.5                                   # the loud stretches reach the target's neighbourhood


@pytest.mark.parametrize("cplx", KINDS, ids=["real", "complex"])
def test_steady_tones(ld, torch, cplx):
    """cos(2 pi t / 16) peaks at its amplitude in every block of 64: the peak sits at the target from block 0 on."""
    B, nb = 64, 12
    t = np.arange(B * nb) % 16                         # the same sixteen values in every block
    amps = np.array([1e-3, 0.1, 10.0])
    x = amps[:, None] * (np.exp(2j * np.pi * t / 16) if cplx else np.cos(2 * np.pi * t / 16))[None, :]
    x = x.astype(np.complex64 if cplx else np.float32)
    y, pq, gq = run(ld.AGCBank(3, B, -12.0, 60.0, 8, 0.5, cplx), dev(torch, x))
    tl = 10.0 ** (-12.0 / 20.0)
    peaks = amp(y.astype(np.complex128 if cplx else np.float64)).reshape(3, nb - 1, B).max(axis=2) / tl
    print("steady tones: peak / target - 1 between", peaks.min() - 1, "and", peaks.max() - 1)
    assert np.abs(peaks - 1).max() <= 1e-6
    assert (gq == gq[:, :1]).all()                     # one gain per row throughout


def test_long_decay_crosses_every_partition(ld, torch):
    """16 rows of 5 000 blocks: a burst in block 0, then noise at -100 dB, d = 0.01 dB, H = 255:
    three passes of the track kernel, every wave and lane boundary inside the decay."""
    C, B, nb, H, decay, mg = 16, 16, 5000, 255, 0.01, 40.0
    rng = np.random.default_rng(77)
    x = (1e-5 * rng.standard_normal((C, nb * B))).astype(np.float32)
    x[:, :B] = (10.0 ** (-np.arange(C) / 20.0))[:, None] * np.where(np.arange(B) % 2, -1.0, 1.0)[None, :]
    xd = dev(torch, x)
    y, pq, gq = run(ld.AGCBank(C, B, -12.0, mg, H, decay), xd)
    assert np.abs(pq.astype(np.int64) - M.quantise(M.block_peaks(x, B))).max() <= 2
    want = M.gain_q(M.track_serial(pq, H, M.units(decay)), M.units(-12.0), M.units(mg))
    assert np.array_equal(gq.astype(np.int64), want), int(np.argmax(gq != want))
    moving = (np.diff(want, axis=1) != 0).sum(axis=1)
    assert (moving > 2000).all() and (want[:, -1] == M.units(mg)).any() and (want[:, -1] < M.units(mg)).any()
    # the same stream with a pending block in front of a call of more than one pass
    ag = ld.AGCBank(C, B, -12.0, mg, H, decay)
    cut = B * 700 + 5
    same(pieces(ag, [xd[:, :cut], xd[:, cut:]]), (y, pq, gq), "two calls")


# ---------------------------------------------------------------- invariance
def ragged(B, n):
    """Ten calls: empty, one sample, B - 1, more than a block, several blocks, the rest."""
    lens = [0, 1, B - 1, 2 * B + 1, 0, B, 5 * B + B // 2, 1, 3 * B - 1]
    assert sum(lens) < n
    return lens + [n - sum(lens)]


@pytest.mark.parametrize("cplx", KINDS, ids=["real", "complex"])
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_ragged_calls(ld, torch, case, cplx):
    C, B, H, decay = case
    x, y, pq, gq = uncut(case, cplx)
    xd = dev(torch, x)
    ag = make(ld, C, B, H, decay, cplx)
    ends = np.cumsum(ragged(B, x.shape[1]))
    got = pieces(ag, [xd[:, a:b] for a, b in zip(np.concatenate([[0], ends[:-1]]), ends)])
    same(got, (y, pq, gq), "ragged")
    assert ag.fill == x.shape[1] - 39 * B
    ag.reset()                                         # and again from the start
    same(run(ag, xd), (y, pq, gq), "after reset")


@pytest.mark.parametrize("cplx", KINDS, ids=["real", "complex"])
def test_other_banks_and_row_orders(ld, torch, cplx):
    case = CASES[2]
    C, B, H, decay = case
    x, y, pq, gq = uncut(case, cplx)
    for rows in ([5], [15, 0, 7], list(range(15, -1, -1)), list(range(16)) * 16):
        got = run(ld.AGCBank(len(rows), B, -12.0, MAX_GAIN, H, decay, cplx), dev(torch, x[rows]))
        same(got, (y[rows], pq[rows], gq[rows]), rows[:3])
    # one target per row, in another order
    x3, y3, pq3, gq3 = uncut(CASES[1], cplx)
    rows, tg = [2, 0, 1], targets_for(3)
    got = run(ld.AGCBank(3, 100, [tg[r] for r in rows], MAX_GAIN, 2, 0.25, cplx), dev(torch, x3[rows]))
    same(got, (y3[rows], pq3[rows], gq3[rows]), "targets")


@pytest.mark.parametrize("cplx", KINDS, ids=["real", "complex"])
@pytest.mark.parametrize("case", [CASES[1], CASES[2], CASES[4]], ids=[IDS[1], IDS[2], IDS[4]])
def test_unaligned_slices_and_host_calls(ld, torch, case, cplx):
    C, B, H, decay = case
    x, y, pq, gq = uncut(case, cplx)
    n = x.shape[1]
    for lead, pad in ((1, 2), (3, 4), (1, 0)):
        wide = torch.zeros((C, lead + n + pad), dtype=torch.complex64 if cplx else torch.float32, device="cuda")
        wide[:, lead:lead + n] = dev(torch, x)
        view = wide[:, lead:lead + n]
        assert view.data_ptr() % 16 != 0 and not view.is_contiguous()
        same(run(make(ld, C, B, H, decay, cplx), view), (y, pq, gq), (lead, pad))
    ag = make(ld, C, B, H, decay, cplx)                # numpy in, numpy out, cut in two
    cut = 7 * B + 5
    got = pieces(ag, [np.ascontiguousarray(x[:, :cut]), np.ascontiguousarray(x[:, cut:])])
    assert isinstance(ag.peak_q, np.ndarray) and isinstance(ag.gain_db, np.ndarray)
    same(got, (y, pq, gq), "host")


def test_ssbbank_output_read_in_place(ld, torch):
    C, B = 16, 64
    rng = np.random.default_rng(5)
    env = np.repeat(rng.choice([1e-3, 0.5], size=(C, 24)), 400, axis=1)
    z = (env * (rng.standard_normal((C, 9600)) + 1j * rng.standard_normal((C, 9600)))).astype(np.complex64)
    a = ld.SSBBank(C, 2)(dev(torch, z))                # float32 [C, 4800]
    assert a.dtype == torch.float32 and a.shape == (C, 4800)
    ag = ld.AGCBank(C, B, hang=2)
    got = run(ag, a)
    xa = a.cpu().numpy()
    same(got, run(ld.AGCBank(C, B, hang=2), xa), "host copy")
    y, pq, gq = got
    assert np.abs(pq.astype(np.int64) - M.quantise(M.block_peaks(xa, B))).max() <= 2
    assert np.array_equal(gq, M.gain_q(M.track_serial(pq, 2, M.units(0.5)), M.units(-12.0), M.units(60.0)))
    tl = 10.0 ** (-12.0 / 20.0)
    assert np.abs(y - M.apply(xa, gq, B)).max() <= 1e-6 * tl and np.abs(y).max() <= tl * (1 + 1e-6)
    db = ag.gain_db
    assert db.dtype == torch.float32 and db.shape == gq.shape
    assert np.allclose(db.cpu().numpy(), gq * (M.DB_PER_OCTAVE / M.Q), rtol=0, atol=1e-5)
    au = ld.AudioBank(C, 0.96, deemphasis=None)(ag(a))           # the next stage reads the rows in place
    assert au.shape[0] == C and bool(torch.isfinite(au).all())


# ---------------------------------------------------------------- containment
@pytest.mark.parametrize("cplx", KINDS, ids=["real", "complex"])
def test_zero_rows(ld, torch, cplx):
    case = CASES[1]
    C, B, H, decay = case
    x = uncut(case, cplx)[0].copy()
    x[1] = 0
    ag = make(ld, C, B, H, decay, cplx)
    y, pq, gq = run(ag, dev(torch, x))
    assert not y[1].any() and not np.signbit(y[1].view(np.float32)).any() and np.isfinite(y).all()
    assert (pq[1] == M.FLOOR).all() and (gq[1] == M.units(MAX_GAIN)).all()
    db = ag.gain_db.cpu().numpy()
    assert db.dtype == np.float32 and (db[1] == np.float32(MAX_GAIN)).all() and np.isfinite(db).all()
    ref = uncut(case, cplx)
    same((y[[0, 2]], pq[[0, 2]], gq[[0, 2]]), tuple(v[[0, 2]] for v in ref[1:]), "other rows")


@pytest.mark.parametrize("cplx", KINDS, ids=["real", "complex"])
@pytest.mark.parametrize("case", [CASES[1], CASES[2]], ids=[IDS[1], IDS[2]])
def test_non_finite_samples_stay_where_they_are(ld, torch, case, cplx):
    C, B, H, decay = case
    x = uncut(case, cplx)[0].copy()
    spots = [(0, 3 * B + 7, np.nan), (C - 1, 10 * B, np.inf), (0, 20 * B + B - 1, -np.inf), (C - 1, 5, np.nan)]
    zeroed = x.copy()
    for r, t, v in spots:
        x[r, t] = v
        zeroed[r, t] = 0
    y, pq, gq = run(make(ld, C, B, H, decay, cplx), dev(torch, x))
    y0, pq0, gq0 = run(make(ld, C, B, H, decay, cplx), dev(torch, zeroed))
    mask = np.zeros(y.shape, bool)
    for r, t, v in spots:
        mask[r, t] = True
        assert not np.isfinite(y[r, t])
    assert np.isfinite(y[~mask]).all()
    assert np.array_equal(bits(y)[np.repeat(~mask, 2, axis=1) if cplx else ~mask],
                          bits(y0)[np.repeat(~mask, 2, axis=1) if cplx else ~mask])
    assert np.array_equal(pq, pq0) and np.array_equal(gq, gq0)


# ---------------------------------------------------------------- streams
@pytest.mark.parametrize("cplx", KINDS, ids=["real", "complex"])
def test_call_order_across_streams(ld, torch, fill, streams, cplx):  # noqa: F811
    """As tests/test_gpu_bank_streams.py for the other banks: calls on three streams in turn, some
    behind a filler, give the bits of the same calls on one stream, read-backs included."""
    C, B, H = 16, 256, 4
    lens = [33 * B + 3, B + 1, 0, 1, 2 * B + 5, 33 * B + B - 1, B - 1, 7]
    x = rows_for(9, C, B, cplx, nblocks=sum(lens) // B, extra=sum(lens) % B)
    mk = lambda: ld.AGCBank(C, B, -12.0, MAX_GAIN, H, 0.1, cplx)
    steps = row_steps(torch, x, lens)
    compare(torch, mk, steps, streams[:3], fill)
    read = ("read", lambda o: (o.peak_q, o.gain_q, o.gain_db, o.state, o.fill))
    compare(torch, mk, [steps[0], steps[1], steps[4], read], streams[:3], fill, plan=[(0, True), (1, True), (2, False)])
