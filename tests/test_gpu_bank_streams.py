"""Call order of the bank objects across streams: Channelizer, Synthesizer,
Downconverter, FMBank, AudioBank, SquelchBank, StereoBank and Spectrogram keep
their calls in call order whichever stream each call is made on
(ldsp_common.hpp, StreamMark), host-memory calls on the library's own stream
included, and their setters, resets and read-backs see the last call.

The reference of every test is the same class fed the same pieces on one
stream; the objects' own suites tie that to the float64 definitions and to the
uncut call.  Every comparison is bitwise.

The race is made certain with a filler: in-place elementwise torch operations on
one large device tensor, enqueued on a stream in front of the object's call, keep
that stream busy for several milliseconds (measured with timing events and
asserted to be at least 5 ms after the final synchronize; the repetition count
is calibrated once per module and printed).  The next call, made at once on
another stream and behind no filler, would run first if the object did not
order it, and would then read the other half of a ping-pong pair or a scratch
buffer the call before it has not written yet.  An object's first call binds it
to the device, which waits for the device, so a filler in front of it holds
nothing back: every sequence below has a filler in front of a later call too.

Sizes are one tile of the object's kernel plus a ragged tail for the first
piece (the grow-only scratch buffers reach their size there; regrowing one waits
for the device), then short pieces: an empty one, one shorter than skip where
the object has a skip, ragged ones."""
import contextlib
import math

import numpy as np
import pytest

from conftest import cgauss
from test_gpu_audiobank import rows_for as audio_rows
from test_gpu_downconverter import freqs_for
from test_gpu_fmbank import KF, rows_for as fm_rows
from test_gpu_ingest import raw_iq
from test_gpu_spectrogram import make as make_spgram, signal
from test_gpu_squelchbank import rows_for as squelch_rows
from test_gpu_stereobank import PILOT, rows_for as stereo_rows
from test_gpu_synthesizer import cgauss2

pytestmark = pytest.mark.gpu

FLOOR_MS = 5.0                                        # a filler shorter than this held nothing back


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


class Filler:
    """fill() keeps the current stream busy for about twice FLOOR_MS; check(), after a
    synchronize, asserts that every filler since the last check took at least FLOOR_MS."""

    def __init__(self, torch):
        self.torch = torch
        self.buf = torch.ones(1 << 26, dtype=torch.float32, device="cuda")    # 256 MiB read and written per pass
        self.pending = []
        self.reps = 8
        for _ in range(8):                            # the clocks come up during the first of them
            self()
        torch.cuda.synchronize()
        best = min(a.elapsed_time(b) for a, b in self.pending)    # the fastest passes ask for the most of them
        self.pending.clear()
        self.reps = max(8, math.ceil(8 * 2 * FLOOR_MS / best))
        print(f"filler: 8 passes took {best:.3f} ms at best, {self.reps} passes per filler")

    def __call__(self):
        ev = [self.torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        for _ in range(self.reps):
            self.buf.neg_()
        ev[1].record()
        self.pending.append(ev)

    def check(self):
        ms = [a.elapsed_time(b) for a, b in self.pending]
        self.pending.clear()
        print("fillers (ms): " + " ".join(f"{m:.2f}" for m in ms))
        assert ms and min(ms) >= FLOOR_MS, f"precondition failed: a filler took {min(ms):.2f} ms, below {FLOOR_MS} ms"
        return ms


@pytest.fixture(scope="module")
def fill(torch):
    return Filler(torch)


@pytest.fixture(scope="module")
def streams(torch):
    return [torch.cuda.Stream() for _ in range(4)]


# ---------------------------------------------------------------- comparing
def bits(a):
    a = np.ascontiguousarray(np.atleast_1d(a))
    return a.view(np.uint8) if a.dtype.itemsize % 4 else a.view(np.uint32)


def host(v):
    """Tensors as numpy arrays, tuples kept; on the current stream."""
    if isinstance(v, tuple):
        return tuple(host(e) for e in v)
    return v.cpu().numpy() if hasattr(v, "is_cuda") else np.asarray(v)


def same(got, want, what):
    if isinstance(want, tuple):
        assert isinstance(got, tuple) and len(got) == len(want), what
        for i, (g, w) in enumerate(zip(got, want)):
            same(g, w, (what, i))
        return
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    assert np.array_equal(bits(got), bits(want)), what


def final(obj):
    """What the object reports of its state once the calls are over."""
    names = ("skip", "fill", "phase", "state", "pilot_level", "stereo", "num_samples", "num_transforms", "psd")
    return tuple(host(getattr(obj, n)) for n in names if hasattr(obj, n))


def grab(obj, kind, res):
    """A call's result, with status and level for the SquelchBank's gate."""
    if kind == "__call__" and hasattr(obj, "threshold_linear"):
        return (res, obj.status, obj.level)
    return res


# ---------------------------------------------------------------- playing a sequence
def rotation(n):
    """(stream, filler) per call: three streams in turn; a filler in front of the first call
    on each stream and of every second call after them, so that each of those is followed at
    once by a call on another stream that sits behind no filler."""
    return [(i % 3, i < 3 or i % 2 == 0) for i in range(n)]


def play(torch, make, steps, streams=None, fill=None, plan=None):
    """A fresh object from make() taken through steps: (method name, input) is a call,
    ("do", f) runs f(obj) on the host and ("read", f) keeps f(obj).  Without streams
    everything runs on the current stream; with them, call i runs on streams[plan[i][0]],
    behind a filler where plan[i][1].  Returns the results on the host, the object's final
    report last; the test itself synchronizes only after the last step."""
    obj, outs, cur, calls = make(), [], None, 0
    torch.cuda.synchronize()
    for kind, arg in steps:
        if kind in ("do", "read"):
            with torch.cuda.stream(cur) if cur is not None else contextlib.nullcontext():
                res = arg(obj)
                if kind == "read":
                    outs.append(host(res))
            continue
        if streams is None:
            outs.append(grab(obj, kind, getattr(obj, kind)(arg)))
        else:
            s, filled = plan[calls]
            cur = streams[s]
            with torch.cuda.stream(cur):
                if filled and hasattr(arg, "is_cuda"):
                    fill()
                outs.append(grab(obj, kind, getattr(obj, kind)(arg)))
        calls += 1
    torch.cuda.synchronize()
    if streams is not None:
        fill.check()
    return [host(o) for o in outs] + [final(obj)]


def compare(torch, make, steps, streams, fill, plan=None, ref_steps=None, axis=-1):
    """The one-stream run against the run on streams: every step's result, the
    concatenation of the calls' (last) outputs and the final report, bit for bit."""
    ncalls = sum(1 for k, _ in steps if k not in ("do", "read"))
    want = play(torch, make, ref_steps or steps)
    got = play(torch, make, steps, streams, fill, plan or rotation(ncalls))
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        same(g, w, i)

    def cat(outs):
        last = [o[-1] if isinstance(o, tuple) else o for o, (k, _) in zip(outs, [s for s in steps if s[0] != "do"])
                if k != "read"]
        arrays = [a for a in last if a.ndim >= 1]
        if len({a.shape[:-1] if axis else a.shape[1:] for a in arrays}) > 1:     # a retune changed the row count
            arrays, ax = [a.reshape(-1) for a in arrays], 0
        else:
            ax = axis
        return np.concatenate(arrays, axis=ax)

    same(cat(got), cat(want), "concatenation")
    return got


# ---------------------------------------------------------------- the cases
def cuts(F, D, skip=True):
    """Eight pieces: a tile and one ragged sample, then an empty piece, one shorter than skip, ragged ones."""
    lens = [F * D + 1, D + 1, 0, 1, 2 * D + 3, F * D + D - 1, max(D - 1, 1), 3 * D + 2]
    assert not skip or (-sum(lens[:3])) % D > 1       # piece 3 ends before the next output
    return lens


def dev(torch, a):
    return torch.from_numpy(np.array(a)).cuda()


def wide_steps(torch, seed, lens, kinds=None, gen=None):
    """1-D pieces: complex64 (gen(n), seeded noise by default), int16 IQ pairs for the ...bytes methods."""
    rng = np.random.default_rng(seed)
    kinds = kinds or ["__call__"] * len(lens)
    steps = []
    for kind, n in zip(kinds, lens):
        a = raw_iq(rng, n) if kind.endswith("bytes") else (gen(n) if gen else cgauss(rng, n))
        steps.append((kind, dev(torch, a)))
    return steps


def row_steps(torch, x, lens, kinds=None):
    """Column ranges of one device image [rows, sum(lens)], read in place."""
    assert x.shape[1] == sum(lens)
    xd, at, steps = dev(torch, x), 0, []
    for i, n in enumerate(lens):
        steps.append((kinds[i] if kinds else "__call__", xd[:, at:at + n]))
        at += n
    return steps


def chan(M, m, D, mixed=False):
    def build(ld, torch):
        make = lambda: ld.Channelizer(M, D, m=m)
        lens = cuts(make().tile, D)
        kinds = ["from_bytes" if mixed and i % 2 else "__call__" for i in range(len(lens))]
        return make, wide_steps(torch, 100 + M + D, lens, kinds), -1
    return build


def synth(M, m, D):
    def build(ld, torch):
        make = lambda: ld.Synthesizer(M, D, m=m)
        sy = make()
        F, Q = sy.tile, -(-len(sy.taps) // D)
        lens = [F + 1, 2, 0, 1, Q, F + Q - 1, Q - 1, 3]
        return make, row_steps(torch, cgauss2(np.random.default_rng(200 + M), M, sum(lens)), lens), -1
    return build


def ddc(C, D, m, mixed=False):
    def build(ld, torch):
        f = freqs_for(np.random.default_rng(300 + C), C)
        make = lambda: ld.Downconverter(f, D, m=m)
        lens = cuts(make().tile, D)
        kinds = ["from_bytes" if mixed and i % 2 else "__call__" for i in range(len(lens))]
        return make, wide_steps(torch, 310 + D, lens, kinds), -1
    return build


def fmbank(C, D, m):
    def build(ld, torch):
        make = (lambda: ld.FMBank(C, KF, D, m=m)) if m else (lambda: ld.FMBank(C, KF))
        lens = cuts(make().tile, D, skip=D > 1)
        return make, row_steps(torch, fm_rows(400 + D, C, sum(lens)), lens), -1
    return build


def audiobank(C, sr, pcm16=False):
    def build(ld, torch):
        rate = 0.192
        make = lambda: ld.AudioBank(C, rate, 20, nfilter=13, deemphasis=sr, pcm16=pcm16)
        n1 = math.ceil((make().tile + 1) / rate) + 3
        lens = [n1, 2, 0, 1, int(1 / rate) + 3, n1 // 2, 5, 17]
        return make, row_steps(torch, audio_rows(500, C, sum(lens)), lens), -1
    return build


def squelch(C, B, alpha, timeout):
    def build(ld, torch):
        make = lambda: ld.SquelchBank(C, B, -10.0, alpha, timeout)
        T = make().tile
        lens = [T * B + 3, B + 1, 0, 1, 2 * B + 5, T * B + B - 1, B - 1, 7]
        assert all(t % B for t in np.cumsum(lens))                # every call leaves an unfinished block behind
        nb = sum(lens) // B
        x, _ = squelch_rows(C, B, alpha, timeout, nb, tail=sum(lens) - nb * B)
        kinds = ["measure" if i % 2 else "__call__" for i in range(len(lens))]
        return make, row_steps(torch, x, lens, kinds), -1
    return build


def stereo(C, D, L):
    def build(ld, torch):
        make = lambda: ld.StereoBank(C, PILOT, D, ntaps=L)
        lens = cuts(make().tile, D)
        return make, row_steps(torch, stereo_rows(600 + D, C, sum(lens))[0], lens), -1
    return build


def spgram(N, W, d, A, window):
    def build(ld, torch):
        make = lambda: make_spgram(ld, N, W, d, A, window)
        F = make().tile
        blocked = A >= 16 and A % 8 == 0
        Ab = 8 if blocked else A
        lens = [d * (F * Ab + 1) + 3, d + 1, 0, 1, d * (Ab + 1) + 2, d * (2 * A + 3) + 5, d - 1, d * (A + Ab // 2 + 1) + 1]
        ends = [int(t) // d for t in np.cumsum(lens)]              # transforms taken after each piece
        assert any(s % A for s in ends)                            # a piece ends inside a row: carry flips
        assert not blocked or any(s >= 8 and (s // 8) % (A // 8) for s in ends)   # and inside a row's blocks: rcarry
        kinds = ["__call__", "write", "from_bytes", "__call__", "write_bytes", "__call__", "write", "from_bytes"]
        seed = 700 + N + d
        return make, wide_steps(torch, seed, lens, kinds, gen=lambda n: signal(seed + n, n, N)), 0
    return build


CASES = {
    "chan-critical": chan(16, 6, 16), "chan-2x": chan(8, 6, 4), "chan-bytes-mixed": chan(64, 6, 32, mixed=True),
    "synth": synth(16, 6, 8),
    "ddc": ddc(3, 5, 6), "ddc-bytes-mixed": ddc(16, 64, 6, mixed=True),
    "fmbank": fmbank(16, 8, 6), "fmbank-disc": fmbank(3, 1, 0),
    "audiobank-deemph": audiobank(4, 250e3), "audiobank-plain": audiobank(4, None),
    "audiobank-pcm16": audiobank(5, 250e3, pcm16=True),
    "squelch": squelch(16, 1024, 1.0, 2), "squelch-odd-block": squelch(3, 100, 0.25, 4),
    "stereo": stereo(3, 5, None), "stereo-16": stereo(16, 4, 181),
    "spgram": spgram(1024, 300, 7, 3, "hann"), "spgram-blocked": spgram(1024, 1024, 64, 24, "hamming"),
}


# ---------------------------------------------------------------- 1. rotating streams
@pytest.mark.parametrize("name", list(CASES))
def test_rotating_streams(ld, torch, fill, streams, name):
    make, steps, axis = CASES[name](ld, torch)
    assert len(steps) >= 6 and any(a.numel() == 0 for _, a in steps)
    compare(torch, make, steps, streams[:3], fill, axis=axis)


# ---------------------------------------------------------------- 2. read-backs see the last call
# stream, filler: the second call behind a filler, the third at once on another stream, then the read
BEHIND = [(0, True), (1, True), (2, False)]


@pytest.mark.parametrize("name,read", [
    ("squelch", lambda o: (o.status, o.level, o.state, o.fill)),
    ("squelch-odd-block", lambda o: (o.status, o.level, o.state, o.fill)),
    ("stereo-16", lambda o: (o.pilot_level, o.stereo)),
    ("spgram", lambda o: (o.psd, o.num_transforms)),
    ("spgram-blocked", lambda o: (o.psd, o.num_transforms)),
])
def test_read_backs_see_the_last_call(ld, torch, fill, streams, name, read):
    """The read comes straight after the third call; the test synchronizes nothing before it."""
    make, steps, axis = CASES[name](ld, torch)
    picked = [steps[0], steps[1], steps[4], ("read", read)]
    compare(torch, make, picked, streams[:3], fill, plan=BEHIND, axis=axis)


# ---------------------------------------------------------------- 3. setters and resets between streams
# call, call behind a filler, the setter on the host, a call at once on a third stream; then a
# call behind a filler and one at once on another stream, after the setter's wait if it has one
AROUND = [(0, True), (1, True), (2, False), (0, True), (1, False)]


def retune(o):
    o.freqs = freqs_for(np.random.default_rng(9), 5)


def thresholds(o):
    o.threshold = np.linspace(-13.25, -3.5, o.nchan)


def set_scale(o):
    o.scale = 0.5


def set_threshold(o):
    o.threshold = 0.2


SETTERS = [("ddc", retune), ("squelch", thresholds), ("squelch-odd-block", thresholds), ("stereo", set_threshold),
           ("chan-2x", set_scale), ("fmbank", set_scale), ("audiobank-deemph", set_scale)]
SETTERS += [(name, "reset") for name in ("chan-critical", "synth", "ddc", "fmbank", "audiobank-deemph", "squelch",
                                          "stereo-16", "spgram-blocked")]
SETTERS += [("spgram", "clear"), ("spgram-blocked", "clear")]


@pytest.mark.parametrize("name,setter", SETTERS, ids=[f"{n}-{s if isinstance(s, str) else s.__name__}" for n, s in SETTERS])
def test_setters_between_streams(ld, torch, fill, streams, name, setter):
    """The calls before the setter give the old setting's output, the calls after it that of an
    object that had the new setting from that point of the stream on: the one-stream sequence."""
    make, steps, axis = CASES[name](ld, torch)
    do = (lambda o: getattr(o, setter)()) if isinstance(setter, str) else setter
    picked = [steps[0], steps[4], ("do", do), steps[1], steps[5], steps[7]]
    got = compare(torch, make, picked, streams[:3], fill, plan=AROUND, axis=axis)
    if setter == "clear":                             # psd counts the later transforms, the rows go on
        sp = make()
        d = sp.delay
        n = [int(a.numel()) // (2 if a.dtype == torch.int16 else 1) for _, a in (steps[0], steps[4], steps[1], steps[5],
                                                                                  steps[7])]
        before, total = sum(n[:2]) // d, sum(n) // d
        assert 0 < before < total and int(got[-1][-2]) == total - before


# ---------------------------------------------------------------- 4. host and device calls on one object
MIXED = [(0, True), (1, True), (0, False), (2, False), (0, True), (0, False), (1, False)]


@pytest.mark.parametrize("name", ["chan-2x", "fmbank", "squelch", "stereo-16", "spgram-blocked"])
def test_host_and_device_calls(ld, torch, fill, streams, name):
    """A device call behind a filler, the next piece as a numpy array (a host-memory call on the
    library's own stream), a device call on a third stream: the bits of the device run on one stream."""
    make, steps, axis = CASES[name](ld, torch)
    ref = [steps[i] for i in (0, 1, 4, 3, 5, 6, 7)]
    mixed = [(k, a.cpu().numpy() if i in (2, 5) else a) for i, (k, a) in enumerate(ref)]
    compare(torch, make, mixed, streams[:3], fill, plan=MIXED, ref_steps=ref, axis=axis)


# ---------------------------------------------------------------- 5. a chain across streams
def chain(ld, torch, kind, pieces, streams=None, fill=None, rotate=False):
    """The producer takes the pieces one right after the other, its second call behind a
    filler and its third behind none; then each consumer follows, piece by piece."""
    C = 16
    ch = ld.Channelizer(C, 8)
    if kind == "squelch":
        sq, fm, au = ld.SquelchBank(C, 64, -20.0, 0.5, 2), ld.FMBank(C, KF, 4), ld.AudioBank(C, 0.192, deemphasis=250e3)
        stages = [ch, sq, fm, au]
    else:
        fm1, st, au = ld.FMBank(C, 0.3), ld.StereoBank(C, PILOT, 5), ld.AudioBank(2 * C, 0.96, deemphasis=50e3)
        stages = [ch, fm1, st, lambda t: au(t.reshape(2 * C, -1))]
    keep = []                                         # no tensor's memory is reused while a stream may read it
    torch.cuda.synchronize()
    vals = [(x, None) for x in pieces]
    for k, stage in enumerate(stages):
        for p, (v, ev) in enumerate(vals):
            if streams is None:
                vals[p] = (stage(v), None)
                continue
            s = streams[(k + p) % 4 if rotate else k]
            with torch.cuda.stream(s):
                if ev is not None:
                    s.wait_event(ev)                  # the caller orders the tensor
                if k == 0 and p < 2:
                    fill()
                v = stage(v)
                ev = torch.cuda.Event()
                ev.record(s)
            keep.append(v)
            vals[p] = (v, ev)
    torch.cuda.synchronize()
    if streams is not None:
        fill.check()
    return [host(v) for v, _ in vals]


@pytest.mark.parametrize("rotate", [False, True], ids=["own-stream", "rotating"])
@pytest.mark.parametrize("kind", ["squelch", "stereo"])
def test_chain_across_streams(ld, torch, fill, streams, kind, rotate):
    """au(fm(sq(ch(x)))) and au(st(fm1(ch(x))).reshape(2C, -1)) over three pieces, every object
    on a stream of its own.  This is the one place where the test orders streams itself, with
    an event per tensor: an object orders its own state and scratch across streams, not the
    tensors its caller hands from one object to the next.  own-stream: an object stays on its
    stream, so its own order is stream order and only the caller's events are at work.
    rotating: every object moves on by one of the four streams with every piece (four
    different streams per piece still), so the producer's third call, behind no filler, is on
    another stream than its second, which waits behind a filler: the object's own order is at
    work as well.  (Four streams, not more: streams beyond the runtime's hardware queues share
    one with an earlier stream and are held back with it.)"""
    rng = np.random.default_rng(800)
    pieces = [dev(torch, cgauss(rng, n)) for n in (8 * 3000 + 5, 8 * 1000 + 3, 8 * 2000 + 1)]
    want = chain(ld, torch, kind, pieces)
    got = chain(ld, torch, kind, pieces, streams, fill, rotate)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape[1] > 0 and w.any()             # the squelch is open: noise at -12 dB per channel, threshold -20 dB
        same(g, w, i)
    same(np.concatenate(got, axis=1), np.concatenate(want, axis=1), "concatenation")
