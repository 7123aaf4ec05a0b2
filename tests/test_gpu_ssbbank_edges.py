"""SSBBank at the edges: one non-finite input sample, calls on different streams,
and a SquelchBank in front.

Non-finite input.  Two fresh banks run over the same finite input, fed as two
calls; in the second run one sample (row r, position t0 in the kernel's second
tile, off the tile's edges) is non-finite.  The calls are cut a few columns
after t0, so the bad sample also passes through the history pair.  0 * NaN is
NaN, so the columns whose bits differ from the clean run's are the exact read
footprint of the kernel: the columns n with 0 <= nD - t0 < L of row r, every one
of them, and no other column or row, in this call and in the next.  Three bad
samples are tried: NaN in both components, one NaN and one infinity (re = NaN,
im = +inf), and +inf in both.  Every column of the footprint is NaN for each of
them.  With a NaN in the sample each of the four sums takes a product with it
or, for the two sums over the infinite component, meets one that did in
S_re = P.x - Q.y and S_im = P.y + Q.x.  With +inf in both components
P.x = P.y = inf Re g and Q.x = Q.y = inf Im g (NaN where the tap is 0), so S_re is
inf - inf where Re g and Im g have the same sign and S_im is where they do not:
one of the two is NaN at every offset, and the rotation passes it on.  The
kernel finishes; nothing here provokes a fault.

Streams.  The bank keeps its calls in call order whichever stream each call is
made on, in the manner of tests/test_gpu_bank_streams.py and with its filler,
sizes and comparisons: the next call, made at once on another stream and behind
no filler, would otherwise read the half of the history pair the call before it
has not written yet; a retune between such calls waits for the calls before it."""
import numpy as np
import pytest

import test_gpu_ssbbank as t_sb
from test_gpu_bank_nonfinite import contained, decim_layout, joined, two_calls
from test_gpu_bank_streams import BEHIND, compare, cuts, fill, row_steps, streams, torch  # noqa: F401  (fixtures among them)

pytestmark = pytest.mark.gpu

SHAPE = (3, 2, 81, 0.025, 0.225)                      # (C, D, L, lo, hi)
BAD = {"nan": complex(np.nan, np.nan), "nan-inf": complex(np.nan, np.inf), "inf": complex(np.inf, np.inf)}


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- non-finite input
@pytest.mark.parametrize("name", list(BAD))
@pytest.mark.parametrize("shape", [SHAPE, (5, 5, 501, 0.004, 0.1)], ids=["3-2-81", "5-5-501"])
def test_one_bad_sample_stays_in_its_footprint(ld, shape, name):
    C, D, L, lo, hi = shape
    row = C - 1
    bfo, side = t_sb.lists_for(600 + C, C)
    mk = lambda: t_sb.make(ld, shape, bfo, side)
    t0, cut, K = decim_layout(mk().tile, D, L)
    x = np.stack([np.array(t_sb.rows_for(600 + c, 1, K, lo, hi, bfo[c:c + 1], side[c:c + 1])[0][0]) for c in range(C)])
    ref = t_sb.Ref(mk().row_taps, mk().words, D, x)
    assert np.isfinite(ref.y).all()
    bad = np.array(x)
    bad[row, t0] = BAD[name]
    clean, dirty_run = two_calls(mk(), x, cut), two_calls(mk(), bad, cut)
    lag = np.arange(-(-K // D)) * D - t0
    dirty = (lag >= 0) & (lag < L)
    assert cut - t0 < L and (lag >= L).sum() >= 3 and (lag < 0).sum() > mk().tile
    yc, yb = joined(clean, 0), joined(dirty_run, 0)
    contained(yc, yb, dirty, row=row, what=f"SSBBank D={D} L={L} {name}")
    assert (bits(yc[row]) != bits(yb[row]))[dirty].all()                   # exactly the footprint, every column of it
    assert np.isfinite(np.delete(yb, row, axis=0)).all() and np.isfinite(yb[row, ~dirty]).all()
    assert np.isnan(yb[row, dirty]).all()


# ---------------------------------------------------------------- streams
def ssbbank(shape):
    def build(ld, torch):
        C, D, L, lo, hi = shape
        bfo, side = t_sb.lists_for(610 + C, C)
        make = lambda: t_sb.make(ld, shape, bfo, side)
        lens = cuts(make().tile, D)
        x, _ = t_sb.rows_for(600 + D, C, sum(lens), lo, hi, bfo, side)
        return make, row_steps(torch, x, lens)
    return build


CASES = {"3-5-501": ssbbank((3, 5, 501, 0.004, 0.1)), "16-4-201": ssbbank((16, 4, 201, 0.01, 0.1))}


def report(o):
    return o.skip, o.words, o.row_taps


@pytest.mark.parametrize("name", list(CASES))
def test_two_calls_on_two_streams(ld, torch, fill, streams, name):
    """The second call behind a filler on one stream, the third at once on another, no host sync between
    them; then the read-backs."""
    make, steps = CASES[name](ld, torch)
    picked = [steps[0], steps[1], steps[4], ("read", report)]
    compare(torch, make, picked, streams[:3], fill, plan=BEHIND)


@pytest.mark.parametrize("name", list(CASES))
def test_rotating_streams(ld, torch, fill, streams, name):
    """Eight pieces, an empty one and one shorter than skip among them, over three streams in turn."""
    make, steps = CASES[name](ld, torch)
    assert len(steps) >= 6 and any(a.numel() == 0 for _, a in steps)
    compare(torch, make, steps + [("read", report)], streams[:3], fill)


def retune(o):
    o.bfo = np.linspace(-0.4, 0.4, o.nchan)
    o.sideband = "lsb"


@pytest.mark.parametrize("setter", [retune, "reset"], ids=["retune", "reset"])
def test_setters_between_streams(ld, torch, fill, streams, setter):
    """The calls before the setter give the old setting's output, the calls after it the new one's."""
    make, steps = CASES["3-5-501"](ld, torch)
    do = (lambda o: o.reset()) if setter == "reset" else setter
    picked = [steps[0], steps[4], ("do", do), steps[1], steps[5], steps[7], ("read", report)]
    compare(torch, make, picked, streams[:3], fill, plan=[(0, True), (1, True), (2, False), (0, True), (1, False)])


# ---------------------------------------------------------------- behind a squelch
def test_squelched_blocks_are_silent(ld):
    """ssb(sq(x)): row 0 is SSB throughout, row 1 falls to -60 dB after 40 blocks and the SquelchBank closes it,
    row 2 is closed throughout.  Every column whose L-sample window lies wholly in zeroed samples is +0.0."""
    C, D, L, B = 3, 4, 201, 64
    lo, hi = 0.01, 0.1
    K = 100 * B + 7
    bfo, side = np.array([0.0, 0.2, -0.35]), np.array([1, -1, 1])
    x = np.stack([np.array(t_sb.rows_for(5000 + c, 1, K, lo, hi, bfo[c:c + 1], side[c:c + 1])[0][0]) for c in range(C)])
    x = (0.5 * x / np.abs(x).max(axis=1, keepdims=True)).astype(np.complex128)
    rng = np.random.default_rng(5005)
    quiet = 1e-3 * (rng.standard_normal((2, K)) + 1j * rng.standard_normal((2, K))) / np.sqrt(2)
    x[1, 40 * B:] = quiet[0, 40 * B:]
    x[2] = quiet[1]
    z = ld.SquelchBank(C, B, -20.0, 0.5, 2)(x.astype(np.complex64))
    assert z.shape == (C, 100 * B)
    zero = z == 0
    assert not zero[0, 10 * B:].any() and zero[2, 10 * B:].all() and not zero[1, 10 * B:40 * B].any() and zero[1, 60 * B:].all()
    y = t_sb.make(ld, (C, D, L, lo, hi), bfo, side)(z)
    before = np.concatenate([np.zeros((C, 1), np.int64), np.cumsum(zero, axis=1)], axis=1)   # zeroed samples before sample i
    n = np.arange(y.shape[1]) * D                     # the window of column n: samples nD - L + 1 .. nD, zeros before 0
    first = np.maximum(n - L + 1, 0)
    silent = (before[:, n + 1] - before[:, first]) == (n + 1 - first)[None, :]
    assert silent[2, 20 * B // D:].all() and silent[1].sum() > 30 * B // D and not silent[0, 20 * B // D:].any()
    assert (bits(y)[silent] == 0).all()
    assert (y[~silent] != 0).mean() > 0.99
