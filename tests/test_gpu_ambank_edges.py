"""AMBank at the edges: one non-finite input sample, and calls on different
streams.

Non-finite input.  Two fresh banks run over the same finite input, fed as two
calls; in the second run one sample (row r, position t0 in the kernel's second
tile, off the tile's edges) is NaN or +inf in both of its components.  The calls
are cut a few columns after t0, so the bad sample also passes through the
history pair.  0 * NaN is NaN, so the columns whose bits differ from the clean
run's are the exact read footprint of the kernel: the columns n with
0 <= nD - t0 < L of row r, every one of them (a NaN in Cr makes m > thr^2 false
and y = +0, an infinity makes m infinite or NaN and y a NaN or +0; the clean
run is non-zero there), and no other column or row, in this call and in the
next.  The kernel finishes; nothing here provokes a fault.

Streams.  The bank keeps its calls in call order whichever stream each call is
made on, in the manner of tests/test_gpu_bank_streams.py and with its filler,
sizes and comparisons: the next call, made at once on another stream and behind
no filler, would otherwise read the half of the history pair the call before it
has not written yet."""
import numpy as np
import pytest

import test_gpu_ambank as t_am
from test_gpu_bank_nonfinite import VALUES, contained, decim_layout, joined, poisoned, two_calls
from test_gpu_bank_streams import BEHIND, compare, cuts, fill, row_steps, streams, torch  # noqa: F401  (fixtures among them)

pytestmark = pytest.mark.gpu

SHAPE = (3, 5, 251, None, 0.016)                      # (C, D, L, audio, carrier)


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    return np.ascontiguousarray(np.atleast_1d(a)).view(np.uint32 if np.asarray(a).dtype.itemsize == 4 else np.uint8)


# ---------------------------------------------------------------- non-finite input
@VALUES
def test_one_bad_sample_stays_in_its_footprint(ld, value):
    C, D, L, audio, carrier = SHAPE
    row = 1
    mk = lambda: t_am.make(ld, *SHAPE)
    t0, cut, K = decim_layout(mk().tile, D, L)
    rows = [t_am.am_row(600 + 31 * c, K, t_am.cutoff(D, audio), carrier, L)[0] for c in range(C)]
    x = np.stack(rows).astype(np.complex64)
    ref = t_am.Ref(mk().carrier_taps, mk().band_taps, D, x, 0.0)
    assert np.isfinite(ref.y).all() and not ref.edge.any()

    def call(o, p):
        return o(p), o.carrier_level, o.carrier_present

    clean, bad = two_calls(mk(), x, cut, call), two_calls(mk(), poisoned(x, (row, t0), value), cut, call)
    lag = np.arange(-(-K // D)) * D - t0
    dirty = (lag >= 0) & (lag < L)
    assert cut - t0 < L and (lag >= L).sum() >= 3 and (lag < 0).sum() > mk().tile
    yc, yb = joined(clean, 0), joined(bad, 0)
    contained(yc, yb, dirty, row=row, what=f"AMBank D={D} L={L}")
    assert (bits(yc[row]) != bits(yb[row]))[dirty].all()                   # exactly the footprint, every column of it
    assert np.isfinite(np.delete(yb, row, axis=0)).all() and np.isfinite(yb[row, ~dirty]).all()
    for i in (1, 2):                                  # carrier_level, carrier_present: of the call's last column
        first = bits(clean[0][i]) == bits(bad[0][i])
        assert np.delete(first, row).all()
        assert (bits(clean[1][i]) == bits(bad[1][i])).all()                # past the footprint after the second call
    assert not (bits(clean[0][1]) == bits(bad[0][1]))[row]                 # inside it after the first


# ---------------------------------------------------------------- streams
def ambank(shape):
    def build(ld, torch):
        C, D, L, audio, carrier = shape
        make = lambda: t_am.make(ld, *shape)
        lens = cuts(make().tile, D)
        x, _, _ = t_am.rows_for(600 + D, C, sum(lens), t_am.cutoff(D, audio), carrier, L)
        return make, row_steps(torch, x, lens)
    return build


CASES = {"3-5-251": ambank(SHAPE), "16-4-181": ambank((16, 4, 181, None, 4 / 180))}


def report(o):
    return o.carrier_level, o.carrier_present, o.skip


@pytest.mark.parametrize("name", list(CASES))
def test_two_calls_on_two_streams(ld, torch, fill, streams, name):
    """The second call behind a filler on one stream, the third at once on another, no host sync between
    them; then the read-backs, which wait for the last call."""
    make, steps = CASES[name](ld, torch)
    picked = [steps[0], steps[1], steps[4], ("read", report)]
    compare(torch, make, picked, streams[:3], fill, plan=BEHIND)


@pytest.mark.parametrize("name", list(CASES))
def test_rotating_streams(ld, torch, fill, streams, name):
    """Eight pieces, an empty one and one shorter than skip among them, over three streams in turn."""
    make, steps = CASES[name](ld, torch)
    assert len(steps) >= 6 and any(a.numel() == 0 for _, a in steps)
    compare(torch, make, steps + [("read", report)], streams[:3], fill)


def set_threshold(o):
    o.threshold = 2.0


@pytest.mark.parametrize("setter", [set_threshold, "reset"], ids=["threshold", "reset"])
def test_setters_between_streams(ld, torch, fill, streams, setter):
    """The calls before the setter give the old setting's output, the calls after it the new one's."""
    make, steps = CASES["3-5-251"](ld, torch)
    do = (lambda o: o.reset()) if setter == "reset" else setter
    picked = [steps[0], steps[4], ("do", do), steps[1], steps[5], steps[7], ("read", report)]
    compare(torch, make, picked, streams[:3], fill, plan=[(0, True), (1, True), (2, False), (0, True), (1, False)])
