"""The walker's interval test over all lanes of a lane-block, on the fields that
pll_walk_fold computes (through ldsp_debug_walk_fold: the very function
k_pll_entries calls), against the two predicates in Python integers:

    passes  <=>  not an event (f in [lo, hi])  or  pre-repair offset f in [fl, fh]

with [lo, hi] the table cell around the candidate cut to [-B, B] when a
neighbouring gap is non-empty, and [fl, fh] the one possible crossing cut to
[-B, B] (left gap) and [-B - dk2, B - dk2] (right gap).  The walker evaluates
x <=u W or x - amin <=u awidth with x = f - lo (sat(x - W) and sat((x - amin) -
awidth) both non-zero is a failure).

[fl, fh] mostly starts where [lo, hi] ends, and the two would then fold into one
interval; where it does not (only the right gap non-empty, the cell's side towards
the crossing cut to +-B, dk2 pointing back inside) the offsets between them must
fail, which is why the walker keeps two tests.  Those cases are counted below."""
import ctypes as C
import itertools
import os

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(os.path.dirname(HERE), "python-liquiddsp_amd", "libldsp.so")
M32 = (1 << 32) - 1
CELL = 1 << 22


@pytest.fixture(scope="module")
def fold():
    if not os.path.exists(LIBPATH):
        pytest.fail("libldsp.so not built (run __graft_entry__.build())")
    lib = C.CDLL(LIBPATH)
    fn = lib.ldsp_debug_walk_fold
    fn.argtypes = [C.c_uint32, C.c_int32, C.c_int, C.c_int, C.c_uint32, C.POINTER(C.c_uint32)]
    fn.restype = C.c_int
    out = (C.c_uint32 * 4)()

    def call(u, B, lne, rne, dk2):
        assert fn(u, B, int(lne), int(rne), dk2 & M32, out) == 0
        lo = out[0] - (1 << 32) if out[0] >> 31 else out[0]
        return lo, out[1], out[2], out[3]
    return call


def predicates(u, B, lne, rne, d2):
    """[lo, hi], [fl, fh] as Python integers (fl > fh: empty)"""
    lo, hi = -u, CELL - 1 - u
    if lne or rne:
        lo, hi = max(lo, -B), min(hi, B)
    fl = CELL - u if u >= CELL // 2 else -CELL - u
    fh = fl + CELL - 1
    if lne:
        fl, fh = max(fl, -B), min(fh, B)
    if rne:
        fl, fh = max(fl, -B - d2), min(fh, B - d2)
    return lo, hi, fl, fh


def cases():
    for B in (1 << 18, 1 << 19, 1 << 21):
        us = set()
        for c in (0, B, 1 << 21, CELL - 1 - B, CELL - 1):
            us.update(v for v in (c - 1, c, c + 1) if 0 <= v < CELL)
        for u, lne, rne in itertools.product(sorted(us), (False, True), (False, True)):   # both directions: u
            for d2 in (0, 1, -1, 1000, -1000, (1 << 18) - 1, -(1 << 18) + 1, 1 << 18, -(1 << 18)):
                yield u, B, lne, rne, d2


def sweep(lo, hi, fl, fh):
    """edges of every interval +-1, and the wrapped side (offsets half a turn away)"""
    xs = set()
    for e in (lo, hi, fl, fh, fl + CELL - 1, -CELL, CELL, 0):
        xs.update((e - 1, e, e + 1))
    for e in (1 << 31, -(1 << 31), (1 << 31) - CELL, -(1 << 31) + CELL):
        xs.update((e - 1, e, e + 1))
    return sorted(v for v in xs if -(1 << 31) <= v < (1 << 31))


def walker_passes(x, W, amin, awidth):
    beyond = max(x - W, 0)                              # v_sub_u32 clamp
    outside = max(((x - amin) & M32) - awidth, 0)       # v_sub_u32, v_sub_u32 clamp
    return min(beyond, outside) == 0                    # v_min_u32, or'ed into the block's accumulator


def test_padding_entry():
    # k_pll_entries pads with W = ~0: never an event, and the test passes whatever x, amin, awidth
    for x in (0, 1, 1 << 31, M32):
        assert walker_passes(x, M32, 0, 0) and walker_passes(x, M32, 12345, 7)


def test_empty_accepted_interval_fails_every_repair(fold):
    # left gap non-empty and the cell cut on the crossing's side: [fl, fh] is empty
    u, B = 1 << 21, 1 << 19
    lo, hi, fl, fh = predicates(u, B, True, False, 0)
    assert fl > fh
    _, W, amin, awidth = fold(u, B, True, False, 0)
    assert (amin, awidth) == (0, 0)
    for x in (W + 1, W + 2, 1 << 31, M32):
        assert not walker_passes(x, W, amin, awidth)
    for x in (0, 1, W):
        assert walker_passes(x, W, amin, awidth)


def test_walker_test_equals_predicates(fold):
    n = detached = empty = 0
    bad = []
    for u, B, lne, rne, d2 in cases():
        lo, hi, fl, fh = predicates(u, B, lne, rne, d2)
        flo, W, amin, awidth = fold(u, B, lne, rne, d2)
        assert (flo, W) == (lo, hi - lo), (u, B, lne, rne, d2)
        up = u >= CELL // 2
        empty += fl > fh
        detached += fl <= fh and not (fl == hi + 1 if up else fh == lo - 1)
        for f in sweep(lo, hi, fl, fh):
            x = (f - lo) & M32
            event = x > W
            assert event == (not lo <= f <= hi)
            want = (not event) or fl <= f <= fh
            n += 1
            if walker_passes(x, W, amin, awidth) != want:
                bad.append((u, B, lne, rne, d2, f, want))
    print(f"{n} offsets checked; {empty} cases with an empty repair interval, {detached} with a detached one")
    assert n > 30_000 and empty > 0 and detached > 0
    assert not bad, (len(bad), bad[:5])
