"""The PLL walk with the repaired outputs stored and the repairs counted by the
loader waves one block after the walker (k_pll_walk: walk_help, xbuf, redone[]):
block counts around the LDS ring (8 slots, 6 blocks DMA'd ahead), ragged calls on
one object, redone blocks, the merged many-call launch and the Costas loop.  Every
output is compared bit for bit with the restatement's AmpModem (or, for the
many-call, with the same objects' single calls), and each case asserts the number
of walker blocks it was meant to hit."""
import numpy as np
import pytest

from test_gpu_walk_loop import am_signal, assert_bitwise, dsbsc_signal

pytestmark = pytest.mark.gpu

BLK = 512            # entries per walker block (kBlkE)


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def nblk(g):
    return -(-g._walk_stats()[0] // BLK)


@pytest.fixture(scope="module")
def signal():
    return am_signal(70000, 1200.0)


@pytest.fixture(scope="module")
def reference(ora, signal):
    """the restatement's output and state per prefix length, computed once"""
    memo = {}

    def get(n):
        if n not in memo:
            o = ora.AmpModem(0.5, "dsb", carrier=True)
            memo[n] = (o(signal[:n]), o.pll_state)
        return memo[n]
    return get


# PCM samples -> walker blocks (about 0.26 entries per sample at B = 2^19): one block
# (the smallest candidates + walk call), two, and the counts around the 6 blocks the
# prologue DMAs ahead and the ring's 8 slots, then well past one turn of the ring
@pytest.mark.parametrize("n,blocks", [(1024, 1), (3072, 2), (11400, 6), (13000, 7), (15000, 8), (17000, 9),
                                      (24600, 13)])
def test_block_counts(ld, signal, reference, n, blocks):
    ref, state = reference(n)
    g = ld.AmpModem(modulation=0.5, type="dsb", carrier=True)
    y = g(signal[:n])
    entries, repairs, fallbacks = g._walk_stats()
    print(f"n {n}: entries {entries} repairs {repairs} fallbacks {fallbacks}")
    assert nblk(g) == blocks
    assert_bitwise(y, ref)
    assert g.pll_state() == state
    assert repairs > 0


def test_ragged_calls(ld, signal, reference):
    # 1, 9 and 2 blocks on one object: xbuf's halves, redone[] and the loaders' count start afresh each call
    cuts = [0, 1024, 1024 + 17000, 1024 + 17000 + 3072]
    ref, state = reference(cuts[-1])
    g = ld.AmpModem(modulation=0.5, type="dsb", carrier=True)
    ys, blocks = [], []
    for a, b in zip(cuts, cuts[1:]):
        ys.append(g(signal[a:b]))
        blocks.append(nblk(g))
    assert blocks == [1, 9, 2]
    assert_bitwise(np.concatenate(ys), ref)
    assert g.pll_state() == state


# Entry margin B = 2^18 (the product: 2^19) on the first 32 800 samples: 9 walker
# blocks, gaps whose proofs fail and blocks that fail their interval test and are
# redone by the walker (the loaders skip them).  (entries, repairs, fallbacks)
# measured on the commit before the loader waves took over the stores and counts.
MARGIN_N = 32800
MARGIN_STATS = (4392, 594, 28)


def test_redone_blocks(ld, signal, reference):
    ref, state = reference(MARGIN_N)
    g = ld.AmpModem(modulation=0.5, type="dsb", carrier=True)
    prev = ld._debug_pll_margin(18)
    try:
        y = g(signal[:MARGIN_N])
        stats = tuple(g._walk_stats())
    finally:
        ld._debug_pll_margin(prev)
    print(f"margin 2^18: entries, repairs, fallbacks {stats}")
    assert nblk(g) == 9
    assert stats[2] > 0
    assert_bitwise(y, ref)
    assert g.pll_state() == state
    assert stats == MARGIN_STATS


def test_many_call(ld):
    # One merged launch, one workgroup per object.  A many-call takes one length for all
    # its objects, so the block counts differ through the loops instead: two carrier loops
    # and a Costas loop (every sample an entry), 1 / 1 / 3 blocks, then 3 / 3 / 9 on the
    # same objects, against the same objects' kind called one by one.
    import torch
    cuts = [0, 1536, 1536 + 4608]
    xs = [am_signal(cuts[-1], 1200.0), am_signal(cuts[-1], -1200.0, seed=22), dsbsc_signal(cuts[-1])]
    carrier = [True, True, False]

    def make():
        return [ld.AmpModem(modulation=0.5, type="dsb", carrier=c) for c in carrier]
    many, single = make(), make()
    for (a, b), want in zip(zip(cuts, cuts[1:]), ([1, 1, 3], [3, 3, 9])):
        ins = [torch.from_numpy(x[a:b]).cuda() for x in xs]
        outs = ld.execute_many(many, ins)
        assert [nblk(g) for g in many] == want
        for g, s, x, y in zip(many, single, ins, outs):
            assert_bitwise(y.cpu().numpy(), s(x).cpu().numpy())
            assert g._walk_stats() == s._walk_stats()
            assert g.pll_state() == s.pll_state()


def test_costas(ld, ora):
    # suppressed carrier: every sample is an entry (4 full blocks) and B = 2^21
    x = dsbsc_signal(2048)
    o = ora.AmpModem(0.5, "dsb", carrier=False)
    g = ld.AmpModem(modulation=0.5, type="dsb", carrier=False)
    y = g(x)
    assert g._walk_stats()[0] == len(x) and nblk(g) == 4
    assert_bitwise(y, o(x))
    assert g.pll_state() == o.pll_state
