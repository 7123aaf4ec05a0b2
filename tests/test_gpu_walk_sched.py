"""The PLL walker's lane-block transition and block end (k_pll_walk's asm loop) on a
call of 20 walker blocks: more than twice the 8-block LDS ring, so every slot is
reused and the entry reads that the walker issues behind the block-end barrier hit
a wrapped ring.  The transition's interval test runs in the shadow of the next
lane-block's offsets, beside the LDS reads that refill this lane-block's entry
registers: an order that read a refilled register would change which blocks fail
their test, so the (entries, repairs, fallbacks) counts are pinned per entry margin
beside the bitwise comparison with the restatement's AmpModem."""
import numpy as np
import pytest

from test_gpu_walk_loop import am_signal, assert_bitwise

pytestmark = pytest.mark.gpu

N = 40000
RAGGED = (1024, 17000, 21976)


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


@pytest.fixture(scope="module")
def long_case(ora):
    """40 000 PCM samples at each carrier offset of the bench with the restatement's output and state"""
    out = {}
    for fcar in (1200.0, -1200.0):
        x = am_signal(N, fcar)
        o = ora.AmpModem(0.5, "dsb", carrier=True)
        ref = o(x)
        ref.setflags(write=False)
        out[fcar] = (x, ref, o.pll_state)
    return out


# (entries, repairs, fallbacks) of the one 40 000-sample call per carrier offset and
# entry margin B = 2^margin (None: the product's 2^19), measured on the commit before
# the transition was re-spaced.  The same instructions in another order repair the
# same lanes and fail the same blocks, so the counts stay.
SCHED_STATS = {
    (1200.0, None): (10215, 759, 0),
    (1200.0, 18): (5170, 759, 40),
    (1200.0, 17): (2748, 759, 43),
    (-1200.0, None): (10129, 785, 1),
    (-1200.0, 18): (5256, 785, 33),
    (-1200.0, 17): (2824, 785, 45),
}


@pytest.mark.parametrize("margin", [None, 18, 17])
@pytest.mark.parametrize("fcar", [1200.0, -1200.0])
def test_walk_sched_wrapped_ring(ld, long_case, fcar, margin):
    x, ref, state = long_case[fcar]
    g = ld.AmpModem(modulation=0.5, type="dsb", carrier=True)
    prev = ld._debug_pll_margin(margin) if margin is not None else None
    try:
        y = g(x)
        stats = tuple(g._walk_stats())
    finally:
        if prev is not None:
            ld._debug_pll_margin(prev)
    print(f"fcar {fcar}: margin {margin}: entries, repairs, fallbacks {stats}")
    assert_bitwise(y, ref)
    assert g.pll_state() == state
    if margin is None:
        assert stats[0] > 2 * 8 * 512        # more than twice the ring of 512-entry blocks: every slot reused
    else:
        assert stats[2] > 0                  # (a smaller margin makes fewer entries: 11 and 6 blocks)
    assert stats == SCHED_STATS[(fcar, margin)]


@pytest.mark.parametrize("fcar", [1200.0, -1200.0])
def test_walk_sched_ragged_calls(ld, long_case, fcar):
    x, ref, state = long_case[fcar]
    assert sum(RAGGED) == N
    g = ld.AmpModem(modulation=0.5, type="dsb", carrier=True)
    ys, at = [], 0
    for n in RAGGED:
        ys.append(np.asarray(g(x[at:at + n])))
        at += n
        assert g._walk_stats()[0] > 0        # walked, not the sequential loop
    assert_bitwise(np.concatenate(ys), ref)
    assert g.pll_state() == state
