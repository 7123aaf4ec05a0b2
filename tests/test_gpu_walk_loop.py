"""The PLL walker's repair loop (k_pll_walk) on calls just large enough for the
candidates + walk path: both crossing directions, state carried over ragged
calls with a padded last walker block, lane-blocks redone by walk_fallback, and
the Costas loop (every sample an entry).  Every output is compared bit for bit
with the restatement's AmpModem on the same input."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

FS = 48000.0


def am_signal(n, fcar, seed=20):
    """AM, modulation 0.5, on a carrier fcar Hz off centre, SNR 30 dB."""
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    msg = (np.sin(2 * np.pi * 400 * t) + np.sin(2 * np.pi * 1000 * t) + np.sin(2 * np.pi * 2500 * t)) / 3
    s = (1 + 0.5 * msg) * np.exp(1j * (2 * np.pi * fcar * t + 0.7))
    s = s + 10 ** (-1.5) * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
    return s.astype(np.complex64)


def dsbsc_signal(n, seed=21):
    rng = np.random.default_rng(seed)
    t = np.arange(n) / FS
    m = (np.sin(2 * np.pi * 400 * t) + np.sin(2 * np.pi * 1000 * t)) / 2
    s = m * np.exp(1j * (2 * np.pi * 100 * t + 0.7))
    s = s + 0.02 * (rng.standard_normal(n) + 1j * rng.standard_normal(n)) / np.sqrt(2)
    return s.astype(np.complex64)


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def assert_bitwise(y, ref):
    y, ref = np.asarray(y), np.asarray(ref)
    assert y.shape == ref.shape, (y.shape, ref.shape)
    eq = y.view(np.uint32) == ref.view(np.uint32)
    if not eq.all():
        i = int(np.argmin(eq))
        raise AssertionError(f"{(~eq).sum()} of {eq.size} differ; first at {i}: {y[i]!r} vs {ref[i]!r}")


@pytest.fixture(scope="module")
def carrier_case(ora):
    """4 096 PCM samples at each carrier offset of the bench (+-1.2 kHz) with the restatement's output"""
    out = {}
    for fcar in (1200.0, -1200.0):
        x = am_signal(4096, fcar)
        o = ora.AmpModem(0.5, "dsb", carrier=True)
        out[fcar] = (x, o(x), o.pll_state)
    return out


@pytest.mark.parametrize("fcar", [1200.0, -1200.0])
def test_walk_both_crossing_directions(ld, carrier_case, fcar):
    x, ref, state = carrier_case[fcar]
    g = ld.AmpModem(modulation=0.5, type="dsb", carrier=True)
    y = g(x)
    entries, repairs, fallbacks = g._walk_stats()
    print(f"fcar {fcar}: entries {entries} repairs {repairs} fallbacks {fallbacks}")
    assert_bitwise(y, ref)
    assert g.pll_state() == state
    assert repairs > 0


def test_walk_ragged_calls(ld, ora):
    # 1 024 samples (the smallest candidates + walk call), then 1 537 on the same
    # object: the state carried across and a padded last walker block in each
    x = am_signal(1024 + 1537, 1200.0)
    o = ora.AmpModem(0.5, "dsb", carrier=True)
    g = ld.AmpModem(modulation=0.5, type="dsb", carrier=True)
    y0 = g(x[:1024])
    assert g._walk_stats()[0] > 0            # walked, not the sequential loop
    y1 = g(x[1024:])
    assert g._walk_stats()[0] > 0
    assert_bitwise(np.concatenate([y0, y1]), o(x))
    assert g.pll_state() == o.pll_state


# Entry margin B = 2^MARGIN_LOG2 (2^19 in the product) at which the 4 096-sample
# calls below leave gaps whose proofs fail (2^19: none), measured on the commit
# before the repair loop's accumulators moved behind its compare: (entries,
# repairs, fallbacks) = MARGIN_STATS per offset.  A reordered loop repairs the
# same lanes, so the counts stay.
MARGIN_LOG2 = 18
MARGIN_STATS = {1200.0: (538, 59, 3), -1200.0: (546, 91, 6)}


@pytest.mark.parametrize("fcar", [1200.0, -1200.0])
def test_walk_fallback_lane_blocks(ld, carrier_case, fcar):
    x, ref, state = carrier_case[fcar]
    g = ld.AmpModem(modulation=0.5, type="dsb", carrier=True)
    prev = ld._debug_pll_margin(MARGIN_LOG2)
    try:
        y = g(x)
        stats = tuple(g._walk_stats())
    finally:
        ld._debug_pll_margin(prev)
    print(f"fcar {fcar}: margin 2^{MARGIN_LOG2}: entries, repairs, fallbacks {stats}")
    assert_bitwise(y, ref)
    assert g.pll_state() == state
    assert stats[2] > 0
    assert stats == MARGIN_STATS[fcar]


def test_walk_costas(ld, ora):
    # suppressed carrier: every sample is an entry and B = 2^21
    x = dsbsc_signal(2048)
    o = ora.AmpModem(0.5, "dsb", carrier=False)
    g = ld.AmpModem(modulation=0.5, type="dsb", carrier=False)
    y = g(x)
    entries = g._walk_stats()[0]
    assert_bitwise(y, o(x))
    assert g.pll_state() == o.pll_state
    assert entries == len(x)
