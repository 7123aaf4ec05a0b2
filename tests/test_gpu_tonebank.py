"""ToneBank on the GPU: the per-row tone detector and tone squelch over bank rows
(k_tonebank.hip, the powers on v_mfma_f32_32x32x2_f32) against its definition
(include/ldsp.h), restated in numpy in tests/tonebank_model.py: the powers in float64 from
the object's own float32 tables, the decision as an exact function of float32 powers, the
hold window with its carried counter.

Rows are seeded noise (sigma 0.003, a different stream per row) plus a script of bursts whose
edges fall on block boundaries and inside blocks: a listed tone at 0.2, the row's wanted
tone, a frequency midway between two listed ones, a listed tone at 0.02 (dominant but under
the floor of 1e-3), all listed tones at once (over the floor, no dominance), silence.  One
row carries a component of amplitude 0.5 midway between two listed tones beside a listed
tone of 0.15; from five rows up one row is zeros and one is always on its wanted tone.  A
block whose float64 ratio or best power falls within 1e-3 of its threshold is replaced by
noise when the input is built; what the tests need of the inputs -- every decision value,
open by hit and by hold, the margins -- is then asserted on the float64 reference alone
before anything is compared.

Sizes come from the kernel's tile (T columns per workgroup): one call of B (2T + 1) + 3
samples per row is two full tiles, a ragged one and a carried tail.  The power gate of 1e-6
is the project's gate for this class of kernel, relative to the larger of the
row's largest float64 power and the row's largest block mean square (the power a listed
tone of that level would read: the arithmetic's scale where out-of-list content dominates).
tone, open and the gated rows are compared exactly.

Measured on an MI355X, worst over rows, (of the row's scale, of the largest power alone on
the rows without the strong component): (1, 2, 64, 0) 4.2e-8, -; (3, 5, 192, 1) 1.6e-7, 2.0e-7;
(16, 33, 1024, 2) 2.2e-7, 3.0e-7; (256, 9, 64, 1) 2.5e-7, 3.5e-7; (5, 64, 4096, 3) 2.0e-7, 2.2e-7;
(2, 50, 16384, 0) 1.4e-8, 1.7e-7.  DESIGN.md section 4, "ToneBank kernel", has the same table."""
import functools

import numpy as np
import pytest

import tonebank_model as M
from conftest import cgauss

pytestmark = pytest.mark.gpu

GATE = 1e-6
MARGIN = 1e-3
FLOOR = 1e-3
DOM = 8.0
SHAPES = [(1, 2, 64, 0), (3, 5, 192, 1), (16, 33, 1024, 2), (256, 9, 64, 1), (5, 64, 4096, 3), (2, 50, 16384, 0)]
SMALL = SHAPES[:4]            # the variations that run a stream several times


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def host(t):
    return t.cpu().numpy() if hasattr(t, "cpu") else np.asarray(t)


def tones_for(F):
    return 0.03 + (np.arange(F) + 0.37) * (0.44 / F)


def wants_for(C, F):
    w = (np.arange(C) * 7 + 1) % F
    w[0] = -1
    return w


def make(ld, C, F, B, hold, **kw):
    return ld.ToneBank(C, tones_for(F), block=B, dominance=DOM, floor=FLOOR, hold=hold, want=wants_for(C, F), **kw)


# ---------------------------------------------------------------- the inputs
def margins_ok(p64, F):
    k, _ = M.detect(p64, FLOOR, DOM)
    best = np.take_along_axis(p64, k[..., None], axis=-1)[..., 0]
    lhs, rhs = best * (F - 1), DOM * (p64.sum(axis=-1) - best)
    big = np.maximum(lhs, rhs)
    return ((np.abs(lhs - rhs) >= MARGIN * big) | (big == 0)) & (np.abs(best - FLOOR) >= MARGIN * FLOOR)


@functools.lru_cache(maxsize=None)
def case(C, F, B, hold, T):
    """x float32 [C][K], the float64 reference powers and its decisions."""
    rng = np.random.default_rng([C, F, B, hold])
    N = 2 * T + 1
    K = B * N + 3
    f, want = tones_for(F), wants_for(C, F)
    x = (0.003 * rng.standard_normal((C, K))).astype(np.float64)
    t = np.arange(K, dtype=np.float64)

    def add(c, a, b, freq, amp):
        a, b = max(int(a), 0), min(int(b), K)
        if b > a:
            x[c, a:b] += amp * np.cos(2 * np.pi * freq * t[a:b] + rng.uniform(0, 2 * np.pi))

    kinds = ["listed", "wanted", "unlisted", "weak", "comb", "silence", "listed", "wanted"]
    strong = 1 if C > 1 else 0
    for c in range(C):
        if C >= 5 and c == 2:
            x[c] = 0.0
            continue
        if C >= 5 and c == 3:
            add(c, 0, K, f[want[c]], 0.2)
            continue
        pos, i = 0, c
        while pos < K:
            kind = kinds[i % len(kinds)]
            i += 1
            nb = int(rng.integers(1, 2 * hold + 4))
            edge = 0 if rng.random() < 0.5 else int(rng.integers(1, B))       # on a boundary or inside a block
            a, b = pos + edge, pos + nb * B + (0 if rng.random() < 0.5 else int(rng.integers(1, B)))
            if kind == "listed":
                add(c, a, b, f[rng.integers(F)], 0.2)
            elif kind == "wanted":
                add(c, a, b, f[want[c] if want[c] >= 0 else rng.integers(F)], 0.2)
            elif kind == "unlisted":
                add(c, a, b, f[rng.integers(F - 1)] + 0.22 / F, 0.2)
            elif kind == "weak":
                add(c, a, b, f[rng.integers(F)], 0.02)
            elif kind == "comb":
                for k in range(F):
                    add(c, a, b, f[k], 0.1)
            pos = b + int(rng.integers(0, 2)) * B
        if c == strong:                               # the strong out-of-list component beside a listed tone
            add(c, K // 3, K, f[F // 2 - 1] + 0.22 / F, 0.5)
            add(c, K // 3, K, f[min(F // 2 + 1, F - 1)], 0.15)
    x = x.astype(np.float32)
    import liquiddsp
    tables = make(liquiddsp, C, F, B, hold).tables
    for _ in range(8):                                # blocks too near a threshold become noise
        p64 = M.power64(tables, x)
        bad = ~margins_ok(p64, F)
        if not bad.any():
            break
        for c, b in zip(*np.nonzero(bad)):
            x[c, b * B:(b + 1) * B] = (0.003 * rng.standard_normal(B)).astype(np.float32)
    p64 = M.power64(tables, x)
    tone, opn, nxt, acc = M.decide(p64, FLOOR, DOM, want, hold, np.full(C, M.SAT))
    x.setflags(write=False)
    return dict(x=x, p64=p64, tone=tone, open=opn, next=nxt, acc=acc, want=want, tables=tables, N=N, K=K,
                strong=strong)


@functools.lru_cache(maxsize=None)
def run(C, F, B, hold):
    """One call on a device tensor: (case, power, tone, open, y) as numpy."""
    import liquiddsp as ld
    import torch
    tb = make(ld, C, F, B, hold)
    cs = case(C, F, B, hold, tb.tile)
    y = tb(torch.tensor(cs["x"]).cuda())
    out = dict(power=host(tb.power), tone=host(tb.tone), open=host(tb.open), y=host(y), fill=tb.fill,
               state=tb.state.copy())
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return cs, out


def same(a, b, what=""):
    for k in ("power", "tone", "open"):
        assert a[k].shape == b[k].shape and a[k].dtype == b[k].dtype, (what, k)
        assert np.array_equal(bits(a[k]), bits(b[k])), (what, k)
    if "y" in a and "y" in b:
        assert np.array_equal(bits(a["y"]), bits(b["y"])), (what, "y")


# ---------------------------------------------------------------- the reference alone, then the kernel
@pytest.mark.parametrize("shape", SHAPES)
def test_against_the_definition(ld, shape):
    C, F, B, hold = shape
    cs, out = run(*shape)
    p64, N = cs["p64"], cs["N"]
    # what the reference alone must show
    k, hit = M.detect(p64, FLOOR, DOM)
    best = np.take_along_axis(p64, k[..., None], axis=-1)[..., 0]
    above = best > FLOOR
    want = cs["want"][:, None]
    assert hit.any(), "no hit"
    assert (~above).any(), "no miss by floor"
    assert (above & ~hit).any(), "no miss by dominance"
    if C > 1:
        assert (hit & (want >= 0) & (want != k)).any(), "no wrong tone for want"
    assert cs["acc"].any(), "nothing opens by a hit"
    if hold > 0:
        assert ((cs["open"] == 1) & ~cs["acc"]).any(), "nothing is open by hold"
    assert (cs["open"] == 0).any()
    assert margins_ok(p64, F).all(), "a block within 1e-3 of a threshold"
    # the shapes of a call
    assert out["power"].shape == (C, N, F) and out["power"].dtype == np.float32
    assert out["tone"].shape == (C, N) and out["tone"].dtype == np.int8
    assert out["open"].shape == (C, N) and out["open"].dtype == np.uint8
    assert out["y"].shape == (C, N * B) and out["fill"] == 3
    # power within the gate
    x64 = cs["x"][:, :N * B].astype(np.float64).reshape(C, N, B)
    ms = (x64 * x64).mean(axis=2).max(axis=1)
    pmax = p64.max(axis=(1, 2))
    scale = np.maximum(pmax, ms)
    err = np.abs(out["power"].astype(np.float64) - p64).max(axis=(1, 2))
    live = scale > 0
    assert (err[~live] == 0).all()                    # a row of zeros reads zeros
    rel = err[live] / scale[live]
    plain = live & (np.arange(C) != cs["strong"]) if C > 1 else np.zeros(C, bool)
    rel2 = (err[plain] / pmax[plain]).max() if plain.any() else float("nan")
    print(f"\ntonebank {shape}: worst power error {rel.max():.3e} of the row's scale, "
          f"{rel2:.3e} of the largest power on the plain rows")
    assert rel.max() <= GATE
    # tone and open: the numpy rule over the returned power, exactly; and the float64 reference's
    tone, opn, nxt, _ = M.decide(out["power"], FLOOR, DOM, cs["want"], hold, np.full(C, M.SAT))
    assert np.array_equal(out["tone"], tone) and np.array_equal(out["open"], opn)
    assert np.array_equal(out["tone"], cs["tone"]) and np.array_equal(out["open"], cs["open"])
    assert np.array_equal(out["state"], nxt)
    # the gated rows as bits
    assert np.array_equal(bits(out["y"]), bits(M.gate(cs["x"], opn, B)))


# ---------------------------------------------------------------- bit-identical across variations
@pytest.mark.parametrize("shape", SHAPES)
def test_cut_into_ten_uneven_calls(ld, shape):
    import torch
    C, F, B, hold = shape
    cs, out = run(*shape)
    K = cs["K"]
    rng = np.random.default_rng(11)
    cuts = np.sort(rng.choice(np.arange(1, K), 9, replace=False))
    cuts[0] = min(cuts[0], B // 2)                    # a first call too short for a block
    cuts = np.unique(np.concatenate([[0], cuts, [K]]))
    tb = make(ld, C, F, B, hold)
    xd = torch.tensor(cs["x"]).cuda()
    pw, tn, op, done = [], [], [], 0
    for i in range(len(cuts) - 1):
        piece = xd[:, cuts[i]:cuts[i + 1]]
        nb = tb.num_outputs(piece.shape[1])
        if i % 2:
            y = host(tb(piece))
            assert y.shape == (C, nb * B)
            assert np.array_equal(bits(y), bits(out["y"][:, done * B:(done + nb) * B])), i
        else:
            t, p = tb.measure(piece)
            assert t.shape == (C, nb) and p.shape == (C, nb, F)
        assert tb.fill == cuts[i + 1] % B
        done += nb
        pw.append(host(tb.power)), tn.append(host(tb.tone)), op.append(host(tb.open))
    got = dict(power=np.concatenate(pw, axis=1), tone=np.concatenate(tn, axis=1), open=np.concatenate(op, axis=1))
    same(got, out, "cut")
    assert np.array_equal(tb.state, out["state"])


@pytest.mark.parametrize("shape", SMALL)
def test_other_bank_sizes_row_order_strides_and_numpy(ld, shape):
    import torch
    C, F, B, hold = shape
    cs, out = run(*shape)
    x, K = cs["x"], cs["K"]
    # the rows reversed inside a bank of another size, an extra row first
    rows = np.arange(C)[::-1][:min(C, 100)]
    C2 = len(rows) + 1
    x2 = np.concatenate([np.full((1, K), 0.25, np.float32), x[rows]])
    tb = ld.ToneBank(C2, tones_for(F), block=B, dominance=DOM, floor=FLOOR, hold=hold,
                     want=np.concatenate([[-1], cs["want"][rows]]))
    y2 = host(tb(torch.from_numpy(x2).cuda()))
    got = dict(power=host(tb.power)[1:], tone=host(tb.tone)[1:], open=host(tb.open)[1:], y=y2[1:])
    same(got, {k: out[k][rows] for k in ("power", "tone", "open", "y")}, "bank")
    # a column slice of a wider tensor, rows 4 bytes off a 16-byte boundary
    wide = torch.zeros((C, K + 9), dtype=torch.float32, device="cuda")
    wide[:, 1:1 + K] = torch.tensor(x).cuda()
    view = wide[:, 1:1 + K]
    assert view.data_ptr() % 16 == 4 and (view.stride(0) * 4) % 16 == 0
    tb = make(ld, C, F, B, hold)
    got = dict(y=host(tb(view)), power=host(tb.power), tone=host(tb.tone), open=host(tb.open))
    same(got, out, "slice")
    # numpy input against the device tensor
    tb = make(ld, C, F, B, hold)
    y = tb(x)
    assert isinstance(y, np.ndarray) and isinstance(tb.power, np.ndarray)
    same(dict(y=y, power=tb.power, tone=tb.tone, open=tb.open), out, "numpy")
    t, p = tb.measure(x[:, :2 * B])                   # a second host call, from the carried tail
    assert t.shape == (C, 2) and p.shape == (C, 2, F)


def test_an_fmbank_output_read_in_place(ld):
    import torch
    C, F, B = 6, 5, 192
    fm = ld.FMBank(C, 0.25, 4)
    iq = torch.from_numpy(cgauss(np.random.default_rng(3), C * 8200).reshape(C, 8200)).cuda()
    a = fm(iq)
    assert a.dtype == torch.float32 and a.shape[0] == C
    tb = ld.ToneBank(C, tones_for(F), block=B, dominance=1.0, hold=1)
    y = host(tb(a))
    got = dict(y=y, power=host(tb.power), tone=host(tb.tone), open=host(tb.open))
    tb2 = ld.ToneBank(C, tones_for(F), block=B, dominance=1.0, hold=1)
    y2 = tb2(host(a).copy())
    same(got, dict(y=y2, power=tb2.power, tone=tb2.tone, open=tb2.open), "fmbank")
    assert got["power"].shape[1] == a.shape[1] // B and (got["power"] > 0).all()


# ---------------------------------------------------------------- settings and state
@pytest.mark.parametrize("shape", [(3, 5, 192, 1), (16, 33, 1024, 2)])
def test_settings_change_the_next_block_and_reset_restores(ld, shape):
    import torch
    C, F, B, hold = shape
    cs, out = run(*shape)
    xd = torch.tensor(cs["x"]).cuda()
    tb = make(ld, C, F, B, hold)
    cut = B * (cs["N"] // 2) + 17
    n1 = cut // B
    y1 = host(tb(xd[:, :cut]))
    first = dict(power=host(tb.power), tone=host(tb.tone), open=host(tb.open), y=y1)
    same(first, {k: out[k][:, :n1] for k in ("power", "tone", "open")} | {"y": out["y"][:, :n1 * B]}, "first half")
    since = tb.state.copy()
    want2 = (cs["want"] + 1) % F
    tb.want, tb.dominance, tb.floor = want2, 2.0, 0.015
    assert np.array_equal(tb.state, since) and tb.fill == cut % B      # no state touched
    y2 = host(tb(xd[:, cut:]))
    p2 = host(tb.power)
    assert np.array_equal(bits(p2), bits(out["power"][:, n1:]))         # the powers do not depend on them
    tone, opn, nxt, _ = M.decide(p2, 0.015, 2.0, want2, hold, since)
    assert np.array_equal(host(tb.tone), tone) and np.array_equal(host(tb.open), opn)
    assert not np.array_equal(opn, out["open"][:, n1:])                 # and they did change something
    assert np.array_equal(bits(y2), bits(M.gate(cs["x"][:, n1 * B:], opn, B)))
    assert np.array_equal(tb.state, nxt)
    tb.reset()
    assert tb.fill == 0 and (tb.state == M.SAT).all()
    tb.want, tb.dominance, tb.floor = cs["want"], DOM, FLOOR
    again = dict(y=host(tb(xd[:, :cut])), power=host(tb.power), tone=host(tb.tone), open=host(tb.open))
    same(again, first, "reset")


# ---------------------------------------------------------------- a clean tone
@pytest.mark.parametrize("A", [1.0, 0.01])
def test_a_clean_tone_reads_half_its_amplitude_squared(ld, A):
    """Sub-audible tones a few cycles per block, the CTCSS regime: the definition's own deviation
    from A^2 / 2 (the image at -f through the window's side lobes, the table's rounding) is
    computed in float64 and the kernel must stay within twice that."""
    C, B = 4, 256
    f = np.array([3.3, 4.7, 6.2, 8.4]) / B
    tb = ld.ToneBank(C, f, block=B)
    i = np.arange(3 * B, dtype=np.float64)
    x = np.stack([A * np.cos(2 * np.pi * f[k] * i + 0.3 * k) for k in range(C)]).astype(np.float32)
    tone, p = tb.measure(x)
    p64 = M.power64(tb.tables, x)
    for k in range(C):
        dev = np.abs(p64[k, :, k] - A * A / 2)
        got = np.abs(p[k, :, k].astype(np.float64) - A * A / 2)
        print(f"\ntonebank clean tone A = {A}, f = {f[k] * B:.1f} / B: definition off by "
              f"{(dev / (A * A / 2)).max():.3e}, kernel by {(got / (A * A / 2)).max():.3e}")
        assert (got <= 2 * dev).all()
        assert (tone[k] == k).all()


# ---------------------------------------------------------------- non-finite input
@pytest.mark.parametrize("shape", [(3, 5, 192, 1), (5, 64, 4096, 3)])
def test_a_nan_and_an_inf_stay_in_their_blocks(ld, shape):
    import torch
    C, F, B, hold = shape
    cs, out = run(*shape)
    x = cs["x"].copy()
    N = cs["N"]
    bn, bi = N // 2, N // 2 + 5                       # a NaN in row 0, an Inf in the last row
    x[0, bn * B + B // 3] = np.nan
    x[C - 1, bi * B + B // 2] = np.inf
    tb = make(ld, C, F, B, hold)
    y = host(tb(torch.from_numpy(x).cuda()))
    p, tn, op = host(tb.power), host(tb.tone), host(tb.open)
    hit = np.zeros((C, N), bool)
    hit[0, bn] = hit[C - 1, bi] = True
    assert not np.isfinite(p[hit]).any() and (tn[hit] == -1).all()
    assert np.array_equal(bits(p[~hit]), bits(out["power"][~hit]))
    assert np.array_equal(tn[~hit], out["tone"][~hit])
    # the block is not accepted: open there only by hold, and the rule over the returned powers holds everywhere
    tone, opn, _, acc = M.decide(p, FLOOR, DOM, cs["want"], hold, np.full(C, M.SAT))
    assert not acc[hit].any() and np.array_equal(op, opn) and np.array_equal(tn, tone)
    far = np.ones((C, N), bool)
    for c, b in ((0, bn), (C - 1, bi)):
        far[c, b:b + hold + 1] = False                # blocks whose window holds the struck one
    assert np.array_equal(op[far], out["open"][far])
    yb, yo = bits(y).reshape(C, N, B), bits(out["y"]).reshape(C, N, B)
    assert np.array_equal(yb[far], yo[far])
    assert np.array_equal(bits(y), bits(M.gate(x, opn, B)))
