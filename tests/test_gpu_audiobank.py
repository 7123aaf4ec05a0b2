"""AudioBank on the GPU: de-emphasis and the polyphase resampler over bank rows
(k_audiobank.hip) against its definition,

    e[c][t] = b0 sum_{j>=0} a^j u[c][t-j]            (de-emphasis off: e = u)
    y[c][k] = sum_{n<2len} h_{b_k}[n] e[c][j_k - n],  out = y * scale  (or its int16 rounding)

evaluated here in float64 over the float32 input with the object's own a, b0,
taps and schedule; the schedule (j_k, b_k) is computed from step, phase and
nfilter by SURVEY App. A.3's closed form.  Rows are seeded noise (a different
seed per row) and, where there is room, one row that is 0 throughout, one
constant row of 1.0 and one tone.  Sizes come from the kernel's tile:
K = ceil((2 tile + 1) / rate) + 3 samples per row is two full tiles, a
one-output tile and a ragged tail.  The gate of 1e-6 per row is the project's
gate for FIR-class kernels.  Without de-emphasis every row must
carry RealResampler's bits; streams cut into calls, banks of other sizes and
row orders, inputs read in place and the PCM rounding are compared bitwise."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GATE = 1e-6
RESAMP = [(0.192, 20, 13), (1 / 32, 7, 64), (2.5, 4, 16)]                     # (rate, len, nfilter)
# (C, rate, len, nfilter, sample_rate, tau)
DEFN = [(1, 0.192, 20, 13, 250e3, 75e-6), (3, 0.12, 32, 16, 400e3, 75e-6), (16, 1 / 32, 7, 64, 48e3, 75e-6),
        (64, 0.5, 12, 32, 426e3, 75e-6), (256, 0.192, 20, 13, 200e3, 50e-6), (5, 2.5, 4, 16, 100e3, 75e-6)]


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype == np.float32 else np.uint16)


def default_fc(rate):
    return np.float32(0.45 * min(float(np.float32(rate)), 1.0))


def samples_for(ab):
    return math.ceil((2 * ab.tile + 1) / ab.rate) + 3


def rows_for(seed, C, K):
    """C rows of K samples: seeded noise with a seed offset per row; where there is room the
    second row is 0 throughout, the third a constant 1.0 and the fourth a tone."""
    x = np.stack([np.random.default_rng(seed + 17 * c).standard_normal(K).astype(np.float32) for c in range(C)])
    if C >= 2:
        x[1] = 0
    if C >= 3:
        x[2] = 1.0
    if C >= 4:
        x[3] = np.cos(2 * np.pi * ((0.0371 * np.arange(K)) % 1.0)).astype(np.float32)
    return x


def schedule(step, phase, npfb, K):
    """App. A.3: output k's window ends at input j_k, the smallest j >= 0 with
    phase + k step - j 2^24 <= 2^24 - 1, on branch b_k = (that phase) >> (24 - log2 npfb);
    a call of K samples returns the outputs with j_k <= K - 1."""
    last = ((K - 1) << 24) + 0xffffff - phase
    nout = last // step + 1 if K > 0 and last >= 0 else 0
    acc = phase + np.arange(nout, dtype=np.int64) * step
    j = acc >> 24
    b = (acc & 0xffffff) >> (24 - int(math.log2(npfb)))
    assert ((b >= 0) & (b < npfb)).all() and (j < max(K, 1)).all()
    return j, b


def definition(ab, u):
    """The definition in float64 over the float32 rows u, from the start of the stream."""
    u = np.asarray(u).astype(np.float64)
    C, K = u.shape
    b0, a = (float(v) for v in ab.coefs)
    if ab.deemphasis is None:
        e = u
    else:
        e = np.empty_like(u)
        v = np.zeros(C)
        for t in range(K):
            v = u[:, t] + a * v
            e[:, t] = b0 * v
    npfb, L = ab.nfilter, 2 * ab.len
    j, b = schedule(ab.step, 0, npfb, K)
    h = ab.taps.astype(np.float64)
    n = np.arange(L)
    ep = np.concatenate([np.zeros((C, L)), e], axis=1)                         # ep[:, t + L] = e[:, t]
    y = np.einsum("ckn,kn->ck", ep[:, (j[:, None] - n[None, :]) + L], h[b[:, None] + n[None, :] * npfb])
    return y * float(ab.scale)


def per_row_err(y, ref):
    den = np.max(np.abs(ref), axis=1)
    return np.max(np.abs(y - ref), axis=1) / np.where(den > 0, den, 1.0)


def pcm(z):
    return np.clip(np.rint(z * np.float32(32767)), -32768, 32767).astype(np.int16)


# ---------------------------------------------------------------- 1. the resampler alone: RealResampler's bits
@pytest.mark.parametrize("rate,m,npfb", RESAMP)
@pytest.mark.parametrize("C", [1, 3, 16])
def test_resampler_alone_bits(ld, ora, C, rate, m, npfb):
    ab = ld.AudioBank(C, rate, m, nfilter=npfb)
    fc = default_fc(rate)
    K = samples_for(ab)
    x = rows_for(100 + C, C, 2 * K - 5)
    rs = [ld.RealResampler(rate, m, fc, 60.0, npfb) for _ in range(C)]
    oras = [ora.Resampler(rate, m, fc, 60.0, npfb, cplx=False) for _ in range(C)]
    for part in (x[:, :K], x[:, K:]):                # the second call starts from a carried phase and history
        want = ab.num_outputs(part.shape[1])
        y = ab(part)
        assert y.dtype == np.float32 and y.shape == (C, want)
        for c in range(C):
            row = np.ascontiguousarray(part[c])
            a, b = rs[c](row), oras[c](row)
            assert a.shape == b.shape == (want,), c
            assert (bits(y[c]) == bits(a)).all(), c
            assert (bits(y[c]) == bits(b)).all(), c
        assert ab.phase == oras[0].phase


# ---------------------------------------------------------------- 2. the definition
@pytest.mark.parametrize("C,rate,m,npfb,sr,tau", DEFN)
def test_parity_with_definition(ld, ora, C, rate, m, npfb, sr, tau):
    ab = ld.AudioBank(C, rate, m, nfilter=npfb, deemphasis=sr, tau=tau)
    K = samples_for(ab)
    x = rows_for(1000 + 7 * C, C, K)
    y = ab(x)
    want = len(ora.Resampler(rate, m, default_fc(rate), 60.0, npfb, cplx=False)(np.zeros(K, np.float32)))
    assert y.dtype == np.float32 and y.shape == (C, want) and want >= 2 * ab.tile + 1
    assert len(schedule(ab.step, 0, ab.nfilter, K)[0]) == want
    err = per_row_err(y, definition(ab, x))
    print(f"C={C} rate={rate:.4g} len={m} sr={sr:g} tau={tau:g} tile={ab.tile}: worst row {int(np.argmax(err))} "
          f"{err.max():.3g}")
    assert err.max() <= GATE, (int(np.argmax(err)), float(err.max()))
    if C >= 2:
        assert not y[1].any()                        # zeros in, zeros out


# ---------------------------------------------------------------- 3. cuts and reset
@pytest.mark.parametrize("rate,m,npfb,sr", [(0.192, 20, 13, 250e3), (1 / 32, 7, 64, 48e3), (2.5, 4, 16, 100e3),
                                            (0.192, 20, 13, None)])
def test_cuts_and_reset_bitwise(ld, rate, m, npfb, sr):
    C = 4
    ab = ld.AudioBank(C, rate, m, nfilter=npfb, deemphasis=sr)
    K = samples_for(ab)
    x = rows_for(2000, C, K)
    whole = ab(x)
    cut = ld.AudioBank(C, rate, m, nfilter=npfb, deemphasis=sr)
    parts, at = [], 0
    for n in (0, 1, 2, max(int(1 / rate) - 1, 0), ab.tile, K):
        n = min(n, K - at)
        want = cut.num_outputs(n)
        parts.append(cut(x[:, at:at + n]))
        assert parts[-1].shape == (C, want)
        at += n
    assert at == K
    got = np.concatenate(parts, axis=1)
    assert got.shape == whole.shape and (bits(got) == bits(whole)).all()
    ab.reset()
    assert ab.phase == 0 and (bits(ab(x)) == bits(whole)).all()


# ---------------------------------------------------------------- 4. rows
@pytest.mark.parametrize("sr", [250e3, None])
def test_rows_do_not_depend_on_the_bank(ld, sr):
    mk = lambda C: ld.AudioBank(C, 0.192, deemphasis=sr)
    K = samples_for(mk(16))
    x = rows_for(3000, 16, K)
    y = mk(16)(x)
    assert (bits(mk(1)(x[7:8])) == bits(y[7:8])).all()
    perm = [11, 3, 0, 15, 2]
    assert (bits(mk(5)(x[perm])) == bits(y[perm])).all()
    big = rows_for(3100, 64, K)
    where = np.random.default_rng(5).permutation(64)[:16]
    big[where] = x
    assert (bits(mk(64)(big)[where]) == bits(y)).all()


# ---------------------------------------------------------------- 5. inputs read in place
@pytest.mark.parametrize("sr", [250e3, None])
def test_in_place_reads_bitwise(ld, sr):
    import torch
    C = 5
    mk = lambda: ld.AudioBank(C, 0.192, deemphasis=sr)
    K = samples_for(mk())
    x = rows_for(4000, C + 3, K + 11)
    want_cols = mk()(np.ascontiguousarray(x[:C, 4:4 + K]))
    want_rows = mk()(np.ascontiguousarray(x[2:2 + C]))
    xd = torch.from_numpy(x).to("cuda:0")
    got = mk()(xd[:C, 4:4 + K])                      # a column range: row stride K + 11
    assert got.is_cuda and got.dtype == torch.float32
    assert (bits(got.cpu().numpy()) == bits(want_cols)).all()
    got = mk()(xd[2:2 + C])                          # a row block
    assert (bits(got.cpu().numpy()) == bits(want_rows)).all()
    got = mk()(xd[:C, 4:4 + K].contiguous())         # a device tensor against numpy
    assert (bits(got.cpu().numpy()) == bits(want_cols)).all()
    with pytest.raises(ValueError):
        mk()(xd[:C, ::2])


def test_fmbank_output_fed_as_it_is(ld):
    import torch
    from conftest import cgauss
    C = 16
    fm = ld.FMBank(C, 0.25, 4)
    ab = ld.AudioBank(C, 0.192, deemphasis=250e3)
    n = 4 * samples_for(ab)
    x = np.stack([cgauss(np.random.default_rng(4500 + c), n) for c in range(C)])
    d = fm(torch.from_numpy(x).to("cuda:0"))
    want_n = ab.num_outputs(d.shape[1])
    y = ab(d)
    assert y.is_cuda and tuple(y.shape) == (C, want_n) and want_n >= 2 * ab.tile
    want = ld.AudioBank(C, 0.192, deemphasis=250e3)(d.cpu().numpy())
    assert (bits(y.cpu().numpy()) == bits(want)).all()


# ---------------------------------------------------------------- 6. PCM16
@pytest.mark.parametrize("scale", [0.5, 40.0])
def test_pcm16_is_the_rounding_of_the_float_bank(ld, scale):
    import torch
    C = 5
    f = ld.AudioBank(C, 0.192, deemphasis=250e3)
    p = ld.AudioBank(C, 0.192, deemphasis=250e3, pcm16=True)
    f.scale = p.scale = scale
    x = rows_for(5000, C, samples_for(f))
    z, y = f(x), p(x)
    assert y.dtype == np.int16 and y.shape == z.shape
    want = pcm(z)
    assert (want == 32767).any() == (scale == 40.0) and (want == -32768).any() == (scale == 40.0)
    assert (y == want).all()
    p.reset()
    yd = p(torch.from_numpy(x).to("cuda:0"))
    assert yd.dtype == torch.int16 and (yd.cpu().numpy() == want).all()
