"""FMBank on the GPU: the discriminator and decimating FIR over bank rows
(k_fmbank.hip) against its definition,

    d[c][t] = lm_atan2f(im, re) * ref,  (re, im) = conj(x[c][t-1]) * x[c][t]
    y[c][n] = scale * sum_{j<L} h[j] d[c][nD - j]          (d = 0 before t = 0)

evaluated here in float64 over the float32 d of the restatement's freqdem, with
the object's own taps and scale.  Rows are seeded noise (a different seed per
row), one row that is 0 throughout and one constant-frequency tone; sizes come
from the kernel's tile (F output columns per workgroup): one call of
D (2F + 1) + 3 samples per row is two full tiles, a one-column tile and a
ragged tail.  The gate of 1e-6 per row is the project's gate for FIR-class
kernels.  The discriminator alone must carry FreqDem's bits;
streams cut into calls, banks of other sizes and row orders, and inputs read in
place must give the same bits."""
import numpy as np
import pytest

from conftest import cgauss

pytestmark = pytest.mark.gpu

GATE = 1e-6
KF = 0.25
SHAPES = [(1, 2, 6), (3, 5, 4), (16, 8, 6), (5, 64, 8), (64, 4, 2), (256, 3, 1)]   # (C, D, m)


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def rows_for(seed, C, K):
    """C rows of K samples: seeded noise with a seed offset per row; where there is room the
    second row is 0 throughout and the third a constant-frequency tone."""
    x = np.stack([cgauss(np.random.default_rng(seed + 17 * c), K) for c in range(C)])
    if C >= 2:
        x[1] = 0
    if C >= 3:
        x[2] = np.exp(2j * np.pi * ((0.0371 * np.arange(K)) % 1.0)).astype(np.complex64)
    return x


def disc(ora, x, kf=KF):
    """The restatement's freqdem per row, from a fresh object (the sample before t = 0 is 0)."""
    return np.stack([ora.FreqDem(kf)(np.ascontiguousarray(r)) for r in x])


def definition(d, h, scale, D):
    """The definition in float64 over the float32 discriminator rows d."""
    d = np.asarray(d).astype(np.float64)
    h = np.asarray(h).astype(np.float64)
    L, K = h.size, d.shape[1]
    ncols = -(-K // D)
    dp = np.concatenate([np.zeros((d.shape[0], L - 1)), d], axis=1)           # dp[:, t + L - 1] = d[:, t]
    idx = (np.arange(ncols)[:, None] * D - np.arange(L)[None, :]) + L - 1     # [ncols][L]
    return float(scale) * np.einsum("cnl,l->cn", dp[:, idx], h)


def per_row_err(y, ref):
    den = np.max(np.abs(ref), axis=1)
    return np.max(np.abs(y - ref), axis=1) / np.where(den > 0, den, 1.0)


# ---------------------------------------------------------------- 1. the discriminator alone: FreqDem's bits
@pytest.mark.parametrize("C", [1, 3, 16])
def test_discriminator_bits(ld, ora, C):
    fb = ld.FMBank(C, KF)
    K = 2 * fb.tile + 1 + 3
    x = rows_for(100 + C, C, 2 * K)
    if C == 1:
        x[0, 5:9] = 0                                # zeros inside a noise row as well
    dems = [ld.FreqDem(KF) for _ in range(C)]
    oras = [ora.FreqDem(KF) for _ in range(C)]
    for part in (x[:, :K], x[:, K:]):                # the second call carries each row's previous sample
        y = fb(part)
        assert y.dtype == np.float32 and y.shape == (C, K)
        for c in range(C):
            row = np.ascontiguousarray(part[c])
            assert (bits(y[c]) == bits(dems[c](row))).all(), c
            assert (bits(y[c]) == bits(oras[c](row))).all(), c
    z = ld.FMBank(2, KF)(np.zeros((2, 40), np.complex64))
    assert (bits(z) == bits(ora.FreqDem(KF)(np.zeros(40, np.complex64)))[None, :]).all()


# ---------------------------------------------------------------- 2. the definition
@pytest.mark.parametrize("C,D,m", SHAPES)
def test_parity_with_definition(ld, ora, C, D, m):
    fb = ld.FMBank(C, KF, D, m=m)
    F = fb.tile
    K = D * (2 * F + 1) + 3
    x = rows_for(1000 + 7 * C + D, C, K)
    y = fb(x)
    assert y.dtype == np.float32 and y.shape == (C, -(-K // D))
    err = per_row_err(y, definition(disc(ora, x), fb.taps, fb.scale, D))
    print(f"C={C} D={D} m={m} F={F}: worst row {int(np.argmax(err))} {err.max():.3g}")
    assert err.max() <= GATE, (int(np.argmax(err)), float(err.max()))


@pytest.mark.parametrize("D,L", [(8, 3), (4, 37), (64, 17 * 64), (8, 1), (8, 2), (1, 4), (32, 5)])
def test_user_taps_against_definition(ld, ora, D, L):
    """A prototype shorter than D, one that ends inside a phase and the longest supported; then one tap (no
    history), two, a prototype at decimation 1 and one far shorter than a large D."""
    rng = np.random.default_rng(1500 + L)
    h = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
    fb = ld.FMBank(5, KF, D, taps=h)
    fb.scale = 0.5
    x = rows_for(1600 + L, 5, D * (2 * fb.tile + 1) + 3)
    y = fb(x)
    err = per_row_err(y, definition(disc(ora, x), h, 0.5, D))
    print(f"D={D} L={L}: worst row {int(np.argmax(err))} {err.max():.3g}")
    assert err.max() <= GATE, (int(np.argmax(err)), float(err.max()))


# ---------------------------------------------------------------- 3. cuts
@pytest.mark.parametrize("C,D,m", [(3, 5, 4), (16, 8, 6), (5, 64, 8), (2, 1, 0)])
def test_streaming_is_bitwise_invariant(ld, C, D, m):
    """m = 0: the discriminator alone."""
    fb = ld.FMBank(C, KF, D, m=m) if m else ld.FMBank(C, KF)
    F = fb.tile
    lens = [0, 1, D - 1, D, D + 1, F * D - 1, 0, F * D, F * D + 1]
    K = sum(lens) + 2 * D + 3                        # the rest
    lens.append(K - sum(lens))
    x = rows_for(3000 + D, C, K)
    whole = fb(x)
    assert whole.shape == (C, -(-K // D)) and fb.skip == (-K) % D
    fb.reset()
    assert fb.skip == 0
    again = fb(x)
    assert (bits(again) == bits(whole)).all()        # reset, then the same stream: the first result's bits
    fb.reset()
    parts, at = [], 0
    for n in lens:
        want = fb.num_outputs(n)
        p = fb(x[:, at:at + n])
        assert p.shape == (C, want), (n, p.shape, want)
        parts.append(p)
        at += n
    cut = np.concatenate(parts, axis=1)
    assert cut.shape == whole.shape
    assert (bits(cut) == bits(whole)).all()


# ---------------------------------------------------------------- 4. rows are independent
@pytest.mark.parametrize("D,m", [(8, 6), (1, 0)])
def test_rows_are_independent(ld, D, m):
    make = (lambda C: ld.FMBank(C, KF, D, m=m)) if m else (lambda C: ld.FMBank(C, KF))
    fb = make(16)
    K = D * (2 * fb.tile + 1) + 3
    x = rows_for(4000 + D, 16, K)
    y = fb(x)
    for r in (0, 1, 2, 7, 15):
        one = make(1)(x[r:r + 1])
        assert (bits(one[0]) == bits(y[r])).all(), r
        rev = make(r + 1)(x[r::-1])                  # rows r, r - 1, .. 0: row r comes first
        assert (bits(rev[0]) == bits(y[r])).all(), r
    full_rev = make(16)(x[::-1])
    assert (bits(full_rev[::-1]) == bits(y)).all()
    assert (bits(make(1)(x[5])) == bits(y[5:6])).all()       # a 1-D input when nchan is 1


# ---------------------------------------------------------------- 5. in place
def test_inputs_read_in_place(ld):
    import torch
    D, C = 8, 5
    fb = ld.FMBank(C, KF, D)
    K = D * (2 * fb.tile + 1) + 3
    x = rows_for(5000, C, K)
    want = fb(x)
    # a column slice of a wider tensor: row stride above K
    wide = torch.from_numpy(np.concatenate([rows_for(5100, C, 7), x, rows_for(5200, C, 5)], axis=1)).to("cuda:0")
    view = wide[:, 7:7 + K]
    assert view.stride() == (K + 12, 1) and not view.is_contiguous()
    fb.reset()
    got = fb(view)
    assert got.is_cuda and got.dtype == torch.float32 and tuple(got.shape) == want.shape
    assert (bits(got.cpu().numpy()) == bits(want)).all()
    # the contiguous copy of the same view
    fb.reset()
    assert (bits(fb(view.contiguous()).cpu().numpy()) == bits(want)).all()
    # a numpy Fortran-ordered array against its C-ordered copy
    fb.reset()
    xf = np.asfortranarray(x)
    assert xf.flags.f_contiguous and not xf.flags.c_contiguous
    assert (bits(fb(xf)) == bits(want)).all()
    # a non-unit column stride is refused and leaves the state as it was
    fb.reset()
    with pytest.raises(ValueError):
        fb(wide[:, ::2][:, :K // 2])
    with pytest.raises(ValueError):
        fb(torch.from_numpy(x).to("cuda:0").t().contiguous().t())
    assert fb.skip == 0
    assert (bits(fb(view).cpu().numpy()) == bits(want)).all()


def test_rows_of_a_channelizer_output_in_place(ld):
    import torch
    ch = ld.Channelizer(16)
    n = 16 * 700
    xs = torch.from_numpy(cgauss(np.random.default_rng(5300), n)).to("cuda:0")
    rows = ch(xs)
    K = rows.shape[1]
    sl = rows[3:8]
    assert sl.data_ptr() != rows.data_ptr() and sl.stride(1) == 1
    a = ld.FMBank(5, KF, 4)(sl)
    b = ld.FMBank(5, KF, 4)(sl.clone())
    c = ld.FMBank(5, KF, 4)(sl.cpu().numpy())
    assert tuple(a.shape) == (5, -(-K // 4))
    assert (bits(a.cpu().numpy()) == bits(b.cpu().numpy())).all()
    assert (bits(a.cpu().numpy()) == bits(c)).all()


# ---------------------------------------------------------------- 6. sign and scale
def test_sign_and_scale_of_a_tone(ld):
    """exp(2 pi i f t) demodulates to f / kf: a wrong sign, a missing 2 pi or a wrong scale is off
    by 100 % or more, so the 1e-4 margin says nothing about accuracy (the definition tests do)."""
    f, kf, D = 0.0371, 0.25, 8
    fb = ld.FMBank(1, kf, D)
    K = D * (2 * fb.tile + 1) + 3
    x = np.exp(2j * np.pi * ((f * np.arange(K)) % 1.0)).astype(np.complex64)[None, :]
    y = fb(x)[0]
    settled = y[-(-len(fb.taps) // D):]
    assert settled.size > fb.tile
    assert np.max(np.abs(settled / (f / kf) - 1.0)) <= 1e-4, float(np.max(np.abs(settled / (f / kf) - 1.0)))


# ---------------------------------------------------------------- 7. errors and state
def test_row_mismatch_leaves_the_state(ld):
    D = 8
    x = rows_for(7000, 4, D * 40 + 3)
    fb = ld.FMBank(4, KF, D)
    for bad in (x[:3], np.concatenate([x, x[:1]]), x[0]):
        with pytest.raises(ValueError):
            fb(bad)
    import torch
    with pytest.raises(ValueError):
        fb(torch.from_numpy(x[:2]).to("cuda:0"))
    assert fb.skip == 0
    assert (bits(fb(x)) == bits(ld.FMBank(4, KF, D)(x))).all()


def test_scale_takes_effect_on_the_next_call(ld):
    D = 8
    x = rows_for(7100, 3, D * 60)
    a, b = ld.FMBank(3, KF, D), ld.FMBank(3, KF, D)
    half = x.shape[1] // 2
    y0 = a(x[:, :half])
    assert (bits(y0) == bits(b(x[:, :half]))).all()
    a.scale = 2.0 * b.scale                          # a power of two: the products double exactly
    y1, r1 = a(x[:, half:]), b(x[:, half:])
    assert (bits(y1) == bits(2.0 * r1)).all()
    assert not (bits(y1) == bits(r1)).all()
    assert (bits(y0) == bits(ld.FMBank(3, KF, D)(x[:, :half]))).all()      # what was returned stays as it was
