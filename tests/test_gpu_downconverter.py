"""Downconverter on the GPU: the tuned decimating bank (k_ddc.hip) against its
definition, evaluated here in float64 with the object's own taps, scale and
frequency words and the phase reduced in integers,

    y[c][n] = scale * sum_{j<L} h[j] x[nD - j] exp(-2 pi i (((nD - j) w_c) mod 2^32) / 2^32)

with zeros before the stream's first sample.  Sizes come from the kernel's tile
(F output columns per workgroup): one call of D (2F + 1) + 3 samples is two full
tiles, a one-column tile and a ragged tail.  The gate of 1e-6 per row is the
project's gate for FIR-class kernels; streams cut into calls,
banks of other sizes and orders, and retuned banks must give the same bits."""
import numpy as np
import pytest

from conftest import cgauss

pytestmark = pytest.mark.gpu

GATE = 1e-6
SHAPES = [(1, 2, 6), (3, 5, 6), (4, 8, 8), (5, 100, 4), (16, 64, 6), (64, 32, 2), (2, 256, 8)]   # (C, D, m)
# the other side of the tile classes (D = 256 at 64 columns, D < 256 at 32), and a two-tuner block at the defaults
SHAPES += [(3, 256, 2), (3, 240, 8), (2, 16, 6)]


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def definition(x, h, scale, words, D, T=0):
    """The definition in float64 for the call that delivers samples T .. T + len(x) - 1 after a
    seek to T (zeros before T); the phase ((nD - j) w) mod 2^32 is reduced in integers."""
    x = np.asarray(x).astype(np.complex128)
    h = np.asarray(h).astype(np.float64)
    L, N = h.size, x.size
    n0 = -(-T // D)
    ncols = max(0, -(-(T + N - n0 * D) // D))
    xp = np.concatenate([np.zeros(L - 1, np.complex128), x])                  # xp[i + L - 1] = sample T + i
    t = [[(n0 + n) * D - j for j in range(L)] for n in range(ncols)]          # Python integers
    idx = np.array([[v - T for v in row] for row in t], np.int64).reshape(ncols, L)
    tm = np.array([[v % 2 ** 32 for v in row] for row in t], np.uint64).reshape(ncols, L)
    assert ncols == 0 or idx.max() < N
    wx = xp[np.maximum(idx, -(L - 1)) + L - 1] * h[None, :]
    y = np.empty((len(words), ncols), np.complex128)
    for c, w in enumerate(words):
        ph = (tm * np.uint64(int(w))) % np.uint64(2 ** 32)                    # < 2^64 before the reduction
        y[c] = float(scale) * np.sum(wx * np.exp(-2j * np.pi * (ph.astype(np.float64) / 2.0 ** 32)), axis=1)
    return y


def per_row_err(y, ref):
    return np.max(np.abs(y - ref), axis=1) / np.max(np.abs(ref), axis=1)


def freqs_for(rng, C, M=16):
    """0, -0.5, 2^-32, a k / M value, then seeded values in [-0.5, 0.5)."""
    f = [0.0, -0.5, 2.0 ** -32, 3 / M] + list(rng.uniform(-0.5, 0.5, max(C, 5)))
    if C < 5:                                        # small banks: what fits, the seeded value last
        f = (f[:C - 1] + [f[4]]) if C > 1 else [f[4]]
    return f[:C]


# ---------------------------------------------------------------- 1. parity with the definition
@pytest.mark.parametrize("C,D,m", SHAPES)
def test_parity_with_definition(ld, C, D, m):
    rng = np.random.default_rng(1000 + 7 * C + D)
    f = freqs_for(rng, C)
    dc = ld.Downconverter(f, D, m=m)
    F = dc.tile
    N = D * (2 * F + 1) + 3
    x = cgauss(rng, N)
    y = dc(x)
    assert y.dtype == np.complex64 and y.shape == (C, -(-N // D))
    err = per_row_err(y, definition(x, dc.taps, dc.scale, dc.words, D))
    print(f"C={C} D={D} m={m} F={F}: worst row {int(np.argmax(err))} {err.max():.3g}")
    assert err.max() <= GATE, (int(np.argmax(err)), float(err.max()))


def test_parity_special_frequencies_one_tuner_each(ld):
    """The special frequencies as banks of one (the one-tuner kernel), D = 2."""
    rng = np.random.default_rng(1100)
    for f in (0.0, -0.5, 2.0 ** -32, 3 / 16):
        dc = ld.Downconverter(f, 2)
        x = cgauss(rng, 2 * (2 * dc.tile + 1) + 3)
        y = dc(x)
        err = per_row_err(y, definition(x, dc.taps, dc.scale, dc.words, 2))
        print(f"f={f}: {err.max():.3g}")
        assert err.max() <= GATE


# ---------------------------------------------------------------- 2. user taps
@pytest.mark.parametrize("D,L", [(8, 3), (4, 37), (64, 17 * 64), (8, 1), (8, 2), (8, 7), (8, 9), (32, 5)])
def test_user_taps_against_definition(ld, D, L):
    """A prototype shorter than D, one that ends inside a phase and the longest supported; then those around
    the eight waves' parts of ceil(L / 8): no history and seven idle waves, two taps, one tap in each of seven
    waves, parts of two with the last three waves idle, and L far below the largest D of the bank demodulators."""
    rng = np.random.default_rng(1500 + L)
    h = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
    dc = ld.Downconverter(freqs_for(rng, 5), D, taps=h)
    dc.scale = 0.5
    x = cgauss(rng, D * (2 * dc.tile + 1) + 3)
    y = dc(x)
    err = per_row_err(y, definition(x, h, 0.5, dc.words, D))
    print(f"D={D} L={L}: worst row {err.max():.3g}")
    assert err.max() <= GATE


# ---------------------------------------------------------------- 3. direction of the mix
def test_direction_of_the_mix(ld):
    D = 16
    dc = ld.Downconverter([0.0371, -0.0371], D)
    f1 = float(dc.words[0]) / 2.0 ** 32
    assert int(dc.words[1]) == 2 ** 32 - int(dc.words[0])
    N = D * (2 * dc.tile + 1) + 3
    t = np.arange(N)
    x = (np.exp(2j * np.pi * ((t * f1) % 1.0)) + cgauss(np.random.default_rng(2000), N, 1e-3)).astype(np.complex64)
    y = dc(x)
    settled = y[:, -(-len(dc.taps) // D):]           # past the prototype's rise
    print(f"means {np.mean(settled, axis=1)}")
    assert abs(np.mean(settled[0]) - 1.0) <= 1e-2
    assert abs(np.mean(settled[1])) <= 1e-2 and np.max(np.abs(settled[1])) <= 1e-2


# ---------------------------------------------------------------- 4. streaming invariance, bitwise
@pytest.mark.parametrize("C,D,m", [(3, 5, 6), (16, 64, 6), (2, 256, 8)])
def test_streaming_is_bitwise_invariant(ld, C, D, m):
    rng = np.random.default_rng(3000 + D)
    dc = ld.Downconverter(freqs_for(rng, C), D, m=m)
    F, L = dc.tile, len(dc.taps)
    forced = [0, 1, D - 1, D + 1, F * D - 1, F * D, F * D + 1, L - 2]
    seeded = [int(v) for v in rng.integers(1, 3 * D + 2, 6)]
    lens = [seeded[0], *forced[:4], seeded[1], *forced[4:6], seeded[2], seeded[3], *forced[6:], seeded[4], seeded[5]]
    lens.append(2 * D + 1)                          # something after the last forced cut
    x = cgauss(rng, sum(lens))
    whole = dc(x)
    assert dc.skip == (-x.size) % D
    dc.reset()
    assert dc.skip == 0
    parts, T = [], 0
    for c in lens:
        want = dc.num_outputs(c)
        skip = (-T) % D
        assert want == (-(-(c - skip) // D) if c > skip else 0)
        y = dc(x[T:T + c])
        assert y.shape == (C, want), (c, y.shape, want)
        T += c
        assert dc.skip == (-T) % D
        parts.append(y)
    got = np.concatenate(parts, axis=1)
    assert got.shape == whole.shape
    assert np.array_equal(bits(got), bits(whole))


# ---------------------------------------------------------------- 5. reset
def test_reset_reproduces_the_first_output(ld):
    dc = ld.Downconverter([0.0371, -0.31337, 0.25], 8)
    x = cgauss(np.random.default_rng(4000), 8 * dc.tile + 13)
    first = dc(x)
    dc(x[:37])                                       # leaves skip != 0 behind
    assert dc.skip != 0
    dc.reset()
    assert np.array_equal(bits(dc(x)), bits(first))


# ---------------------------------------------------------------- 6. rows do not depend on the other tuners
def test_rows_are_independent_bitwise(ld):
    D = 12
    rng = np.random.default_rng(4500)
    f = freqs_for(rng, 7)
    bank = ld.Downconverter(f, D)
    x = cgauss(rng, D * (2 * bank.tile + 1) + 3)
    y = bank(x)
    for c in range(7):                               # the one-tuner kernel
        assert np.array_equal(bits(ld.Downconverter(f[c], D)(x)[0]), bits(y[c])), c
    pair = ld.Downconverter([f[6], f[4]], D)(x)      # the two-tuner kernel
    assert np.array_equal(bits(pair), bits(y[[6, 4]]))
    perm = rng.permutation(7)
    assert np.array_equal(bits(ld.Downconverter([f[i] for i in perm], D)(x)), bits(y[perm]))


# ---------------------------------------------------------------- 7. retune
def test_retune_is_bitwise_a_fresh_bank(ld):
    D = 10
    rng = np.random.default_rng(4700)
    three, five = list(rng.uniform(-0.5, 0.5, 3)), list(rng.uniform(-0.5, 0.5, 5))
    a, b = ld.Downconverter(three, D), ld.Downconverter(five, D)
    F = a.tile
    cuts = [D * F + 7, D * (F + 1) + 3, 4 * D - 1]
    x = cgauss(rng, sum(cuts))
    p1, p2, p3 = np.split(x, np.cumsum(cuts)[:-1])
    assert a(p1).shape[0] == 3
    a.freqs = five
    assert a.ntuners == 5 and a.skip == (-cuts[0]) % D
    b(p1)
    for p in (p2, p3):
        ya, yb = a(p), b(p)
        assert ya.shape == yb.shape and ya.shape[0] == 5 and ya.shape[1] > 0
        assert np.array_equal(bits(ya), bits(yb))


# ---------------------------------------------------------------- 8. seek: the phase near and past 2^32
@pytest.mark.parametrize("D", [5, 64])
@pytest.mark.parametrize("T", [2 ** 32 - 3 * 64 - 1, 2 ** 32 - 3 * 5 - 1, 2 ** 40 + 7])
def test_seek_against_the_definition_at_absolute_indices(ld, D, T):
    rng = np.random.default_rng(4800 + D)
    dc = ld.Downconverter(freqs_for(rng, 6), D)
    dc._seek(T)
    assert dc.skip == (-T) % D
    x = cgauss(rng, D * (dc.tile + 1) + 3)
    y = dc(x)
    ref = definition(x, dc.taps, dc.scale, dc.words, D, T)
    assert y.shape == ref.shape and y.shape[1] == dc.tile + 1 + (1 if 3 > (-T) % D else 0)
    err = per_row_err(y, ref)
    print(f"D={D} T={T}: worst row {err.max():.3g}")
    assert err.max() <= GATE


# ---------------------------------------------------------------- 9. host and device inputs, the row stride
def test_host_and_device_inputs_agree(ld):
    import torch
    f, D = [0.0371, -0.31337, 0.25], 8
    a, b, c, d = (ld.Downconverter(f, D) for _ in range(4))
    x = cgauss(np.random.default_rng(5000), D * (a.tile + 1) + 5)
    yh = a(x)
    yd = b(torch.from_numpy(x).cuda())
    assert yd.is_cuda and yd.dtype == torch.complex64 and tuple(yd.shape) == yh.shape
    assert all(yd[k].is_contiguous() for k in range(3))
    assert np.array_equal(bits(yd.cpu().numpy()), bits(yh))
    # strided and complex128 inputs are force-cast to contiguous complex64
    wide = np.zeros(2 * x.size, np.complex64)
    wide[::2] = x
    assert np.array_equal(bits(c(wide[::2])), bits(yh))
    assert np.array_equal(bits(d(x.astype(np.complex128))), bits(yh))
    one = ld.Downconverter(0.25, D)(x)               # a float: still two-dimensional
    assert one.shape == (1, yh.shape[1]) and np.array_equal(bits(one[0]), bits(yh[2]))


def test_c_abi_row_stride(ld):
    """ldsp_ddc_execute with ld > ncols, host and device memory: the rows land ld samples
    apart and the samples between them stay as they were."""
    import ctypes as C
    import os
    import torch
    lib = C.CDLL(os.path.join(os.path.dirname(ld.__file__), "..", "libldsp.so"))
    vp, sz = C.c_void_p, C.c_size_t
    lib.ldsp_ddc_create.argtypes = [vp, C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_float, C.POINTER(vp)]
    lib.ldsp_ddc_execute.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    lib.ldsp_ddc_destroy.argtypes = [vp]
    lib.ldsp_stream_synchronize.argtypes = [vp]
    f, D = np.array([0.0371, -0.31337, 0.25, 0.5, 0.1]), 8
    dc = ld.Downconverter(f, D)
    x = cgauss(np.random.default_rng(5500), D * (dc.tile + 2) + 1)
    ref = dc(x)
    K, pad = ref.shape[1], 5
    fill = np.complex64(7 - 3j)
    for mem in (0, 1):
        q = vp()
        assert lib.ldsp_ddc_create(f.ctypes.data, f.size, D, 6, 0.0, 60.0, C.byref(q)) == 0
        k = sz(0)
        if mem == 0:
            y = np.full((f.size, K + pad), fill, np.complex64)
            assert lib.ldsp_ddc_execute(q, x.ctypes.data, x.size, y.ctypes.data, K + pad, C.byref(k), 0, None) == 0
        else:
            xd = torch.from_numpy(x).cuda()
            yd = torch.full((f.size, K + pad), complex(fill), dtype=torch.complex64, device="cuda")
            torch.cuda.synchronize()
            assert lib.ldsp_ddc_execute(q, xd.data_ptr(), x.size, yd.data_ptr(), K + pad, C.byref(k), 1, None) == 0
            assert lib.ldsp_stream_synchronize(None) == 0
            y = yd.cpu().numpy()
        assert k.value == K
        assert np.array_equal(bits(y[:, :K]), bits(ref)), mem
        assert (y[:, K:] == fill).all(), mem
        assert lib.ldsp_ddc_destroy(q) == 0


# ---------------------------------------------------------------- 10. the existing paths
@pytest.mark.parametrize("M,D", [(8, 4), (64, 32)])
def test_agrees_with_the_channelizer(ld, M, D):
    ch = ld.Channelizer(M, D, m=4)                   # 2 M m + 1 = 16 D + 1 taps: within the Downconverter's 17 D
    ks = (0, 3, M - 1)
    dc = ld.Downconverter([k / M for k in ks], D, taps=ch.taps)
    dc.scale = ch.scale
    assert [int(w) for w in dc.words] == [(k << 32) // M for k in ks]
    x = cgauss(np.random.default_rng(6000 + M), D * (2 * ch.tile + 1) + 3)
    yc, yd = ch(x), dc(x)
    ref = definition(x, ch.taps, ch.scale, dc.words, D)
    for i, k in enumerate(ks):
        err = np.max(np.abs(yd[i].astype(np.complex128) - yc[k])) / np.max(np.abs(ref[i]))
        print(f"M={M} k={k}: {err:.3g}")
        assert err <= 2 * GATE                       # each side is within GATE of the float64 definition


def test_agrees_with_mix_down_filter(ld):
    D, f = 5, 5 / 16
    dc = ld.Downconverter(f, D)
    nco = ld.NCO("nco")
    nco.freq = np.float32(2 * np.pi * f)
    assert nco.state()[1] == int(dc.words[0]) == (5 << 32) // 16      # the table NCO is exact on this grid
    x = cgauss(np.random.default_rng(6500), D * (2 * dc.tile + 1) + 3)
    y = dc(x)
    ref = definition(x, dc.taps, dc.scale, dc.words, D)
    z = (ld.mix_down_filter(nco, ld.ComplexFIRFilter(dc.taps), x).astype(np.complex128) * np.float64(dc.scale))[::D]
    assert z.shape == y[0].shape
    err = np.max(np.abs(z - y[0])) / np.max(np.abs(ref[0]))
    print(f"mix_down_filter: {err:.3g}")
    assert err <= 2 * GATE


# ---------------------------------------------------------------- 11. rows feed the many-channel calls
def test_rows_feed_filter_resample_many(ld):
    import torch
    C_, D = 5, 4
    dc = ld.Downconverter(list(np.random.default_rng(7000).uniform(-0.5, 0.5, C_)), D)
    x = cgauss(np.random.default_rng(7001), D * 50_000 + 2)
    y = dc(torch.from_numpy(x).cuda())               # 50001 columns: odd rows start 8 bytes off a 16-byte line
    assert y.shape[1] == 50_001

    def pairs():                                     # the AMRadio front of test_gpu_many.py
        return ([ld.ComplexIIRFilter(filter_type="cheby2", order=8, Fc=15000 / 2e6) for _ in range(C_)],
                [ld.ComplexResampler(rate=48000 / 2e6, Fc=48000 / 2e6) for _ in range(C_)])

    fa, ra = pairs()
    fb, rb = pairs()
    many = ld.filter_resample_many(fa, ra, [y[k] for k in range(C_)])
    single = [ld.filter_resample(fb[k], rb[k], y[k].clone()) for k in range(C_)]
    torch.cuda.synchronize()
    for k in range(C_):
        g, r = many[k].cpu().numpy(), single[k].cpu().numpy()
        assert g.shape == r.shape and g.size > 0
        assert np.array_equal(bits(g), bits(r)), k
