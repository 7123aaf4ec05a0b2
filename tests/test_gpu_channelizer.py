"""Channelizer on the GPU: the polyphase analysis bank (k_chan.hip) against its
definition, evaluated here in float64 with the object's own taps and scale,

    y[k][n] = scale * sum_{j<L} h[j] x[nD - j] exp(-2 pi i k (nD - j) / M)

with zeros before the stream's first sample.  Sizes come from the kernel's tile
(F output frames per workgroup): one call of D (2F + 1) + 3 samples is two full
tiles, a one-frame tile and a ragged tail.  The gate of 1e-6 is the project's
gate for FIR-class kernels; streams cut into calls must give the
single call's bits."""
import numpy as np
import pytest

from conftest import cgauss

pytestmark = pytest.mark.gpu

GATE = 1e-6
SHAPES = [(4, 4, 4), (4, 4, 2), (8, 6, 4), (16, 6, 16), (16, 6, 8), (64, 6, 32), (128, 6, 64), (256, 6, 128),
          (256, 8, 256)]                              # (M, m, D)
# the kernel instantiations the list above leaves out (M = 32 is the only 4 x 8 DFT), and short prototypes
SHAPES += [(8, 6, 8), (32, 6, 32), (32, 6, 16), (64, 6, 64), (128, 6, 128), (16, 1, 8), (256, 2, 128)]


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def definition(x, h, scale, M, D, ncols):
    """The definition in float64; the phase k (nD - j) / M is reduced in integers."""
    x = np.asarray(x).astype(np.complex128)
    h = np.asarray(h).astype(np.float64)
    L = h.size
    xp = np.concatenate([np.zeros(L - 1, np.complex128), x])          # xp[t + L - 1] = x[t]
    t = (np.arange(ncols) * D)[:, None] - np.arange(L)[None, :]       # nD - j
    assert ncols == 0 or t.max() < x.size
    w = xp[t + L - 1] * h[None, :]
    W = np.exp(-2j * np.pi * np.arange(M) / M)
    y = np.empty((M, ncols), np.complex128)
    for k in range(M):
        y[k] = float(scale) * np.sum(w * W[(k * t) % M], axis=1)
    return y


def per_channel_err(y, ref):
    return np.max(np.abs(y - ref), axis=1) / np.max(np.abs(ref), axis=1)


# ---------------------------------------------------------------- 1. parity with the definition
@pytest.mark.parametrize("M,m,D", SHAPES)
def test_parity_with_definition(ld, M, m, D):
    ch = ld.Channelizer(M, D, m=m)
    F = ch.tile
    N = D * (2 * F + 1) + 3
    x = cgauss(np.random.default_rng(1000 + M + D), N)
    y = ch(x)
    assert y.dtype == np.complex64 and y.shape == (M, -(-N // D))
    ref = definition(x, ch.taps, ch.scale, M, D, y.shape[1])
    err = per_channel_err(y, ref)
    print(f"M={M} m={m} D={D}: worst channel {err.max():.3g}")
    assert err.max() <= GATE, (int(np.argmax(err)), float(err.max()))


@pytest.mark.parametrize("M,D,L", [(8, 8, 5), (8, 4, 37), (64, 32, 64 * 17)])
def test_user_taps_against_definition(ld, M, D, L):
    """A prototype shorter than one branch row, one that ends mid-row and the longest supported."""
    rng = np.random.default_rng(1500 + L)
    h = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
    ch = ld.Channelizer(M, D, taps=h)
    ch.scale = 0.5
    x = cgauss(rng, D * (ch.tile + 1) + 2)
    y = ch(x)
    err = per_channel_err(y, definition(x, h, 0.5, M, D, y.shape[1]))
    print(f"M={M} D={D} L={L}: worst channel {err.max():.3g}")
    assert err.max() <= GATE


# ---------------------------------------------------------------- 2. two stations
@pytest.mark.parametrize("M", [8, 16, 64])
def test_two_stations(ld, M):
    ch = ld.Channelizer(M)
    D, F = ch.decim, ch.tile
    N = D * (2 * F + 1) + 3
    rng = np.random.default_rng(2000 + M)
    t = np.arange(N)
    x = ((1 + 0.5 * np.sin(2 * np.pi * 0.011 / M * t)) * np.exp(2j * np.pi * (1 / M) * t)
         + 0.25 * (1 + 0.5 * np.sin(2 * np.pi * 0.017 / M * t)) * np.exp(2j * np.pi * ((M - 3) / M) * t)
         + cgauss(rng, N, 1e-3)).astype(np.complex64)
    y = ch(x)
    ref = definition(x, ch.taps, ch.scale, M, D, y.shape[1])
    err = np.max(np.abs(y - ref)) / np.max(np.abs(ref))
    print(f"M={M}: {err:.3g}")
    assert err <= GATE
    order = np.argsort(np.sum(np.abs(y.astype(np.complex128)) ** 2, axis=1))
    assert order[-1] == 1 and order[-2] == M - 3


# ---------------------------------------------------------------- 3. streaming invariance, bitwise
@pytest.mark.parametrize("M,m,D", [(8, 6, 4), (64, 6, 32), (256, 6, 128)])
def test_streaming_is_bitwise_invariant(ld, M, m, D):
    ch = ld.Channelizer(M, D, m=m)
    F = ch.tile
    P = -(-len(ch.taps) // M)
    rng = np.random.default_rng(3000 + M)
    forced = [0, 1, D - 1, D + 1, F * D - 1, F * D, F * D + 1, P * M - 2]
    seeded = [int(v) for v in rng.integers(1, 3 * D + 2, 6)]
    lens = [seeded[0], *forced[:4], seeded[1], *forced[4:6], seeded[2], seeded[3], *forced[6:], seeded[4], seeded[5]]
    lens.append(2 * D + 1)                          # something after the last forced cut
    x = cgauss(rng, sum(lens))
    whole = ch(x)
    assert ch.skip == (-x.size) % D
    ch.reset()
    assert ch.skip == 0
    parts, T = [], 0
    for c in lens:
        want = ch.num_outputs(c)
        skip = (-T) % D
        assert want == (-(-(c - skip) // D) if c > skip else 0)
        y = ch(x[T:T + c])
        assert y.shape == (M, want), (c, y.shape, want)
        T += c
        assert ch.skip == (-T) % D
        parts.append(y)
    got = np.concatenate(parts, axis=1)
    assert got.shape == whole.shape
    assert np.array_equal(bits(got), bits(whole))


# ---------------------------------------------------------------- 4. reset
def test_reset_reproduces_the_first_output(ld):
    ch = ld.Channelizer(16, 8)
    x = cgauss(np.random.default_rng(4000), 8 * ch.tile + 13)
    first = ch(x)
    ch(x[:37])                                       # leaves skip != 0 and an odd output parity behind
    ch.reset()
    assert np.array_equal(bits(ch(x)), bits(first))


# ---------------------------------------------------------------- 5. host and device inputs
def test_host_and_device_inputs_agree(ld):
    import torch
    M, D = 16, 8
    a, b, c, d = (ld.Channelizer(M, D) for _ in range(4))
    x = cgauss(np.random.default_rng(5000), D * (a.tile + 1) + 5)
    yh = a(x)
    yd = b(torch.from_numpy(x).cuda())
    assert yd.is_cuda and yd.dtype == torch.complex64 and tuple(yd.shape) == yh.shape
    assert np.array_equal(bits(yd.cpu().numpy()), bits(yh))
    # strided and complex128 inputs are force-cast to contiguous complex64
    wide = np.zeros(2 * x.size, np.complex64)
    wide[::2] = x
    assert np.array_equal(bits(c(wide[::2])), bits(yh))
    assert np.array_equal(bits(d(x.astype(np.complex128))), bits(yh))


def test_c_abi_row_stride(ld):
    """ldsp_chan_execute with ld > ncols, host and device memory: the rows land ld samples
    apart and the samples between them stay as they were."""
    import ctypes as C
    import os
    import torch
    lib = C.CDLL(os.path.join(os.path.dirname(ld.__file__), "..", "libldsp.so"))
    vp, sz = C.c_void_p, C.c_size_t
    lib.ldsp_chan_create.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_float, C.POINTER(vp)]
    lib.ldsp_chan_execute.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    lib.ldsp_chan_destroy.argtypes = [vp]
    lib.ldsp_stream_synchronize.argtypes = [vp]
    M, D = 16, 8
    ch = ld.Channelizer(M, D)
    x = cgauss(np.random.default_rng(5500), D * (ch.tile + 2) + 1)
    ref = ch(x)
    K, pad = ref.shape[1], 5
    fill = np.complex64(7 - 3j)
    for mem in (0, 1):
        q = vp()
        assert lib.ldsp_chan_create(M, D, 6, 0.0, 60.0, C.byref(q)) == 0
        k = sz(0)
        if mem == 0:
            y = np.full((M, K + pad), fill, np.complex64)
            assert lib.ldsp_chan_execute(q, x.ctypes.data, x.size, y.ctypes.data, K + pad, C.byref(k), 0, None) == 0
        else:
            xd = torch.from_numpy(x).cuda()
            yd = torch.full((M, K + pad), complex(fill), dtype=torch.complex64, device="cuda")
            torch.cuda.synchronize()
            assert lib.ldsp_chan_execute(q, xd.data_ptr(), x.size, yd.data_ptr(), K + pad, C.byref(k), 1, None) == 0
            assert lib.ldsp_stream_synchronize(None) == 0
            y = yd.cpu().numpy()
        assert k.value == K
        assert np.array_equal(bits(y[:, :K]), bits(ref)), mem
        assert (y[:, K:] == fill).all(), mem
        assert lib.ldsp_chan_destroy(q) == 0


# ---------------------------------------------------------------- 6. the existing path
def test_agrees_with_mix_down_filter(ld):
    M, D = 8, 4
    ch = ld.Channelizer(M, D)
    x = cgauss(np.random.default_rng(6000), D * (ch.tile + 1) + 3)
    y = ch(x)
    ref = definition(x, ch.taps, ch.scale, M, D, y.shape[1])
    for k in (0, 3, 7):
        nco = ld.NCO("nco")
        nco.freq = np.float32(2 * np.pi * k / M)
        fir = ld.ComplexFIRFilter(ch.taps)
        z = (ld.mix_down_filter(nco, fir, x).astype(np.complex128) * np.float64(ch.scale))[::D]
        assert z.shape == y[k].shape
        err = np.max(np.abs(z - y[k])) / np.max(np.abs(ref[k]))
        print(f"k={k}: {err:.3g}")
        assert err <= 2 * GATE                       # each side is within GATE of the float64 definition


# ---------------------------------------------------------------- 7. rows feed the many-channel calls
def test_rows_feed_filter_resample_many(ld):
    import torch
    M = 8
    ch = ld.Channelizer(M)
    x = cgauss(np.random.default_rng(7000), ch.decim * 50_000 + 2)
    y = ch(torch.from_numpy(x).cuda())               # 50001 columns: odd rows start 8 bytes off a 16-byte line

    def pairs():                                     # the AMRadio front of test_gpu_many.py
        return ([ld.ComplexIIRFilter(filter_type="cheby2", order=8, Fc=15000 / 2e6) for _ in range(M)],
                [ld.ComplexResampler(rate=48000 / 2e6, Fc=48000 / 2e6) for _ in range(M)])

    fa, ra = pairs()
    fb, rb = pairs()
    many = ld.filter_resample_many(fa, ra, [y[k] for k in range(M)])
    single = [ld.filter_resample(fb[k], rb[k], y[k].clone()) for k in range(M)]
    torch.cuda.synchronize()
    for k in range(M):
        g, r = many[k].cpu().numpy(), single[k].cpu().numpy()
        assert g.shape == r.shape and g.size > 0
        assert np.array_equal(bits(g), bits(r)), k
