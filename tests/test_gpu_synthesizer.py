"""Synthesizer on the GPU: the polyphase synthesis bank (k_synth.hip) against its
definition, evaluated here in float64 with the object's own taps and scale,

    z[t] = scale * sum_{k<M} sum_{n : 0 <= t - nD < L} g[t - nD] y[k][n] exp(+2 pi i k t / M)

with zeros before column 0 and the phase k t reduced mod M in integers.  Sizes
come from the kernel's tile (F input columns per workgroup) and Q = ceil(L / D):
one call of 2F + 1 + Q columns is two full tiles and a ragged one.  The gate of
1e-6 of max|z| is the project's gate for FIR-class kernels;
column streams cut into calls must give the single call's bits.  The round
trip Synthesizer(M)(Channelizer(M)(x)) is held to the float64 definitions' own
reconstruction error plus 1e-5: the two kernels' 1e-6 gates added over up to 64
rows as independent errors (8e-6)."""
import numpy as np
import pytest

from conftest import cgauss

pytestmark = pytest.mark.gpu

GATE = 1e-6
SHAPES = [(M, 6, D) for M in (4, 8, 16, 32, 64, 128, 256) for D in (M, M // 2)]      # (M, m, D): every instantiation
SHAPES += [(16, 1, 8), (256, 2, 128)]                                                # short prototypes


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def cgauss2(rng, M, K):
    return cgauss(rng, M * K).reshape(M, K)


def definition(y, g, scale, M, D):
    """The definition in float64.  The sum over k is taken first: its phase k t / M depends on t
    through t mod M alone, and k (t mod M) is reduced mod M in integers."""
    y = np.asarray(y).astype(np.complex128)
    g = np.asarray(g).astype(np.float64)
    K, L = y.shape[1], g.size
    Q = -(-L // D)
    gp = np.concatenate([g, np.zeros(Q * D - L)])
    kk = np.arange(M)
    E = np.exp(2j * np.pi * np.arange(M) / M)[(kk[:, None] * kk[None, :]) % M]      # E[p][k]
    A = np.concatenate([np.zeros((M, Q - 1), np.complex128), E @ y], axis=1)         # A[p][n + Q - 1]
    n = np.arange(K)[:, None]
    r = np.arange(D)[None, :]
    p = (n * D + r) % M                                                              # t mod M
    z = np.zeros((K, D), np.complex128)
    for q in range(Q):
        z += gp[q * D + r] * A[p, n - q + Q - 1]                                     # g[t - (n - q) D] A_{n-q}[t mod M]
    return float(scale) * z.reshape(-1)


def chan_definition(x, h, scale, M, D, ncols):
    """The Channelizer's definition (tests/test_gpu_channelizer.py) in float64."""
    x = np.asarray(x).astype(np.complex128)
    h = np.asarray(h).astype(np.float64)
    L = h.size
    xp = np.concatenate([np.zeros(L - 1, np.complex128), x])
    t = (np.arange(ncols) * D)[:, None] - np.arange(L)[None, :]
    w = xp[t + L - 1] * h[None, :]
    W = np.exp(-2j * np.pi * np.arange(M) / M)
    y = np.empty((M, ncols), np.complex128)
    for k in range(M):
        y[k] = float(scale) * np.sum(w * W[(k * t) % M], axis=1)
    return y


def rel_err(z, ref):
    return float(np.max(np.abs(z - ref)) / np.max(np.abs(ref)))


def nq(sy):
    return -(-len(sy.taps) // sy.interp)


# ---------------------------------------------------------------- 1. parity with the definition
@pytest.mark.parametrize("M,m,D", SHAPES)
def test_parity_with_definition(ld, M, m, D):
    sy = ld.Synthesizer(M, D, m=m)
    F, Q = sy.tile, nq(sy)
    K = 2 * F + 1 + Q
    y = cgauss2(np.random.default_rng(1000 + M + D + m), M, K)
    z = sy(y)
    assert z.dtype == np.complex64 and z.shape == (K * D,)
    err = rel_err(z, definition(y, sy.taps, sy.scale, M, D))
    print(f"M={M} m={m} D={D}: {err:.3g} of max|z|")
    assert err <= GATE


@pytest.mark.parametrize("M,D,L", [(8, 8, 5), (8, 4, 37), (64, 32, 64 * 17)])
def test_user_taps_against_definition(ld, M, D, L):
    """A prototype shorter than one column's D outputs, one that ends mid-column and the longest supported."""
    rng = np.random.default_rng(1500 + L)
    g = (rng.standard_normal(L) / np.sqrt(L)).astype(np.float32)
    sy = ld.Synthesizer(M, D, taps=g)
    sy.scale = 0.5
    y = cgauss2(rng, M, sy.tile + 2 + nq(sy))
    z = sy(y)
    err = rel_err(z, definition(y, g, 0.5, M, D))
    print(f"M={M} D={D} L={L}: {err:.3g} of max|z|")
    assert err <= GATE


# ---------------------------------------------------------------- 2. one row carrying a constant
@pytest.mark.parametrize("M,D,k", [(8, 4, 3), (16, 16, 5), (64, 32, 63)])
def test_constant_row_is_a_tone(ld, M, D, k):
    sy = ld.Synthesizer(M, D)
    K = 2 * sy.tile + 1 + nq(sy)
    y = np.zeros((M, K), np.complex64)
    y[k] = 1.0
    z = sy(y)
    err = rel_err(z, definition(y, sy.taps, sy.scale, M, D))
    print(f"M={M} D={D} k={k}: {err:.3g} of max|z|")
    assert err <= GATE
    S = (z.size // 2 // M) * M                       # whole periods of the tone, past the start-up
    s = z[z.size - S:]
    spec = np.abs(np.fft.fft(s.astype(np.complex128)))
    assert int(np.argmax(spec)) == k * (s.size // M)


# ---------------------------------------------------------------- 3. streaming invariance, bitwise
@pytest.mark.parametrize("M,m,D", [(8, 6, 4), (64, 6, 32), (256, 6, 128)])
def test_streaming_is_bitwise_invariant(ld, M, m, D):
    sy = ld.Synthesizer(M, D, m=m)
    F, Q = sy.tile, nq(sy)
    rng = np.random.default_rng(3000 + M)
    forced = [0, 1, Q - 2, Q - 1, Q, F - 1, F, F + 1]
    seeded = [int(v) for v in rng.integers(1, 2 * Q + 2, 6)]
    lens = [seeded[0], *forced[:4], seeded[1], *forced[4:6], seeded[2], seeded[3], *forced[6:], seeded[4], seeded[5]]
    lens.append(3)                                   # something after the last forced cut
    y = cgauss2(rng, M, sum(lens))
    whole = sy(y)
    sy.reset()
    parts, T = [], 0
    for c in lens:
        assert sy.num_outputs(c) == c * D
        z = sy(y[:, T:T + c])
        assert z.shape == (c * D,), (c, z.shape)
        T += c
        parts.append(z)
    got = np.concatenate(parts)
    assert got.shape == whole.shape
    assert np.array_equal(bits(got), bits(whole))


# ---------------------------------------------------------------- 4. reset
def test_reset_reproduces_the_first_output(ld):
    sy = ld.Synthesizer(16, 8)
    y = cgauss2(np.random.default_rng(4000), 16, sy.tile + 13)
    first = sy(y)
    sy(y[:, :37])                                    # leaves an odd column parity behind
    sy.reset()
    assert np.array_equal(bits(sy(y)), bits(first))


# ---------------------------------------------------------------- 5. host and device inputs
def test_host_and_device_inputs_agree(ld):
    import torch
    M, D = 16, 8
    a, b, c, d, e = (ld.Synthesizer(M, D) for _ in range(5))
    K = a.tile + 1 + nq(a)
    y = cgauss2(np.random.default_rng(5000), M, K)
    zh = a(y)
    zd = b(torch.from_numpy(y).cuda())
    assert zd.is_cuda and zd.dtype == torch.complex64 and tuple(zd.shape) == zh.shape
    assert np.array_equal(bits(zd.cpu().numpy()), bits(zh))
    # complex128 and Fortran-ordered inputs are force-cast to C-contiguous complex64
    assert np.array_equal(bits(c(y.astype(np.complex128))), bits(zh))
    yf = np.asfortranarray(y)
    assert not yf.flags.c_contiguous
    assert np.array_equal(bits(d(yf)), bits(zh))
    # a device tensor whose columns are not contiguous is made contiguous first
    assert np.array_equal(bits(e(torch.from_numpy(np.ascontiguousarray(y.T)).cuda().T).cpu().numpy()), bits(zh))


def test_device_view_is_read_in_place(ld):
    """A block of rows and a range of columns of a larger device tensor (ld > K)."""
    import torch
    M, D = 16, 8
    a, b = ld.Synthesizer(M, D), ld.Synthesizer(M, D)
    K = a.tile + 3
    big = cgauss2(np.random.default_rng(5200), 3 * M, K + 11)
    bd = torch.from_numpy(big).cuda()
    view = bd[M:2 * M, 7:7 + K]
    assert view.stride(1) == 1 and view.stride(0) == K + 11 and not view.is_contiguous()
    zv = a(view)
    zc = b(np.ascontiguousarray(big[M:2 * M, 7:7 + K]))
    assert np.array_equal(bits(zv.cpu().numpy()), bits(zc))
    assert np.array_equal(bd.cpu().numpy(), big)     # the input is left as it was


def test_c_abi_row_stride(ld):
    """ldsp_synth_execute with ld > ncols, host and device memory."""
    import ctypes as C
    import os
    import torch
    lib = C.CDLL(os.path.join(os.path.dirname(ld.__file__), "..", "libldsp.so"))
    vp, sz = C.c_void_p, C.c_size_t
    lib.ldsp_synth_create.argtypes = [C.c_uint, C.c_uint, C.c_uint, C.c_float, C.c_float, C.POINTER(vp)]
    lib.ldsp_synth_execute.argtypes = [vp, vp, sz, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    lib.ldsp_synth_destroy.argtypes = [vp]
    lib.ldsp_stream_synchronize.argtypes = [vp]
    M, D = 16, 8
    sy = ld.Synthesizer(M, D)
    K, pad = sy.tile + 2, 5
    wide = cgauss2(np.random.default_rng(5500), M, K + pad)
    ref = sy(np.ascontiguousarray(wide[:, :K]))
    fill = np.complex64(7 - 3j)
    for mem in (0, 1):
        q = vp()
        assert lib.ldsp_synth_create(M, D, 6, 0.0, 60.0, C.byref(q)) == 0
        n = sz(0)
        if mem == 0:
            z = np.full(K * D + pad, fill, np.complex64)
            assert lib.ldsp_synth_execute(q, wide.ctypes.data, K + pad, K, z.ctypes.data, z.size, C.byref(n), 0,
                                          None) == 0
        else:
            yd = torch.from_numpy(wide).cuda()
            zd = torch.full((K * D + pad,), complex(fill), dtype=torch.complex64, device="cuda")
            torch.cuda.synchronize()
            assert lib.ldsp_synth_execute(q, yd.data_ptr(), K + pad, K, zd.data_ptr(), K * D + pad, C.byref(n), 1,
                                          None) == 0
            assert lib.ldsp_stream_synchronize(None) == 0
            z = zd.cpu().numpy()
        assert n.value == K * D
        assert np.array_equal(bits(z[:K * D]), bits(ref)), mem
        assert (z[K * D:] == fill).all(), mem
        assert lib.ldsp_synth_destroy(q) == 0


# ---------------------------------------------------------------- 6. round trip with the Channelizer
@pytest.mark.parametrize("M", [8, 16, 64])
def test_round_trip_with_channelizer(ld, M):
    ch, sy = ld.Channelizer(M), ld.Synthesizer(M)
    D, L = M // 2, len(sy.taps)
    N = D * (-(-4 * L // D))
    x = cgauss(np.random.default_rng(6000 + M), N)
    z = sy(ch(x))
    assert z.shape == (N,)
    zr = definition(chan_definition(x, ch.taps, ch.scale, M, D, N // D), sy.taps, sy.scale, M, D)
    xs = x[:N - L + 1].astype(np.complex128)
    e_gpu = float(np.max(np.abs(z[L - 1:] - xs)) / np.max(np.abs(x)))
    e_ref = float(np.max(np.abs(zr[L - 1:] - xs)) / np.max(np.abs(x)))
    print(f"M={M}: e_gpu {e_gpu:.4g}  e_ref {e_ref:.4g}")
    assert e_gpu <= e_ref + 1e-5
