"""Host side of the Synthesizer without a GPU (CPU suite): construction, the
default prototypes (bit-identical to the restatement's firdes_kaiser at both
default cutoffs) and their scale, user taps, num_outputs, the argument errors of
ldsp_synth_create* / _execute (decided before any device work), the tile hook,
the row centres, the stand-alone C driver under ASan + UBSan, and a design
check in float64: the Channelizer's and the Synthesizer's definitions, with the
objects' own taps and scales, reproduce the input delayed by L - 1 samples to
the prototype's stop-band level.  The GPU side is tests/test_gpu_synthesizer.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import cgauss

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "python-liquiddsp_amd")
LIBPATH = os.path.join(PKG, "libldsp.so")

LDSP_EINVAL, LDSP_EHIP, LDSP_ERANGE, LDSP_EUNSUP = -1, -3, -4, -5
MEM_HOST = 0
SUPPORTED = [(M, D) for M in (4, 8, 16, 32, 64, 128, 256) for D in (M, M // 2)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIBPATH):
        pytest.fail("libldsp.so not built (run __graft_entry__.build())")
    L = C.CDLL(LIBPATH)
    L.ldsp_last_error.restype = C.c_char_p
    vp, u, f, sz = C.c_void_p, C.c_uint, C.c_float, C.c_size_t
    L.ldsp_synth_create.argtypes = [u, u, u, f, f, C.POINTER(vp)]
    L.ldsp_synth_create_taps.argtypes = [u, u, vp, u, C.POINTER(vp)]
    L.ldsp_synth_destroy.argtypes = [vp]
    L.ldsp_synth_reset.argtypes = [vp]
    L.ldsp_synth_get_info.argtypes = [vp, C.POINTER(u), C.POINTER(u), C.POINTER(u)]
    L.ldsp_synth_get_taps.argtypes = [vp, vp]
    L.ldsp_synth_get_scale.argtypes = [vp, C.POINTER(f)]
    L.ldsp_synth_set_scale.argtypes = [vp, f]
    L.ldsp_synth_num_outputs.argtypes = [vp, sz, C.POINTER(sz)]
    L.ldsp_synth_execute.argtypes = [vp, vp, sz, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    L.ldsp_debug_synth_tile.argtypes = [u, u, C.POINTER(sz)]
    return L


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def create(lib, M, D, m=6, fc=0.0, As=60.0):
    q = C.c_void_p()
    return lib.ldsp_synth_create(M, D, m, fc, As, C.byref(q)), q


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- construction
@pytest.mark.parametrize("M,D", [(4, 4), (4, 2), (64, 32), (256, 128), (256, 256)])
def test_constructs(ld, M, D):
    sy = ld.Synthesizer(M, D)
    assert (sy.nchan, sy.interp) == (M, D)
    assert len(sy.taps) == 2 * M * 6 + 1
    sy.reset()                                       # before the first call: nothing on the device yet
    assert ld.Synthesizer(M).interp == M // 2
    assert ld.Synthesizer(nchan=M, interp=None, m=2, Fc=0.4 / M, As=40.0, taps=None).interp == M // 2


# ---------------------------------------------------------------- design
@pytest.mark.parametrize("M,D,m,As", [(4, 2, 4, 60.0), (16, 8, 6, 60.0), (16, 16, 6, 60.0), (256, 128, 8, 40.0),
                                      (256, 256, 2, 80.0)])
def test_default_prototype_bitwise(ld, lib, ora, M, D, m, As):
    sy = ld.Synthesizer(M, D, m=m, As=As)
    fc = 1.0 / M if D == M // 2 else 0.5 / M
    ref = ora.firdes_kaiser(2 * M * m + 1, fc, As, 0)
    assert sy.taps.dtype == np.float32 and sy.taps.shape == ref.shape
    assert (bits(sy.taps) == bits(ref)).all()
    assert np.float32(sy.scale) == np.float32(D / np.sum(sy.taps.astype(np.float64)))
    # the same object through the C ABI
    rc, q = create(lib, M, D, m, 0.0, As)
    assert rc == 0, lib.ldsp_last_error()
    Mo, Do, Lo = C.c_uint(), C.c_uint(), C.c_uint()
    assert lib.ldsp_synth_get_info(q, C.byref(Mo), C.byref(Do), C.byref(Lo)) == 0
    assert (Mo.value, Do.value, Lo.value) == (M, D, 2 * M * m + 1)
    assert lib.ldsp_synth_get_info(q, None, None, None) == 0
    g = np.full(Lo.value, np.nan, np.float32)
    assert lib.ldsp_synth_get_taps(q, g.ctypes.data) == 0
    assert (bits(g) == bits(ref)).all()
    s = C.c_float()
    assert lib.ldsp_synth_get_scale(q, C.byref(s)) == 0 and np.float32(s.value) == np.float32(sy.scale)
    assert lib.ldsp_synth_destroy(q) == 0


def test_cutoff_override(ld, ora):
    sy = ld.Synthesizer(16, m=4, Fc=0.05)
    assert (bits(sy.taps) == bits(ora.firdes_kaiser(2 * 16 * 4 + 1, 0.05, 60.0, 0))).all()
    assert np.float32(sy.scale) == np.float32(8 / np.sum(sy.taps.astype(np.float64)))


def test_user_taps(ld):
    g = np.random.default_rng(5).standard_normal(37).astype(np.float32)
    sy = ld.Synthesizer(8, 8, taps=g)
    assert (bits(sy.taps) == bits(g)).all() and sy.scale == 1.0
    sy.scale = 0.25
    assert sy.scale == 0.25
    assert len(ld.Synthesizer(4, taps=[1.0]).taps) == 1
    ld.Synthesizer(4, 4, taps=np.ones(17 * 4, np.float32))      # 17 taps per branch: the most supported
    ld.Synthesizer(4, 2, taps=np.ones(17 * 4, np.float32))


def test_num_outputs(ld, lib):
    sy = ld.Synthesizer(16, 8)
    assert [sy.num_outputs(K) for K in (0, 1, 7, 43)] == [0, 8, 56, 344]
    assert ld.Synthesizer(16, 16).num_outputs(43) == 688
    for M, D in SUPPORTED:
        rc, q = create(lib, M, D)
        assert rc == 0
        n = C.c_size_t(12345)
        for K in (0, 1, 5, 1 << 20):
            assert lib.ldsp_synth_num_outputs(q, K, C.byref(n)) == 0 and n.value == K * D
        assert lib.ldsp_synth_reset(q) == 0
        lib.ldsp_synth_destroy(q)


# ---------------------------------------------------------------- errors
def test_constructor_errors(ld):
    for M in (0, 2, 3, 12):
        with pytest.raises(ValueError):
            ld.Synthesizer(M)
        with pytest.raises(ValueError):
            ld.Synthesizer(M, M)
    for D in (0, 1, 4, 15, 32):
        with pytest.raises(ValueError):
            ld.Synthesizer(16, D)
    with pytest.raises(ValueError):
        ld.Synthesizer(16, m=0)
    for As in (0.0, -60.0):
        with pytest.raises(ValueError):
            ld.Synthesizer(16, As=As)
    for Fc in (0.5, 0.75):
        with pytest.raises(ValueError):
            ld.Synthesizer(16, Fc=Fc)
    with pytest.raises(ValueError):
        ld.Synthesizer(16, taps=[])
    with pytest.raises(NotImplementedError):
        ld.Synthesizer(512)
    with pytest.raises(NotImplementedError):
        ld.Synthesizer(16, m=9)
    with pytest.raises(NotImplementedError):
        ld.Synthesizer(4, taps=np.ones(17 * 4 + 1, np.float32))


def test_create_codes(lib):
    for M in (0, 2, 3, 12):
        assert create(lib, M, M)[0] == LDSP_EINVAL
        assert create(lib, M, M // 2)[0] == LDSP_EINVAL
    for D in (0, 4, 32):
        assert create(lib, 16, D)[0] == LDSP_EINVAL
    assert create(lib, 16, 8, m=0)[0] == LDSP_EINVAL
    assert create(lib, 16, 8, As=0.0)[0] == LDSP_EINVAL
    assert create(lib, 16, 8, fc=0.5)[0] == LDSP_EINVAL
    assert create(lib, 512, 256)[0] == LDSP_EUNSUP
    assert create(lib, 16, 8, m=9)[0] == LDSP_EUNSUP
    assert lib.ldsp_synth_create(16, 8, 6, 0.0, 60.0, None) == LDSP_EINVAL
    g = np.ones(8, np.float32)
    q = C.c_void_p()
    assert lib.ldsp_synth_create_taps(8, 4, g.ctypes.data, 0, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_synth_create_taps(8, 4, None, 8, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_synth_create_taps(8, 4, g.ctypes.data, 8, None) == LDSP_EINVAL
    assert lib.ldsp_synth_create_taps(12, 6, g.ctypes.data, 8, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_synth_create_taps(512, 512, g.ctypes.data, 8, C.byref(q)) == LDSP_EUNSUP
    big = np.ones(17 * 8 + 1, np.float32)
    assert lib.ldsp_synth_create_taps(8, 4, big.ctypes.data, big.size, C.byref(q)) == LDSP_EUNSUP
    assert lib.ldsp_synth_create_taps(8, 4, big.ctypes.data, big.size - 1, C.byref(q)) == 0
    assert lib.ldsp_synth_destroy(q) == 0


def test_execute_argument_errors_need_no_gpu(lib):
    rc, q = create(lib, 8, 4)
    assert rc == 0
    y = np.zeros((8, 16), np.complex64)
    z = np.zeros(64, np.complex64)
    yp, zp = y.ctypes.data, z.ctypes.data
    n = C.c_size_t(0)
    assert lib.ldsp_synth_execute(q, yp, 16, 16, zp, 63, C.byref(n), MEM_HOST, None) == LDSP_ERANGE
    assert n.value == 64
    assert lib.ldsp_synth_execute(q, yp, 16, 16, zp, 63, None, MEM_HOST, None) == LDSP_ERANGE
    assert lib.ldsp_synth_execute(q, yp, 15, 16, zp, 64, C.byref(n), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_synth_execute(None, yp, 16, 16, zp, 64, C.byref(n), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_synth_execute(q, None, 16, 16, zp, 64, C.byref(n), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_synth_execute(q, yp, 16, 16, None, 64, C.byref(n), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_synth_execute(q, yp, 16, 16, zp, 64, C.byref(n), 7, None) == LDSP_EINVAL
    # the object is untouched: the same taps, scale and counts as a fresh one
    rc, f = create(lib, 8, 4)
    a, b = np.zeros(97, np.float32), np.ones(97, np.float32)
    assert lib.ldsp_synth_get_taps(q, a.ctypes.data) == 0 and lib.ldsp_synth_get_taps(f, b.ctypes.data) == 0
    assert (bits(a) == bits(b)).all()
    sa, sb = C.c_float(), C.c_float(1.0)
    assert lib.ldsp_synth_get_scale(q, C.byref(sa)) == 0 and lib.ldsp_synth_get_scale(f, C.byref(sb)) == 0
    assert sa.value == sb.value
    assert lib.ldsp_synth_num_outputs(q, 16, C.byref(n)) == 0 and n.value == 64
    assert lib.ldsp_synth_num_outputs(q, 64, None) == LDSP_EINVAL
    assert lib.ldsp_synth_num_outputs(None, 64, C.byref(n)) == LDSP_EINVAL
    assert lib.ldsp_synth_get_taps(q, None) == LDSP_EINVAL
    assert lib.ldsp_synth_get_scale(q, None) == LDSP_EINVAL
    assert lib.ldsp_synth_reset(None) == LDSP_EINVAL
    assert lib.ldsp_synth_destroy(q) == 0 and lib.ldsp_synth_destroy(f) == 0


def test_call_shape_errors(ld):
    sy = ld.Synthesizer(8)
    with pytest.raises(ValueError):
        sy(np.zeros(64, np.complex64))                          # 1-D
    with pytest.raises(ValueError):
        sy(np.zeros((4, 16), np.complex64))                     # a wrong row count
    with pytest.raises(ValueError):
        sy(np.zeros((8, 4, 2), np.complex64))


# ---------------------------------------------------------------- no GPU
def test_call_raises_without_gpu(ld):
    if ld.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ld.Synthesizer(4)(np.zeros((4, 16), np.complex64))


# ---------------------------------------------------------------- other properties
@pytest.mark.parametrize("M", [4, 16, 256])
def test_centers(ld, M):
    c = ld.Synthesizer(M).centers
    k = np.arange(M)
    assert c.dtype == np.float64 and np.array_equal(c, ((k / M + 0.5) % 1) - 0.5)
    assert c[0] == 0 and c[M // 2] == -0.5 and c[M - 1] == -1 / M
    assert np.array_equal(c, ld.Channelizer(M).centers)


def test_tile_hook(lib, ld):
    f = C.c_size_t()
    assert len(SUPPORTED) == 14
    for M, D in SUPPORTED:
        assert lib.ldsp_debug_synth_tile(M, D, C.byref(f)) == 0
        assert f.value >= 32
        assert ld.Synthesizer(M, D).tile == f.value
    assert lib.ldsp_debug_synth_tile(12, 6, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_synth_tile(16, 4, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_synth_tile(512, 256, C.byref(f)) == LDSP_EUNSUP
    assert lib.ldsp_debug_synth_tile(16, 8, None) == LDSP_EINVAL


# ---------------------------------------------------------------- the C driver under ASan + UBSan
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:")


def test_synth_driver_asan_ubsan():
    r = subprocess.run(["make", "-s", "-j8", "-C", PKG, "synth_asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(PKG, "build", "synth_driver_asan")
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the driver is not instrumented"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert not any(k in out for k in REPORTS), out[-4000:]
    assert "all checks passed" in r.stdout


# ---------------------------------------------------------------- design check, float64
def chan_definition(x, h, scale, M, D, ncols):
    """The Channelizer's definition (tests/test_gpu_channelizer.py) in float64:
    y[k][n] = scale sum_j h[j] x[nD - j] exp(-2 pi i k (nD - j) / M), the phase reduced in integers."""
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


def synth_definition(y, g, scale, M, D):
    """The Synthesizer's definition in float64:
    z[t] = scale sum_k sum_n g[t - nD] y[k][n] exp(+2 pi i k t / M), the phase k t reduced mod M in
    integers; the sum over k is taken first (it depends on t through t mod M alone)."""
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


@pytest.mark.parametrize("M", [8, 16, 64])
def test_default_designs_reconstruct(ld, M):
    """Channelizer(M) -> Synthesizer(M) at the defaults (D = M / 2, m = 6, As = 60), both by
    their float64 definitions: z[t + L - 1] = x[t] to twice the 60 dB stop-band level."""
    ch, sy = ld.Channelizer(M), ld.Synthesizer(M)
    D, L = M // 2, len(sy.taps)
    assert L == len(ch.taps) == 12 * M + 1
    N = D * (-(-4 * L // D))
    x = cgauss(np.random.default_rng(9000 + M), N)
    y = chan_definition(x, ch.taps, ch.scale, M, D, N // D)
    z = synth_definition(y, sy.taps, sy.scale, M, D)
    assert z.size == N
    err = np.max(np.abs(z[L - 1:] - x[:N - L + 1])) / np.max(np.abs(x))
    print(f"M={M}: reconstruction error {err:.3g} of max|x|")
    assert err <= 2e-3
