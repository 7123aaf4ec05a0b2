"""Host side of the Channelizer without a GPU (CPU suite): construction, the
default prototype (bit-identical to the restatement's firdes_kaiser) and its
scale, the output schedule of first calls, the argument errors of
ldsp_chan_create* / _execute (decided before any device work) and the channel
centres.  The GPU side is tests/test_gpu_channelizer.py."""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIBPATH = os.path.join(REPO, "python-liquiddsp_amd", "libldsp.so")

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
    L.ldsp_chan_create.argtypes = [u, u, u, f, f, C.POINTER(vp)]
    L.ldsp_chan_create_taps.argtypes = [u, u, vp, u, C.POINTER(vp)]
    L.ldsp_chan_destroy.argtypes = [vp]
    L.ldsp_chan_reset.argtypes = [vp]
    L.ldsp_chan_get_info.argtypes = [vp, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)]
    L.ldsp_chan_get_taps.argtypes = [vp, vp]
    L.ldsp_chan_get_scale.argtypes = [vp, C.POINTER(f)]
    L.ldsp_chan_set_scale.argtypes = [vp, f]
    L.ldsp_chan_num_outputs.argtypes = [vp, sz, C.POINTER(sz)]
    L.ldsp_chan_execute.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    L.ldsp_debug_chan_tile.argtypes = [u, u, C.POINTER(sz)]
    return L


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def create(lib, M, D, m=6, fc=0.0, As=60.0):
    q = C.c_void_p()
    return lib.ldsp_chan_create(M, D, m, fc, As, C.byref(q)), q


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- construction
@pytest.mark.parametrize("M,D", [(4, 4), (4, 2), (64, 32), (256, 128)])
def test_constructs(ld, M, D):
    ch = ld.Channelizer(M, D)
    assert (ch.nchan, ch.decim, ch.skip) == (M, D, 0)
    assert len(ch.taps) == 2 * M * 6 + 1
    ch.reset()                                       # before the first call: nothing on the device yet
    assert ld.Channelizer(M).decim == M // 2
    assert ld.Channelizer(nchan=M, decim=None, m=2, Fc=0.4 / M, As=40.0).decim == M // 2


# ---------------------------------------------------------------- design
@pytest.mark.parametrize("M,m,As", [(4, 4, 60.0), (16, 6, 60.0), (256, 8, 40.0)])
def test_default_prototype_bitwise(ld, lib, ora, M, m, As):
    ch = ld.Channelizer(M, m=m, As=As)
    ref = ora.firdes_kaiser(2 * M * m + 1, 0.5 / M, As, 0)
    assert ch.taps.dtype == np.float32 and ch.taps.shape == ref.shape
    assert (bits(ch.taps) == bits(ref)).all()
    assert np.float32(ch.scale) == np.float32(1 / np.sum(ch.taps.astype(np.float64)))
    # the same object through the C ABI
    rc, q = create(lib, M, M // 2, m, 0.0, As)
    assert rc == 0, lib.ldsp_last_error()
    Mo, Do, Lo, sk = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint(99)
    assert lib.ldsp_chan_get_info(q, C.byref(Mo), C.byref(Do), C.byref(Lo), C.byref(sk)) == 0
    assert (Mo.value, Do.value, Lo.value, sk.value) == (M, M // 2, 2 * M * m + 1, 0)
    h = np.full(Lo.value, np.nan, np.float32)
    assert lib.ldsp_chan_get_taps(q, h.ctypes.data) == 0
    assert (bits(h) == bits(ref)).all()
    s = C.c_float()
    assert lib.ldsp_chan_get_scale(q, C.byref(s)) == 0 and np.float32(s.value) == np.float32(ch.scale)
    assert lib.ldsp_chan_destroy(q) == 0


def test_cutoff_override(ld, ora):
    ch = ld.Channelizer(16, m=4, Fc=0.05)
    assert (bits(ch.taps) == bits(ora.firdes_kaiser(2 * 16 * 4 + 1, 0.05, 60.0, 0))).all()


def test_user_taps(ld):
    h = np.random.default_rng(5).standard_normal(37).astype(np.float32)
    ch = ld.Channelizer(8, 8, taps=h)
    assert (bits(ch.taps) == bits(h)).all() and ch.scale == 1.0
    ch.scale = 0.25
    assert ch.scale == 0.25
    assert len(ld.Channelizer(4, taps=[1.0]).taps) == 1
    ld.Channelizer(4, 4, taps=np.ones(17 * 4, np.float32))      # 17 taps per branch: the most supported


# ---------------------------------------------------------------- output schedule
@pytest.mark.parametrize("M,D", [(4, 4), (4, 2), (16, 8), (256, 128), (256, 256)])
def test_first_call_schedule(lib, M, D):
    # the library has no host-only way to advance the stream position, so: first calls on
    # fresh objects (the GPU streaming test pins the closed form for the later ones)
    for n in (0, 1, D - 1, D, D + 1, 5 * D + 3):
        rc, q = create(lib, M, D)
        assert rc == 0
        k = C.c_size_t(12345)
        assert lib.ldsp_chan_num_outputs(q, n, C.byref(k)) == 0
        assert k.value == -(-n // D), (n, k.value)
        assert lib.ldsp_chan_reset(q) == 0
        assert lib.ldsp_chan_num_outputs(q, n, C.byref(k)) == 0 and k.value == -(-n // D)
        lib.ldsp_chan_destroy(q)


def test_num_outputs_method(ld):
    ch = ld.Channelizer(16, 8)
    assert [ch.num_outputs(n) for n in (0, 1, 7, 8, 9, 43)] == [0, 1, 1, 1, 2, 6]


# ---------------------------------------------------------------- errors
def test_constructor_errors(ld):
    for M in (0, 2, 3, 12):
        with pytest.raises(ValueError):
            ld.Channelizer(M)
        with pytest.raises(ValueError):
            ld.Channelizer(M, M)
    for D in (0, 1, 4, 15, 32):
        with pytest.raises(ValueError):
            ld.Channelizer(16, D)
    for As in (0.0, -60.0):
        with pytest.raises(ValueError):
            ld.Channelizer(16, As=As)
    for Fc in (0.5, 0.75):
        with pytest.raises(ValueError):
            ld.Channelizer(16, Fc=Fc)
    with pytest.raises(ValueError):
        ld.Channelizer(16, taps=[])
    with pytest.raises(NotImplementedError):
        ld.Channelizer(512)
    with pytest.raises(NotImplementedError):
        ld.Channelizer(16, m=9)
    with pytest.raises(NotImplementedError):
        ld.Channelizer(4, taps=np.ones(17 * 4 + 1, np.float32))


def test_create_codes(lib):
    for M in (0, 2, 3, 12):
        assert create(lib, M, M)[0] == LDSP_EINVAL
        assert create(lib, M, M // 2)[0] == LDSP_EINVAL
    for D in (0, 4, 32):
        assert create(lib, 16, D)[0] == LDSP_EINVAL
    assert create(lib, 16, 8, As=0.0)[0] == LDSP_EINVAL
    assert create(lib, 16, 8, fc=0.5)[0] == LDSP_EINVAL
    assert create(lib, 512, 256)[0] == LDSP_EUNSUP
    assert create(lib, 16, 8, m=9)[0] == LDSP_EUNSUP
    assert lib.ldsp_chan_create(16, 8, 6, 0.0, 60.0, None) == LDSP_EINVAL
    h = np.ones(8, np.float32)
    q = C.c_void_p()
    assert lib.ldsp_chan_create_taps(8, 4, h.ctypes.data, 0, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_chan_create_taps(8, 4, None, 8, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_chan_create_taps(8, 4, h.ctypes.data, 8, None) == LDSP_EINVAL
    assert lib.ldsp_chan_create_taps(12, 6, h.ctypes.data, 8, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_chan_create_taps(512, 512, h.ctypes.data, 8, C.byref(q)) == LDSP_EUNSUP
    big = np.ones(17 * 8 + 1, np.float32)
    assert lib.ldsp_chan_create_taps(8, 4, big.ctypes.data, big.size, C.byref(q)) == LDSP_EUNSUP
    assert lib.ldsp_chan_create_taps(8, 4, big.ctypes.data, big.size - 1, C.byref(q)) == 0
    assert lib.ldsp_chan_destroy(q) == 0


def test_execute_argument_errors_need_no_gpu(lib):
    rc, q = create(lib, 8, 4)
    assert rc == 0
    x = np.zeros(64, np.complex64)
    y = np.zeros((8, 16), np.complex64)
    xp, yp = x.ctypes.data, y.ctypes.data
    k = C.c_size_t(0)
    assert lib.ldsp_chan_execute(q, xp, 64, yp, 15, C.byref(k), MEM_HOST, None) == LDSP_ERANGE
    assert k.value == 16
    assert lib.ldsp_chan_execute(q, xp, 64, yp, 15, None, MEM_HOST, None) == LDSP_ERANGE
    assert lib.ldsp_chan_execute(None, xp, 64, yp, 16, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_chan_execute(q, None, 64, yp, 16, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_chan_execute(q, xp, 64, None, 16, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_chan_execute(q, xp, 64, yp, 16, C.byref(k), 7, None) == LDSP_EINVAL
    sk = C.c_uint(99)
    assert lib.ldsp_chan_get_info(q, None, None, None, C.byref(sk)) == 0 and sk.value == 0   # nothing was consumed
    assert lib.ldsp_chan_num_outputs(q, 64, None) == LDSP_EINVAL
    assert lib.ldsp_chan_num_outputs(None, 64, C.byref(k)) == LDSP_EINVAL
    assert lib.ldsp_chan_get_taps(q, None) == LDSP_EINVAL
    assert lib.ldsp_chan_get_scale(q, None) == LDSP_EINVAL
    assert lib.ldsp_chan_reset(None) == LDSP_EINVAL
    assert lib.ldsp_chan_destroy(q) == 0


# ---------------------------------------------------------------- no GPU
def test_call_raises_without_gpu(ld):
    if ld.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ld.Channelizer(4)(np.zeros(64, np.complex64))


# ---------------------------------------------------------------- other properties
@pytest.mark.parametrize("M", [4, 16, 256])
def test_centers(ld, M):
    c = ld.Channelizer(M).centers
    k = np.arange(M)
    assert c.dtype == np.float64 and np.array_equal(c, ((k / M + 0.5) % 1) - 0.5)
    assert c[0] == 0 and c[M // 2] == -0.5 and c[M - 1] == -1 / M


def test_tile_hook(lib, ld):
    f = C.c_size_t()
    for M, D in SUPPORTED:
        assert lib.ldsp_debug_chan_tile(M, D, C.byref(f)) == 0
        assert f.value >= 32
        assert ld.Channelizer(M, D).tile == f.value
    assert lib.ldsp_debug_chan_tile(12, 6, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_chan_tile(16, 4, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_chan_tile(512, 256, C.byref(f)) == LDSP_EUNSUP
    assert lib.ldsp_debug_chan_tile(16, 8, None) == LDSP_EINVAL
