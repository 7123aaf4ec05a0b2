"""Host side of the FMBank without a GPU (CPU suite): the exported ldsp_fmbank_*
symbols, construction and defaults, the default prototype (bit-identical to the
restatement's firdes_kaiser) and its scale, user taps, the discriminator-alone
mode, num_outputs / skip over ragged call lengths against the closed form,
every argument error of ldsp_fmbank_create* / _execute (decided before any
device work) and the tile hook.  The GPU side is tests/test_gpu_fmbank.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "python-liquiddsp_amd")
LIBPATH = os.path.join(PKG, "libldsp.so")
HEADER = os.path.join(REPO, "include", "ldsp.h")

LDSP_EINVAL, LDSP_ERANGE, LDSP_EUNSUP = -1, -4, -5
MEM_HOST = 0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIBPATH):
        pytest.fail("libldsp.so not built (run __graft_entry__.build())")
    L = C.CDLL(LIBPATH)
    L.ldsp_last_error.restype = C.c_char_p
    vp, u, f, sz = C.c_void_p, C.c_uint, C.c_float, C.c_size_t
    L.ldsp_fmbank_create.argtypes = [u, f, u, u, f, f, C.POINTER(vp)]
    L.ldsp_fmbank_create_taps.argtypes = [u, f, u, vp, u, C.POINTER(vp)]
    L.ldsp_fmbank_destroy.argtypes = [vp]
    L.ldsp_fmbank_reset.argtypes = [vp]
    L.ldsp_fmbank_get_info.argtypes = [vp, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)]
    L.ldsp_fmbank_get_taps.argtypes = [vp, vp]
    L.ldsp_fmbank_get_scale.argtypes = [vp, C.POINTER(f)]
    L.ldsp_fmbank_set_scale.argtypes = [vp, f]
    L.ldsp_fmbank_num_outputs.argtypes = [vp, sz, C.POINTER(sz)]
    L.ldsp_fmbank_execute.argtypes = [vp, vp, sz, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    L.ldsp_debug_fmbank_tile.argtypes = [u, u, C.POINTER(sz)]
    return L


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def create(lib, C_=3, kf=0.25, D=8, m=6, fc=0.0, As=60.0):
    q = C.c_void_p()
    return lib.ldsp_fmbank_create(C_, kf, D, m, fc, As, C.byref(q)), q


def create_taps(lib, h, C_=3, kf=0.25, D=8, L=None):
    h = np.asarray(h, np.float32)
    q = C.c_void_p()
    return lib.ldsp_fmbank_create_taps(C_, kf, D, h.ctypes.data, h.size if L is None else L, C.byref(q)), q


def info(lib, q):
    c, d, l, s = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
    assert lib.ldsp_fmbank_get_info(q, C.byref(c), C.byref(d), C.byref(l), C.byref(s)) == 0
    return c.value, d.value, l.value, s.value


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


# ---------------------------------------------------------------- symbols
def test_library_exports_what_the_header_declares(lib):
    with open(HEADER) as f:
        names = sorted(set(re.findall(r"\b(ldsp_(?:debug_)?fmbank_\w+)\s*\(", f.read())))
    want = {"ldsp_fmbank_create", "ldsp_fmbank_create_taps", "ldsp_fmbank_destroy", "ldsp_fmbank_reset",
            "ldsp_fmbank_get_info", "ldsp_fmbank_get_taps", "ldsp_fmbank_get_scale", "ldsp_fmbank_set_scale",
            "ldsp_fmbank_num_outputs", "ldsp_fmbank_execute", "ldsp_debug_fmbank_tile"}
    assert want <= set(names), sorted(want - set(names))
    for n in names:
        assert hasattr(lib, n), n


# ---------------------------------------------------------------- construction
@pytest.mark.parametrize("D", [2, 5, 8, 64])
def test_constructs(ld, D):
    fb = ld.FMBank(3, 0.25, D)
    assert (fb.nchan, fb.kf, fb.decim, fb.skip) == (3, 0.25, D, 0)
    assert len(fb.taps) == 2 * D * 6 + 1
    fb.reset()                                       # before the first call: nothing on the device yet
    assert ld.FMBank(nchan=256, kf=0.1, decim=D, m=2, Fc=0.4 / D, As=40.0, taps=None).nchan == 256
    assert fb.tile in (128, 256)


def test_discriminator_alone(ld, lib):
    fb = ld.FMBank(16, 0.3)                          # decim = 1, no taps
    assert (fb.nchan, fb.decim, fb.skip) == (16, 1, 0)
    assert fb.taps.dtype == np.float32 and fb.taps.size == 0 and fb.scale == 1.0
    assert [fb.num_outputs(k) for k in (0, 1, 77)] == [0, 1, 77]
    with pytest.raises(ValueError):
        fb.scale = 0.5                               # no filter arithmetic: nothing to scale
    rc, q = create(lib, 16, 0.3, 1)
    assert rc == 0 and info(lib, q) == (16, 1, 0, 0)
    assert lib.ldsp_fmbank_set_scale(q, 0.5) == LDSP_EINVAL
    assert lib.ldsp_fmbank_destroy(q) == 0
    # D = 1 with taps is a full-rate filter
    full = ld.FMBank(2, 0.3, 1, taps=np.ones(17, np.float32))
    assert len(full.taps) == 17 and full.decim == 1
    full.scale = 0.25
    assert full.scale == 0.25


# ---------------------------------------------------------------- design
@pytest.mark.parametrize("D,m,As", [(2, 4, 60.0), (8, 6, 60.0), (64, 8, 80.0)])
def test_default_prototype_bitwise(ld, lib, ora, D, m, As):
    fb = ld.FMBank(2, 0.25, D, m=m, As=As)
    ref = ora.firdes_kaiser(2 * D * m + 1, 0.5 / D, As, 0)
    assert fb.taps.dtype == np.float32 and fb.taps.shape == ref.shape
    assert (bits(fb.taps) == bits(ref)).all()
    assert np.float32(fb.scale) == np.float32(1.0 / np.sum(fb.taps.astype(np.float64)))
    rc, q = create(lib, 2, 0.25, D, m, 0.0, As)
    assert rc == 0, lib.ldsp_last_error()
    assert info(lib, q) == (2, D, 2 * D * m + 1, 0)
    assert lib.ldsp_fmbank_get_info(q, None, None, None, None) == 0
    h = np.full(2 * D * m + 1, np.nan, np.float32)
    assert lib.ldsp_fmbank_get_taps(q, h.ctypes.data) == 0
    assert (bits(h) == bits(ref)).all()
    s = C.c_float()
    assert lib.ldsp_fmbank_get_scale(q, C.byref(s)) == 0 and np.float32(s.value) == np.float32(fb.scale)
    assert lib.ldsp_fmbank_destroy(q) == 0


def test_cutoff_override(ld, ora):
    fb = ld.FMBank(1, 0.25, 16, m=4, Fc=0.05)
    assert (bits(fb.taps) == bits(ora.firdes_kaiser(2 * 16 * 4 + 1, 0.05, 60.0, 0))).all()


def test_user_taps(ld):
    h = np.random.default_rng(5).standard_normal(37).astype(np.float32)
    fb = ld.FMBank(2, 0.25, 4, taps=h)
    assert (bits(fb.taps) == bits(h)).all() and fb.scale == 1.0
    fb.scale = 0.25
    assert fb.scale == 0.25
    assert len(ld.FMBank(1, 0.25, 8, taps=[1.0]).taps) == 1
    ld.FMBank(1, 0.25, 4, taps=np.ones(17 * 4, np.float32))          # 17 taps per output phase: the most supported
    ld.FMBank(1, 0.25, 64, taps=np.ones(17 * 64, np.float32))


# ---------------------------------------------------------------- the column schedule
def model(T, D, K):
    skip = (-T) % D
    ncols = -(-(K - skip) // D) if K > skip else 0
    return skip, ncols


@pytest.mark.parametrize("D", [1, 2, 5, 8, 64])
def test_num_outputs_and_skip_over_ragged_calls(ld, D):
    """Stepping the stream needs a device, so the sequence is checked through a bank's own
    bookkeeping where one is present and through the closed form at T = 0 otherwise."""
    fb = ld.FMBank(2, 0.25, D, taps=np.ones(3, np.float32))
    rng = np.random.default_rng(100 + D)
    lens = [0, 1, D - 1, D, D + 1, 0, 3 * D + 2] + [int(v) for v in rng.integers(0, 5 * D, 8)]
    T = 0
    for K in lens:
        skip, ncols = model(T, D, K)
        assert fb.skip == skip
        for k in (0, 1, D - 1, D, D + 1, K):
            assert fb.num_outputs(k) == model(T, D, k)[1], (T, k)
        if ld.device_count() == 0:
            continue                                 # the stream cannot advance: T stays 0
        y = fb(np.zeros((2, K), np.complex64))
        assert y.shape == (2, ncols)
        T += K
    fb.reset()
    assert fb.skip == 0


# ---------------------------------------------------------------- errors
def test_constructor_errors(ld):
    for C_ in (0, -1, 257):
        with pytest.raises(ValueError):
            ld.FMBank(C_, 0.25, 8)
    for D in (0, -3, 65, 1000):
        with pytest.raises(ValueError):
            ld.FMBank(3, 0.25, D)
    for kf in (0.0, -0.25, np.nan):
        with pytest.raises(ValueError):
            ld.FMBank(3, kf, 8)
    for m in (0, -1):
        with pytest.raises(ValueError):
            ld.FMBank(3, 0.25, 8, m=m)
    with pytest.raises(NotImplementedError):
        ld.FMBank(3, 0.25, 8, m=9)
    for As in (0.0, -60.0):
        with pytest.raises(ValueError):
            ld.FMBank(3, 0.25, 8, As=As)
    for Fc in (0.5, 0.75):
        with pytest.raises(ValueError):
            ld.FMBank(3, 0.25, 8, Fc=Fc)
    with pytest.raises(ValueError):
        ld.FMBank(3, 0.25, 8, taps=[])
    with pytest.raises(NotImplementedError):
        ld.FMBank(3, 0.25, 4, taps=np.ones(17 * 4 + 1, np.float32))
    with pytest.raises(NotImplementedError):
        ld.FMBank(3, 0.25, 1, taps=np.ones(18, np.float32))


def test_create_codes(lib):
    assert create(lib, C_=0)[0] == LDSP_EINVAL
    assert create(lib, C_=257)[0] == LDSP_EINVAL
    assert create(lib, D=0)[0] == LDSP_EINVAL
    assert create(lib, D=65)[0] == LDSP_EINVAL
    assert create(lib, kf=0.0)[0] == LDSP_EINVAL
    assert create(lib, kf=-1.0)[0] == LDSP_EINVAL
    assert create(lib, kf=float("nan"))[0] == LDSP_EINVAL
    assert create(lib, m=0)[0] == LDSP_EINVAL
    assert create(lib, m=9)[0] == LDSP_EUNSUP
    assert create(lib, As=0.0)[0] == LDSP_EINVAL
    assert create(lib, fc=0.5)[0] == LDSP_EINVAL
    assert lib.ldsp_fmbank_create(3, 0.25, 8, 6, 0.0, 60.0, None) == LDSP_EINVAL
    h = np.ones(8, np.float32)
    q = C.c_void_p()
    assert create_taps(lib, h, L=0)[0] == LDSP_EINVAL
    assert create_taps(lib, h, C_=0)[0] == LDSP_EINVAL
    assert create_taps(lib, h, C_=257)[0] == LDSP_EINVAL
    assert create_taps(lib, h, D=0)[0] == LDSP_EINVAL
    assert create_taps(lib, h, D=65)[0] == LDSP_EINVAL
    assert create_taps(lib, h, kf=0.0)[0] == LDSP_EINVAL
    assert lib.ldsp_fmbank_create_taps(3, 0.25, 8, None, 8, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_fmbank_create_taps(3, 0.25, 8, h.ctypes.data, 8, None) == LDSP_EINVAL
    big = np.ones(17 * 8 + 1, np.float32)
    assert create_taps(lib, big)[0] == LDSP_EUNSUP
    rc, q = create_taps(lib, big, L=big.size - 1)
    assert rc == 0 and lib.ldsp_fmbank_destroy(q) == 0
    for C_, D in ((1, 1), (256, 64)):                # the ends of the ranges are allowed
        rc, q = create(lib, C_=C_, D=D)
        assert rc == 0 and lib.ldsp_fmbank_destroy(q) == 0


def test_execute_argument_errors_need_no_gpu(lib):
    rc, q = create(lib, 3, 0.25, 4)
    assert rc == 0
    x = np.zeros((3, 64), np.complex64)
    y = np.zeros((3, 20), np.float32)
    xp, yp = x.ctypes.data, y.ctypes.data
    k = C.c_size_t(0)
    assert lib.ldsp_fmbank_execute(q, xp, 64, 64, yp, 15, C.byref(k), MEM_HOST, None) == LDSP_ERANGE
    assert k.value == 16
    assert lib.ldsp_fmbank_execute(q, xp, 64, 64, yp, 15, None, MEM_HOST, None) == LDSP_ERANGE
    assert lib.ldsp_fmbank_execute(q, xp, 63, 64, yp, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_fmbank_execute(None, xp, 64, 64, yp, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_fmbank_execute(q, None, 64, 64, yp, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_fmbank_execute(q, xp, 64, 64, None, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_fmbank_execute(q, xp, 64, 64, yp, 20, C.byref(k), 7, None) == LDSP_EINVAL
    # the object is untouched: the same taps, scale and counts as a fresh one
    rc, f = create(lib, 3, 0.25, 4)
    a, b = np.zeros(49, np.float32), np.ones(49, np.float32)
    assert lib.ldsp_fmbank_get_taps(q, a.ctypes.data) == 0 and lib.ldsp_fmbank_get_taps(f, b.ctypes.data) == 0
    assert (bits(a) == bits(b)).all()
    sa, sb = C.c_float(), C.c_float(1.0)
    assert lib.ldsp_fmbank_get_scale(q, C.byref(sa)) == 0 and lib.ldsp_fmbank_get_scale(f, C.byref(sb)) == 0
    assert sa.value == sb.value
    assert info(lib, q) == info(lib, f) == (3, 4, 49, 0)
    assert lib.ldsp_fmbank_num_outputs(q, 64, C.byref(k)) == 0 and k.value == 16
    assert lib.ldsp_fmbank_num_outputs(q, 64, None) == LDSP_EINVAL
    assert lib.ldsp_fmbank_num_outputs(None, 64, C.byref(k)) == LDSP_EINVAL
    assert lib.ldsp_fmbank_get_taps(q, None) == LDSP_EINVAL
    assert lib.ldsp_fmbank_get_scale(q, None) == LDSP_EINVAL
    assert lib.ldsp_fmbank_reset(None) == LDSP_EINVAL
    assert lib.ldsp_fmbank_reset(q) == 0
    assert lib.ldsp_fmbank_destroy(q) == 0 and lib.ldsp_fmbank_destroy(f) == 0
    assert lib.ldsp_fmbank_destroy(None) == 0


def test_python_shape_errors_need_no_gpu(ld):
    fb = ld.FMBank(3, 0.25, 4)
    for bad in (np.zeros((2, 64), np.complex64), np.zeros((4, 64), np.complex64), np.zeros(64, np.complex64),
                np.zeros((3, 4, 4), np.complex64)):
        with pytest.raises(ValueError):
            fb(bad)
    assert fb.skip == 0


def test_call_raises_without_gpu(ld):
    if ld.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ld.FMBank(2, 0.25, 4)(np.zeros((2, 64), np.complex64))


# ---------------------------------------------------------------- the tile hook
# 256 columns per workgroup, or 128 where the span of 256 takes more than 40 KiB of LDS
TILES = [(1, 0, 256), (1, 17, 256), (2, 25, 256), (8, 3, 256), (8, 97, 256), (4, 37, 256), (32, 385, 256),
         (37, 17 * 37, 256), (38, 17 * 38, 128), (64, 769, 128), (64, 17 * 64, 128), (64, 1, 128)]


def test_tile_hook(lib, ld):
    f = C.c_size_t()
    for D, L, want in TILES:
        assert lib.ldsp_debug_fmbank_tile(D, L, C.byref(f)) == 0
        assert f.value == want, (D, L)
        if L:
            assert ld.FMBank(1, 0.25, D, taps=np.ones(L, np.float32)).tile == want
    assert ld.FMBank(4, 0.25).tile == 256 and ld.FMBank(4, 0.25, 64).tile == 128
    assert lib.ldsp_debug_fmbank_tile(0, 8, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_fmbank_tile(65, 8, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_fmbank_tile(8, 17 * 8 + 1, C.byref(f)) == LDSP_EUNSUP
    assert lib.ldsp_debug_fmbank_tile(8, 8, None) == LDSP_EINVAL
