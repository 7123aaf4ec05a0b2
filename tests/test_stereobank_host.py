"""Host side of the StereoBank without a GPU (CPU suite): the exported
ldsp_stbank_* symbols, construction and defaults, the designed prototypes
(bit-identical to the restatement's firdes_kaiser normalised the same way), user
taps, the pilot word, num_outputs / skip over ragged call lengths against the
closed form, every argument error of ldsp_stbank_create* / _execute (decided
before any device work) and the tile hook.  The GPU side is
tests/test_gpu_stereobank.py."""
import ctypes as C
import math
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
PILOT = 0.076


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIBPATH):
        pytest.fail("libldsp.so not built (run __graft_entry__.build())")
    L = C.CDLL(LIBPATH)
    L.ldsp_last_error.restype = C.c_char_p
    vp, u, f, d, sz = C.c_void_p, C.c_uint, C.c_float, C.c_double, C.c_size_t
    L.ldsp_stbank_create.argtypes = [u, d, u, u, f, f, C.POINTER(vp)]
    L.ldsp_stbank_create_taps.argtypes = [u, d, u, vp, u, vp, u, f, C.POINTER(vp)]
    L.ldsp_stbank_destroy.argtypes = [vp]
    L.ldsp_stbank_reset.argtypes = [vp]
    L.ldsp_stbank_get_info.argtypes = [vp, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u),
                                       C.POINTER(C.c_uint32)]
    L.ldsp_stbank_get_taps.argtypes = [vp, vp, vp]
    L.ldsp_stbank_get_threshold.argtypes = [vp, C.POINTER(f)]
    L.ldsp_stbank_set_threshold.argtypes = [vp, f]
    L.ldsp_stbank_num_outputs.argtypes = [vp, sz, C.POINTER(sz)]
    L.ldsp_stbank_execute.argtypes = [vp, vp, sz, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    L.ldsp_stbank_get_pilot_level.argtypes = [vp, vp]
    L.ldsp_debug_stbank_tile.argtypes = [u, u, C.POINTER(sz)]
    return L


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def create(lib, C_=3, pilot=PILOT, D=5, L=0, As=60.0, thr=0.01):
    q = C.c_void_p()
    return lib.ldsp_stbank_create(C_, pilot, D, L, As, thr, C.byref(q)), q


def create_taps(lib, h, g, C_=3, pilot=PILOT, D=5, thr=0.01, L=None, Lg=None):
    h, g = np.asarray(h, np.float32), np.asarray(g, np.float32)
    q = C.c_void_p()
    return lib.ldsp_stbank_create_taps(C_, pilot, D, h.ctypes.data, h.size if L is None else L, g.ctypes.data,
                                       g.size if Lg is None else Lg, thr, C.byref(q)), q


def info(lib, q):
    c, d, l, s, w = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint32()
    assert lib.ldsp_stbank_get_info(q, C.byref(c), C.byref(d), C.byref(l), C.byref(s), C.byref(w)) == 0
    return c.value, d.value, l.value, s.value, w.value


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def designed(ora, L, fc, As):
    """firdes_kaiser with every tap divided in double by the double sum of the float32 design."""
    h = ora.firdes_kaiser(L, np.float32(fc), As, 0)
    return (h.astype(np.float64) / np.sum(h.astype(np.float64))).astype(np.float32)


# ---------------------------------------------------------------- symbols
def test_library_exports_what_the_header_declares(lib):
    with open(HEADER) as f:
        names = sorted(set(re.findall(r"\b(ldsp_(?:debug_)?stbank_\w+)\s*\(", f.read())))
    want = {"ldsp_stbank_create", "ldsp_stbank_create_taps", "ldsp_stbank_destroy", "ldsp_stbank_reset",
            "ldsp_stbank_get_info", "ldsp_stbank_get_taps", "ldsp_stbank_get_threshold", "ldsp_stbank_set_threshold",
            "ldsp_stbank_num_outputs", "ldsp_stbank_execute", "ldsp_stbank_get_pilot_level", "ldsp_debug_stbank_tile"}
    assert want == set(names), sorted(want ^ set(names))
    for n in names:
        assert hasattr(lib, n), n


# ---------------------------------------------------------------- construction
def test_defaults(ld):
    sb = ld.StereoBank(16, PILOT)
    assert (sb.nchan, sb.decim, sb.skip, sb.tile) == (16, 1, 0, 64)
    assert sb.threshold == np.float32(0.01)
    assert len(sb.taps) == len(sb.pilot_taps) == 2 * math.ceil(8.5 / PILOT) + 1 == 225
    assert sb.taps.dtype == sb.pilot_taps.dtype == np.float32
    assert sb.pilot_level.dtype == np.float32 and (sb.pilot_level == 0).all() and sb.pilot_level.shape == (16,)
    assert sb.stereo.dtype == bool and not sb.stereo.any()
    sb.reset()                                       # before the first call: nothing on the device yet
    sb.threshold = 0.25
    assert sb.threshold == 0.25
    sb.threshold = 0.0                               # allowed: every column with m > 0 is decoded
    kw = ld.StereoBank(nchan=128, pilot=0.1, decim=32, ntaps=1025, As=40.0, threshold=0.02, taps=None, pilot_taps=None)
    assert (kw.nchan, kw.decim, len(kw.taps), kw.threshold) == (128, 32, 1025, np.float32(0.02))
    assert len(ld.StereoBank(1, 0.2, ntaps=1).taps) == 1


@pytest.mark.parametrize("pilot", [19e3 / 250e3, 0.095, 0.2])
def test_pilot_word(ld, lib, pilot):
    w = int(np.rint(pilot * 2.0 ** 32)) % 2 ** 32    # the product is exact, ties to even
    sb = ld.StereoBank(2, pilot, 4)
    assert sb.word == w and sb.pilot == w / 2.0 ** 32
    assert abs(sb.pilot - pilot) <= 2.0 ** -33
    rc, q = create(lib, 2, pilot, 4)
    assert rc == 0 and info(lib, q) == (2, 4, 2 * math.ceil(8.5 / pilot) + 1, 0, w)
    assert lib.ldsp_stbank_get_info(q, None, None, None, None, None) == 0
    assert lib.ldsp_stbank_destroy(q) == 0


# ---------------------------------------------------------------- design
@pytest.mark.parametrize("pilot,L,As", [(PILOT, None, 60.0), (0.095, None, 60.0), (0.2, 33, 80.0), (0.05, 1025, 40.0)])
def test_designed_prototypes_bitwise(ld, lib, ora, pilot, L, As):
    sb = ld.StereoBank(2, pilot, 5, ntaps=L, As=As)
    n = L or 2 * math.ceil(8.5 / pilot) + 1
    h, g = designed(ora, n, 17.0 / 19.0 * pilot, As), designed(ora, n, 2.0 / 19.0 * pilot, As)
    assert sb.taps.shape == h.shape and (bits(sb.taps) == bits(h)).all()
    assert sb.pilot_taps.shape == g.shape and (bits(sb.pilot_taps) == bits(g)).all()
    assert abs(np.sum(sb.taps.astype(np.float64)) - 1) < 1e-6 and abs(np.sum(sb.pilot_taps.astype(np.float64)) - 1) < 1e-6
    rc, q = create(lib, 2, pilot, 5, L or 0, As)
    assert rc == 0, lib.ldsp_last_error()
    a, b = np.full(n, np.nan, np.float32), np.full(n, np.nan, np.float32)
    assert lib.ldsp_stbank_get_taps(q, a.ctypes.data, b.ctypes.data) == 0
    assert (bits(a) == bits(h)).all() and (bits(b) == bits(g)).all()
    assert lib.ldsp_stbank_get_taps(q, None, None) == 0
    assert lib.ldsp_stbank_destroy(q) == 0


def test_user_taps(ld):
    rng = np.random.default_rng(5)
    h, g = rng.standard_normal(37).astype(np.float32), rng.standard_normal(37).astype(np.float32)
    sb = ld.StereoBank(2, PILOT, 4, taps=h, pilot_taps=g)
    assert (bits(sb.taps) == bits(h)).all() and (bits(sb.pilot_taps) == bits(g)).all()
    one = ld.StereoBank(1, PILOT, 8, taps=[1.0], pilot_taps=[0.5])
    assert len(one.taps) == 1 and one.pilot_taps[0] == 0.5
    ld.StereoBank(1, PILOT, 1, taps=np.ones(1025, np.float32), pilot_taps=np.ones(1025, np.float32))   # the longest


# ---------------------------------------------------------------- the column schedule
def model(T, D, K):
    skip = (-T) % D
    ncols = -(-(K - skip) // D) if K > skip else 0
    return skip, ncols


@pytest.mark.parametrize("D", [1, 2, 5, 8, 32])
def test_num_outputs_and_skip_over_ragged_calls(ld, D):
    """Stepping the stream needs a device, so the sequence is checked through a bank's own
    bookkeeping where one is present and through the closed form at T = 0 otherwise."""
    sb = ld.StereoBank(2, PILOT, D, ntaps=3)
    rng = np.random.default_rng(100 + D)
    lens = [0, 1, D - 1, D, D + 1, 0, 3 * D + 2] + [int(v) for v in rng.integers(0, 5 * D, 8)]
    T = 0
    for K in lens:
        skip, ncols = model(T, D, K)
        assert sb.skip == skip
        for k in (0, 1, D - 1, D, D + 1, K):
            assert sb.num_outputs(k) == model(T, D, k)[1], (T, k)
        if ld.device_count() == 0:
            continue                                 # the stream cannot advance: T stays 0
        y = sb(np.zeros((2, K), np.float32))
        assert y.shape == (2, 2, ncols)
        T += K
    sb.reset()
    assert sb.skip == 0


# ---------------------------------------------------------------- errors
def test_constructor_errors(ld):
    for C_ in (0, -1, 129):
        with pytest.raises(ValueError):
            ld.StereoBank(C_, PILOT, 5)
    for D in (0, -3, 33, 1000):
        with pytest.raises(ValueError):
            ld.StereoBank(3, PILOT, D)
    for pilot in (0.0, -0.076, 0.25, 0.3, np.nan, np.inf):
        with pytest.raises(ValueError):
            ld.StereoBank(3, pilot, 5)
    for n in (0, -1, 1026):
        with pytest.raises(ValueError):
            ld.StereoBank(3, PILOT, 5, ntaps=n)
    for As in (0.0, -60.0, np.nan):
        with pytest.raises(ValueError):
            ld.StereoBank(3, PILOT, 5, As=As)
    for thr in (-0.01, np.nan):
        with pytest.raises(ValueError):
            ld.StereoBank(3, PILOT, 5, threshold=thr)
    with pytest.raises(NotImplementedError):
        ld.StereoBank(3, 0.016, 5)                   # default L = 1065
    assert len(ld.StereoBank(3, 0.0167, 5).taps) == 1019
    assert len(ld.StereoBank(3, 0.016, 5, ntaps=1025).taps) == 1025
    ones = np.ones(8, np.float32)
    for kw in (dict(taps=ones), dict(pilot_taps=ones), dict(taps=ones, pilot_taps=ones[:7]), dict(taps=[], pilot_taps=[]),
               dict(taps=ones, pilot_taps=ones, ntaps=8), dict(taps=np.ones(1026), pilot_taps=np.ones(1026))):
        with pytest.raises(ValueError):
            ld.StereoBank(3, PILOT, 5, **kw)
    sb = ld.StereoBank(3, PILOT, 5)
    for thr in (-1.0, np.nan):
        with pytest.raises(ValueError):
            sb.threshold = thr
    assert sb.threshold == np.float32(0.01)


def test_create_codes(lib):
    for kw in (dict(C_=0), dict(C_=129), dict(D=0), dict(D=33), dict(pilot=0.0), dict(pilot=-0.1), dict(pilot=0.25),
               dict(pilot=float("nan")), dict(L=1026), dict(As=0.0), dict(As=float("nan")), dict(thr=-0.5),
               dict(thr=float("nan"))):
        assert create(lib, **kw)[0] == LDSP_EINVAL, kw
    assert create(lib, pilot=0.016)[0] == LDSP_EUNSUP
    assert lib.ldsp_stbank_create(3, PILOT, 5, 0, 60.0, 0.01, None) == LDSP_EINVAL
    h = np.ones(8, np.float32)
    q = C.c_void_p()
    for kw in (dict(C_=0), dict(C_=129), dict(D=0), dict(D=33), dict(pilot=0.0), dict(pilot=0.25), dict(thr=-1.0), dict(L=0),
               dict(L=0, Lg=0), dict(Lg=7), dict(L=7), dict(L=1026, Lg=1026)):
        assert create_taps(lib, h, h, **kw)[0] == LDSP_EINVAL, kw
    assert lib.ldsp_stbank_create_taps(3, PILOT, 5, None, 8, h.ctypes.data, 8, 0.01, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_stbank_create_taps(3, PILOT, 5, h.ctypes.data, 8, None, 8, 0.01, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_stbank_create_taps(3, PILOT, 5, h.ctypes.data, 8, h.ctypes.data, 8, 0.01, None) == LDSP_EINVAL
    for C_, D, L in ((1, 1, 1), (128, 32, 1025)):    # the ends of the ranges are allowed
        rc, q = create(lib, C_=C_, D=D, L=L, thr=0.0)
        assert rc == 0 and lib.ldsp_stbank_destroy(q) == 0


def test_execute_argument_errors_need_no_gpu(lib):
    rc, q = create(lib, 3, PILOT, 4)
    assert rc == 0
    x = np.zeros((3, 64), np.float32)
    y = np.zeros((6, 20), np.float32)
    xp, yp = x.ctypes.data, y.ctypes.data
    k = C.c_size_t(0)
    assert lib.ldsp_stbank_execute(q, xp, 64, 64, yp, 15, C.byref(k), MEM_HOST, None) == LDSP_ERANGE
    assert k.value == 16
    assert lib.ldsp_stbank_execute(q, xp, 64, 64, yp, 15, None, MEM_HOST, None) == LDSP_ERANGE
    assert lib.ldsp_stbank_execute(q, xp, 63, 64, yp, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_stbank_execute(None, xp, 64, 64, yp, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_stbank_execute(q, None, 64, 64, yp, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_stbank_execute(q, xp, 64, 64, None, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_stbank_execute(q, xp, 64, 64, yp, 20, C.byref(k), 7, None) == LDSP_EINVAL
    # the object is untouched: the same geometry, threshold and level as a fresh one
    rc, f = create(lib, 3, PILOT, 4)
    assert info(lib, q) == info(lib, f) and info(lib, q)[:4] == (3, 4, 225, 0)
    t = C.c_float(-1.0)
    assert lib.ldsp_stbank_get_threshold(q, C.byref(t)) == 0 and np.float32(t.value) == np.float32(0.01)
    assert lib.ldsp_stbank_set_threshold(q, -0.5) == LDSP_EINVAL
    assert lib.ldsp_stbank_set_threshold(q, 0.05) == 0
    assert lib.ldsp_stbank_get_threshold(q, C.byref(t)) == 0 and np.float32(t.value) == np.float32(0.05)
    lv = np.full(3, np.nan, np.float32)
    assert lib.ldsp_stbank_get_pilot_level(q, lv.ctypes.data) == 0 and (lv == 0).all()
    assert lib.ldsp_stbank_get_pilot_level(q, None) == LDSP_EINVAL
    assert lib.ldsp_stbank_get_pilot_level(None, lv.ctypes.data) == LDSP_EINVAL
    assert lib.ldsp_stbank_num_outputs(q, 64, C.byref(k)) == 0 and k.value == 16
    assert lib.ldsp_stbank_num_outputs(q, 64, None) == LDSP_EINVAL
    assert lib.ldsp_stbank_num_outputs(None, 64, C.byref(k)) == LDSP_EINVAL
    assert lib.ldsp_stbank_get_taps(None, None, None) == LDSP_EINVAL
    assert lib.ldsp_stbank_get_threshold(q, None) == LDSP_EINVAL
    assert lib.ldsp_stbank_get_threshold(None, C.byref(t)) == LDSP_EINVAL
    assert lib.ldsp_stbank_set_threshold(None, 0.1) == LDSP_EINVAL
    assert lib.ldsp_stbank_reset(None) == LDSP_EINVAL
    assert lib.ldsp_stbank_reset(q) == 0
    assert lib.ldsp_stbank_destroy(q) == 0 and lib.ldsp_stbank_destroy(f) == 0
    assert lib.ldsp_stbank_destroy(None) == 0


def test_python_shape_errors_need_no_gpu(ld):
    sb = ld.StereoBank(3, PILOT, 4)
    for bad in (np.zeros((2, 64), np.float32), np.zeros((4, 64), np.float32), np.zeros(64, np.float32),
                np.zeros((3, 4, 4), np.float32)):
        with pytest.raises(ValueError):
            sb(bad)
    assert sb.skip == 0
    if ld.device_count() == 0:                       # a well-formed call without a device is an error, not a fallback
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            sb(np.zeros((3, 64), np.float32))


# ---------------------------------------------------------------- the tile hook
def test_tile_hook(lib, ld):
    """64 columns per workgroup at every (D, L): the widest span, D = 32 with L = 1025, takes 17 KiB of LDS."""
    f = C.c_size_t()
    for D, L in ((1, 1), (1, 1025), (5, 225), (8, 363), (32, 1), (32, 1025)):
        assert lib.ldsp_debug_stbank_tile(D, L, C.byref(f)) == 0
        assert f.value == 64, (D, L)
        assert ld.StereoBank(1, PILOT, D, ntaps=L).tile == 64
    assert lib.ldsp_debug_stbank_tile(0, 8, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_stbank_tile(33, 8, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_stbank_tile(8, 0, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_stbank_tile(8, 1026, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_stbank_tile(8, 8, None) == LDSP_EINVAL
