"""Host side of the SquelchBank without a GPU (CPU suite): the exported
ldsp_sqbank_* symbols, construction and defaults with scalar and per-row
thresholds, the dB -> float32 threshold conversion bit for bit, num_outputs /
fill over ragged call lengths against the closed form, every argument error of
ldsp_sqbank_create / _set_thresholds / _execute (decided before any device
work) and the tile hook.  The GPU side is tests/test_gpu_squelchbank.py."""
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

LDSP_EINVAL, LDSP_ERANGE = -1, -4
MEM_HOST = 0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIBPATH):
        pytest.fail("libldsp.so not built (run __graft_entry__.build())")
    L = C.CDLL(LIBPATH)
    L.ldsp_last_error.restype = C.c_char_p
    vp, u, d, sz = C.c_void_p, C.c_uint, C.c_double, C.c_size_t
    L.ldsp_sqbank_create.argtypes = [u, u, d, d, u, C.POINTER(vp)]
    L.ldsp_sqbank_destroy.argtypes = [vp]
    L.ldsp_sqbank_reset.argtypes = [vp]
    L.ldsp_sqbank_set_thresholds.argtypes = [vp, vp, u]
    L.ldsp_sqbank_get_thresholds.argtypes = [vp, vp, vp]
    L.ldsp_sqbank_get_info.argtypes = [vp, C.POINTER(u), C.POINTER(u), C.POINTER(d), C.POINTER(u), C.POINTER(u)]
    L.ldsp_sqbank_num_outputs.argtypes = [vp, sz, C.POINTER(sz)]
    L.ldsp_sqbank_execute.argtypes = [vp, vp, sz, sz, vp, sz, vp, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    L.ldsp_sqbank_get_state.argtypes = [vp, vp, vp, vp]
    L.ldsp_debug_sqbank_tile.argtypes = [u, C.POINTER(sz)]
    return L


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def create(lib, C_=3, B=64, alpha=0.25, dB=-30.0, timeout=4):
    q = C.c_void_p()
    return lib.ldsp_sqbank_create(C_, B, alpha, dB, timeout, C.byref(q)), q


def info(lib, q):
    c, b, a, t, f = C.c_uint(), C.c_uint(), C.c_double(), C.c_uint(), C.c_uint()
    assert lib.ldsp_sqbank_get_info(q, C.byref(c), C.byref(b), C.byref(a), C.byref(t), C.byref(f)) == 0
    return c.value, b.value, a.value, t.value, f.value


def thresholds(lib, q, n):
    db, lin = np.full(n, np.nan), np.full(n, np.nan, np.float32)
    assert lib.ldsp_sqbank_get_thresholds(q, db.ctypes.data, lin.ctypes.data) == 0
    return db, lin


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def lin_of(dB):
    """The definition's threshold: 10 ** (dB / 10) in double, rounded to float32 once."""
    return np.array([np.float32(10.0 ** (float(v) / 10)) for v in np.atleast_1d(dB)], np.float32)


# ---------------------------------------------------------------- symbols
def test_library_exports_what_the_header_declares(lib):
    with open(HEADER) as f:
        names = sorted(set(re.findall(r"\b(ldsp_(?:debug_)?sqbank_\w+)\s*\(", f.read())))
    want = {"ldsp_sqbank_create", "ldsp_sqbank_destroy", "ldsp_sqbank_reset", "ldsp_sqbank_set_thresholds",
            "ldsp_sqbank_get_thresholds", "ldsp_sqbank_get_info", "ldsp_sqbank_num_outputs", "ldsp_sqbank_execute",
            "ldsp_sqbank_get_state", "ldsp_debug_sqbank_tile"}
    assert want <= set(names), sorted(want - set(names))
    for n in names:
        assert hasattr(lib, n), n


# ---------------------------------------------------------------- construction
def test_defaults(ld):
    sq = ld.SquelchBank(5)
    assert (sq.nchan, sq.block, sq.bandwidth, sq.timeout, sq.fill) == (5, 1024, 0.25, 4, 0)
    assert sq.threshold.dtype == np.float64 and (sq.threshold == -30.0).all() and sq.threshold.shape == (5,)
    assert sq.threshold_linear.dtype == np.float32 and (bits(sq.threshold_linear) == bits(lin_of([-30.0] * 5))).all()
    assert sq.status is None and sq.level is None            # no call yet
    mode, timer, s = sq.state
    assert (mode == 1).all() and (timer == 0).all() and (s == 0.0).all()      # ENABLED, before any device work
    sq.reset()                                               # before the first call: nothing on the device yet


@pytest.mark.parametrize("B", [16, 17, 100, 1024, 4095, 4096])
def test_constructs_over_block_lengths(ld, B):
    sq = ld.SquelchBank(nchan=256, block=B, threshold=-10.0, bandwidth=1.0, timeout=1)
    assert (sq.nchan, sq.block, sq.bandwidth, sq.timeout) == (256, B, 1.0, 1)
    assert sq.num_outputs(B - 1) == 0 and sq.num_outputs(B) == 1 and sq.num_outputs(3 * B + 1) == 3


def test_per_row_thresholds(ld, lib):
    dB = [-10.0, -12.5, 3.0, -33.3]
    sq = ld.SquelchBank(4, 64, dB)
    assert (sq.threshold == np.array(dB)).all()
    assert (bits(sq.threshold_linear) == bits(lin_of(dB))).all()
    sq.threshold = -7.25                                     # a scalar: every row
    assert (sq.threshold == -7.25).all() and (bits(sq.threshold_linear) == bits(lin_of([-7.25] * 4))).all()
    sq.threshold = np.array(dB[::-1], np.float32)            # any array-like of nchan values
    assert (sq.threshold == np.array(dB[::-1], np.float32).astype(np.float64)).all()
    for bad in ([-10.0, -20.0], [-10.0] * 5, [], [[-10.0] * 4] * 2):
        with pytest.raises(ValueError):
            sq.threshold = bad
    with pytest.raises(ValueError):
        ld.SquelchBank(4, 64, [-10.0, -20.0])
    assert (sq.threshold == np.array(dB[::-1], np.float32).astype(np.float64)).all()      # refused setters change nothing
    rc, q = create(lib, 4, 64, 0.25, -10.0, 4)
    assert rc == 0
    v = np.array(dB)
    assert lib.ldsp_sqbank_set_thresholds(q, v.ctypes.data, 4) == 0
    db, lin = thresholds(lib, q, 4)
    assert (db == v).all() and (bits(lin) == bits(lin_of(dB))).all()
    assert lib.ldsp_sqbank_get_thresholds(q, None, None) == 0
    assert lib.ldsp_sqbank_destroy(q) == 0


@pytest.mark.parametrize("dB", [-30.0, -10.0, 0.0, 3.0, -12.5, -33.3, 0.1, -6.0206, 17.77, -99.9])
def test_threshold_conversion_bitwise(ld, dB):
    sq = ld.SquelchBank(2, 64, dB)
    want = np.float32(10.0 ** (dB / 10))
    assert (bits(sq.threshold_linear) == bits(want)).all(), (dB, sq.threshold_linear, want)
    sq.threshold = [dB - 0.37, dB + 0.37]
    assert bits(sq.threshold_linear)[0] == bits(np.float32(10.0 ** ((dB - 0.37) / 10)))[0]
    assert bits(sq.threshold_linear)[1] == bits(np.float32(10.0 ** ((dB + 0.37) / 10)))[0]


# ---------------------------------------------------------------- the block schedule
def model(T, B, K):
    return (T + K) // B - T // B, (T + K) % B


@pytest.mark.parametrize("B", [16, 17, 100, 1024])
def test_num_outputs_and_fill_over_ragged_calls(ld, B):
    """Stepping the stream needs a device, so the sequence is checked through a bank's own
    bookkeeping where one is present and through the closed form at T = 0 otherwise."""
    sq = ld.SquelchBank(2, B)
    rng = np.random.default_rng(100 + B)
    lens = [0, 1, B - 1, B, B + 1, 0, 3 * B + 2] + [int(v) for v in rng.integers(0, 5 * B, 8)]
    T = 0
    for i, K in enumerate(lens):
        assert sq.fill == T % B
        for k in (0, 1, B - 1, B, B + 1, K):
            assert sq.num_outputs(k) == model(T, B, k)[0], (T, k)
        if ld.device_count() == 0:
            continue                                 # the stream cannot advance: T stays 0
        nb, fill = model(T, B, K)
        x = np.zeros((2, K), np.complex64)
        if i % 2:
            y = sq(x)
            assert y.shape == (2, nb * B)
        else:
            st, lv = sq.measure(x)
            assert st.shape == lv.shape == (2, nb)
        T += K
        assert sq.fill == fill
    sq.reset()
    assert sq.fill == 0


# ---------------------------------------------------------------- errors
def test_constructor_errors(ld):
    for C_ in (0, -1, 257):
        with pytest.raises(ValueError):
            ld.SquelchBank(C_)
    for B in (0, -1, 15, 4097):
        with pytest.raises(ValueError):
            ld.SquelchBank(3, B)
    for a in (0.0, -0.25, 1.0000001, np.nan, np.inf):
        with pytest.raises(ValueError):
            ld.SquelchBank(3, bandwidth=a)
    for t in (0, -1):
        with pytest.raises(ValueError):
            ld.SquelchBank(3, timeout=t)
    for dB in (np.nan, np.inf, -np.inf, [-10.0, np.nan, -10.0]):
        with pytest.raises(ValueError):
            ld.SquelchBank(3, threshold=dB)


def test_create_codes(lib):
    for kw in (dict(C_=0), dict(C_=257), dict(B=0), dict(B=15), dict(B=4097), dict(alpha=0.0), dict(alpha=-0.5),
               dict(alpha=1.5), dict(alpha=float("nan")), dict(alpha=float("inf")), dict(timeout=0),
               dict(dB=float("nan")), dict(dB=float("inf")), dict(dB=float("-inf"))):
        assert create(lib, **kw)[0] == LDSP_EINVAL, kw
    assert lib.ldsp_sqbank_create(3, 64, 0.25, -30.0, 4, None) == LDSP_EINVAL
    for kw in (dict(C_=1, B=16, alpha=1.0, timeout=1), dict(C_=256, B=4096, alpha=1e-9, timeout=1 << 20, dB=300.0)):
        rc, q = create(lib, **kw)                    # the ends of the ranges are allowed
        assert rc == 0, (kw, lib.ldsp_last_error())
        assert lib.ldsp_sqbank_destroy(q) == 0


def test_set_thresholds_codes(lib):
    rc, q = create(lib, 3)
    assert rc == 0
    v = np.array([-10.0, -20.0, -30.0, -40.0])
    before = thresholds(lib, q, 3)
    assert lib.ldsp_sqbank_set_thresholds(q, v.ctypes.data, 0) == LDSP_EINVAL
    assert lib.ldsp_sqbank_set_thresholds(q, v.ctypes.data, 2) == LDSP_EINVAL
    assert lib.ldsp_sqbank_set_thresholds(q, v.ctypes.data, 4) == LDSP_EINVAL
    assert lib.ldsp_sqbank_set_thresholds(q, None, 3) == LDSP_EINVAL
    assert lib.ldsp_sqbank_set_thresholds(None, v.ctypes.data, 3) == LDSP_EINVAL
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[1] = bad
        assert lib.ldsp_sqbank_set_thresholds(q, w.ctypes.data, 3) == LDSP_EINVAL
        assert lib.ldsp_sqbank_set_thresholds(q, w[1:].ctypes.data, 1) == LDSP_EINVAL
    after = thresholds(lib, q, 3)                    # refused: nothing changed
    assert (before[0] == after[0]).all() and (bits(before[1]) == bits(after[1])).all()
    assert lib.ldsp_sqbank_set_thresholds(q, v.ctypes.data, 1) == 0
    assert (thresholds(lib, q, 3)[0] == -10.0).all()
    assert lib.ldsp_sqbank_set_thresholds(q, v.ctypes.data, 3) == 0
    assert (thresholds(lib, q, 3)[0] == v[:3]).all()
    assert lib.ldsp_sqbank_get_thresholds(None, None, None) == LDSP_EINVAL
    assert lib.ldsp_sqbank_destroy(q) == 0


def test_execute_argument_errors_need_no_gpu(lib):
    rc, q = create(lib, 3, 16)
    assert rc == 0
    x = np.zeros((3, 64), np.complex64)
    st, lv, y = np.zeros((3, 4), np.uint8), np.zeros((3, 4), np.float32), np.zeros((3, 64), np.complex64)
    xp, sp, lp, yp = x.ctypes.data, st.ctypes.data, lv.ctypes.data, y.ctypes.data
    k = C.c_size_t(0)
    ex = lib.ldsp_sqbank_execute
    assert ex(q, xp, 64, 64, sp, 3, lp, 4, yp, 64, C.byref(k), MEM_HOST, None) == LDSP_ERANGE       # lds
    assert k.value == 4
    assert ex(q, xp, 64, 64, sp, 4, lp, 3, yp, 64, C.byref(k), MEM_HOST, None) == LDSP_ERANGE       # ldl
    assert ex(q, xp, 64, 64, sp, 4, lp, 4, yp, 63, C.byref(k), MEM_HOST, None) == LDSP_ERANGE       # ldy
    assert ex(q, xp, 64, 64, sp, 4, lp, 4, yp, 63, None, MEM_HOST, None) == LDSP_ERANGE
    assert ex(q, xp, 64, 64, sp, 3, lp, 4, None, 0, C.byref(k), MEM_HOST, None) == LDSP_ERANGE      # measuring
    assert ex(q, xp, 63, 64, sp, 4, lp, 4, yp, 64, C.byref(k), MEM_HOST, None) == LDSP_EINVAL       # ldx < K
    assert ex(None, xp, 64, 64, sp, 4, lp, 4, yp, 64, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert ex(q, None, 64, 64, sp, 4, lp, 4, yp, 64, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert ex(q, xp, 64, 64, None, 4, lp, 4, yp, 64, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert ex(q, xp, 64, 64, sp, 4, None, 4, yp, 64, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert ex(q, xp, 64, 64, sp, 4, lp, 4, yp, 64, C.byref(k), 7, None) == LDSP_EINVAL              # mem
    assert ex(q, xp, 64, 64, sp, 4, lp, 4, None, 0, C.byref(k), 7, None) == LDSP_EINVAL
    # the object is untouched: the stream position, the thresholds and the state of a fresh one
    rc, f = create(lib, 3, 16)
    assert info(lib, q) == info(lib, f) == (3, 16, 0.25, 4, 0)
    assert lib.ldsp_sqbank_get_info(q, None, None, None, None, None) == 0
    assert (thresholds(lib, q, 3)[0] == thresholds(lib, f, 3)[0]).all()
    mode, timer, s = np.zeros(3, np.int32), np.ones(3, np.uint32), np.ones(3)
    assert lib.ldsp_sqbank_get_state(q, mode.ctypes.data, timer.ctypes.data, s.ctypes.data) == 0
    assert (mode == 1).all() and (timer == 0).all() and (s == 0).all()
    assert lib.ldsp_sqbank_get_state(q, None, None, None) == 0
    assert lib.ldsp_sqbank_get_state(None, None, None, None) == LDSP_EINVAL
    assert lib.ldsp_sqbank_num_outputs(q, 64, C.byref(k)) == 0 and k.value == 4
    assert lib.ldsp_sqbank_num_outputs(q, 64, None) == LDSP_EINVAL
    assert lib.ldsp_sqbank_num_outputs(None, 64, C.byref(k)) == LDSP_EINVAL
    assert lib.ldsp_sqbank_get_info(None, None, None, None, None, None) == LDSP_EINVAL
    assert lib.ldsp_sqbank_reset(None) == LDSP_EINVAL
    assert lib.ldsp_sqbank_reset(q) == 0
    assert lib.ldsp_sqbank_destroy(q) == 0 and lib.ldsp_sqbank_destroy(f) == 0
    assert lib.ldsp_sqbank_destroy(None) == 0


def test_python_shape_errors_need_no_gpu(ld):
    sq = ld.SquelchBank(3, 16)
    for bad in (np.zeros((2, 64), np.complex64), np.zeros((4, 64), np.complex64), np.zeros(64, np.complex64),
                np.zeros((3, 4, 4), np.complex64)):
        with pytest.raises(ValueError):
            sq(bad)
        with pytest.raises(ValueError):
            sq.measure(bad)
    assert sq.fill == 0 and sq.status is None


def test_call_raises_without_gpu(ld):
    if ld.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ld.SquelchBank(2, 16)(np.zeros((2, 64), np.complex64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ld.SquelchBank(2, 16).measure(np.zeros((2, 64), np.complex64))


# ---------------------------------------------------------------- the tile hook
def test_tile_hook(lib, ld):
    t = C.c_size_t()
    for B in (16, 100, 4096):
        assert lib.ldsp_debug_sqbank_tile(B, C.byref(t)) == 0
        assert t.value > 0, B
        assert ld.SquelchBank(1, B).tile == t.value
    assert lib.ldsp_debug_sqbank_tile(15, C.byref(t)) == LDSP_EINVAL
    assert lib.ldsp_debug_sqbank_tile(4097, C.byref(t)) == LDSP_EINVAL
    assert lib.ldsp_debug_sqbank_tile(64, None) == LDSP_EINVAL
