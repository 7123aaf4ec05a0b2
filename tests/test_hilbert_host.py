"""Host side of SSBDemod / HilbertTransform without a GPU (CPU suite): the
firhilbf taps behind the C ABI are bit-identical to the restatement, the
argument errors of ldsp_firhilb_create / _execute come back before any device
work, and the two Python classes construct and dispatch on dtype like Delay.
(reference src/demod.hpp:155-187, src/utility.hpp:71-108)"""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIBPATH = os.path.join(REPO, "python-liquiddsp_amd", "libldsp.so")

LDSP_EINVAL, LDSP_EUNSUP = -1, -5
R2C, C2R, DECIM, INTERP = 0, 1, 2, 3
MEM_HOST = 0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIBPATH):
        pytest.fail("libldsp.so not built (run __graft_entry__.build())")
    L = C.CDLL(LIBPATH)
    L.ldsp_last_error.restype = C.c_char_p
    L.ldsp_firhilb_create.argtypes = [C.c_uint, C.c_float, C.c_int, C.POINTER(C.c_void_p)]
    L.ldsp_firhilb_destroy.argtypes = [C.c_void_p]
    L.ldsp_firhilb_get_taps.argtypes = [C.c_void_p, C.c_void_p]
    L.ldsp_firhilb_execute.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int,
                                       C.c_void_p]
    return L


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def make(lib, m, As, op):
    q = C.c_void_p()
    rc = lib.ldsp_firhilb_create(m, As, op, C.byref(q))
    return rc, q


@pytest.mark.parametrize("m", [2, 5, 25, 64])
@pytest.mark.parametrize("As", [40.0, 60.0])
def test_taps_bitwise(lib, ora, m, As):
    rc, q = make(lib, m, As, C2R)
    assert rc == 0, lib.ldsp_last_error()
    h = np.full(2 * m, np.nan, np.float32)
    assert lib.ldsp_firhilb_get_taps(q, h.ctypes.data) == 0
    ref = ora.FirHilb(m, As).taps()
    assert (h.view(np.uint32) == ref.view(np.uint32)).all()
    assert lib.ldsp_firhilb_destroy(q) == 0


def test_create_errors(lib):
    for m in (0, 1):
        rc, _ = make(lib, m, 60.0, C2R)
        assert rc == LDSP_EINVAL
    for op in (-1, 4):
        rc, _ = make(lib, 5, 60.0, op)
        assert rc == LDSP_EINVAL
    rc, _ = make(lib, 65, 60.0, R2C)
    assert rc == LDSP_EUNSUP
    rc, q = make(lib, 64, 60.0, INTERP)
    assert rc == 0
    lib.ldsp_firhilb_destroy(q)
    assert lib.ldsp_firhilb_create(5, 60.0, C2R, None) == LDSP_EINVAL


def test_execute_argument_errors_need_no_gpu(lib):
    # checked on the host before any device work: the codes are the same with and without a GPU
    x = np.zeros(16, np.complex64)
    y = np.zeros(32, np.complex64)
    xp, yp = x.ctypes.data, y.ctypes.data
    rc, q = make(lib, 5, 60.0, DECIM)
    assert lib.ldsp_firhilb_execute(q, xp, 7, yp, None, MEM_HOST, None) == LDSP_EINVAL      # odd n
    assert b"even" in lib.ldsp_last_error()
    assert lib.ldsp_firhilb_execute(q, xp, 8, yp, yp, MEM_HOST, None) == LDSP_EINVAL        # y1 on a non-c2r object
    lib.ldsp_firhilb_destroy(q)
    for op in (R2C, INTERP):
        rc, q = make(lib, 5, 60.0, op)
        assert lib.ldsp_firhilb_execute(q, xp, 8, yp, yp, MEM_HOST, None) == LDSP_EINVAL
        assert lib.ldsp_firhilb_execute(q, xp, 8, None, None, MEM_HOST, None) == LDSP_EINVAL
        lib.ldsp_firhilb_destroy(q)
    rc, q = make(lib, 25, 60.0, C2R)
    assert lib.ldsp_firhilb_execute(q, xp, 8, None, None, MEM_HOST, None) == LDSP_EINVAL    # neither sideband
    assert lib.ldsp_firhilb_execute(q, None, 8, yp, None, MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_firhilb_execute(None, xp, 8, yp, None, MEM_HOST, None) == LDSP_EINVAL
    lib.ldsp_firhilb_destroy(q)


def test_tile_hook(lib, ld):
    t = C.c_size_t()
    for op in (R2C, C2R, DECIM, INTERP):
        assert lib.ldsp_debug_firhilb_tile(op, C.byref(t)) == 0
        assert t.value == ld._hilbert_tile(op) and t.value >= 256
    assert lib.ldsp_debug_firhilb_tile(4, C.byref(t)) == LDSP_EINVAL


def test_classes_construct(ld):
    for band in ("usb", "lsb", "anything else is the lower sideband"):
        s = ld.SSBDemod(band)
        s.reset()                                  # before the first call: nothing on the device yet
    h = ld.HilbertTransform()
    h.reset()
    ld.HilbertTransform(m=25, As=40.0)
    ld.HilbertTransform(2)
    with pytest.raises(ValueError):
        ld.HilbertTransform(m=1)
    with pytest.raises(NotImplementedError):
        ld.HilbertTransform(m=65)
    with pytest.raises(TypeError):
        ld.SSBDemod()


def test_call_returns_none_for_other_dtypes(ld):
    h = ld.HilbertTransform()
    assert h(np.zeros(4, np.float64)) is None       # as Delay does for a dtype it does not take
    assert h(np.zeros(4, np.int16)) is None
    assert ld.Delay(1)(np.zeros(4, np.float64)) is None


def test_decim_odd_length_is_a_value_error(ld):
    # rejected on the host, so it raises ValueError even where no GPU is present
    h = ld.HilbertTransform()
    with pytest.raises(ValueError):
        h.decim(np.zeros(5, np.float32))
    with pytest.raises(ValueError):
        h(np.zeros(5, np.float32))
