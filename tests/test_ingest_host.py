"""Host side of the int16 IQ ingest without a GPU (CPU suite):
ldsp_chan_execute_iq16, ldsp_ddc_execute_iq16 and ldsp_spgram_execute_iq16 are
exported, decide their argument errors on the host before any device work as
their _execute siblings do, take n = 0, and fail loudly (LDSP_EHIP) where there
is no GPU; Channelizer.from_bytes, Downconverter.from_bytes,
Spectrogram.from_bytes and Spectrogram.write_bytes exist and raise likewise.
The GPU side is tests/test_gpu_ingest.py."""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIBPATH = os.path.join(REPO, "python-liquiddsp_amd", "libldsp.so")

LDSP_EINVAL, LDSP_EHIP, LDSP_ERANGE = -1, -3, -4
MEM_HOST = 0
ENTRIES = ["ldsp_chan_execute_iq16", "ldsp_ddc_execute_iq16", "ldsp_spgram_execute_iq16"]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIBPATH):
        pytest.fail("libldsp.so not built (run __graft_entry__.build())")
    L = C.CDLL(LIBPATH)
    L.ldsp_last_error.restype = C.c_char_p
    vp, u, f, sz = C.c_void_p, C.c_uint, C.c_float, C.c_size_t
    L.ldsp_chan_create.argtypes = [u, u, u, f, f, C.POINTER(vp)]
    L.ldsp_ddc_create.argtypes = [C.POINTER(C.c_double), u, u, u, f, f, C.POINTER(vp)]
    L.ldsp_spgram_create.argtypes = [u, C.c_int, u, u, u, C.POINTER(vp)]
    for name in ("chan", "ddc", "spgram"):
        getattr(L, "ldsp_%s_destroy" % name).argtypes = [vp]
    L.ldsp_chan_get_info.argtypes = [vp, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)]
    L.ldsp_ddc_get_info.argtypes = [vp, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)]
    L.ldsp_spgram_get_info.argtypes = [vp, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u),
                                       C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]
    return L


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def make(lib, entry):
    """A small object for `entry`: (handle, destroy, rows of its output, columns for 64 samples)."""
    q = C.c_void_p()
    if "chan" in entry:                              # 8 channels, 2x oversampled: 16 columns of 64 samples
        assert lib.ldsp_chan_create(8, 4, 6, 0.0, 60.0, C.byref(q)) == 0
        return q, lib.ldsp_chan_destroy, 8, 16
    if "ddc" in entry:                               # 2 tuners, decimation 4: 16 columns
        f = (C.c_double * 2)(0.1, -0.2)
        assert lib.ldsp_ddc_create(f, 2, 4, 6, 0.0, 60.0, C.byref(q)) == 0
        return q, lib.ldsp_ddc_destroy, 2, 16
    assert lib.ldsp_spgram_create(256, 1, 32, 16, 1, C.byref(q)) == 0    # hann, W = 32, hop 16: 4 rows of 256
    return q, lib.ldsp_spgram_destroy, 4, 256


def execute(lib, entry):
    fn = getattr(lib, entry)
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.c_int,
                   C.c_void_p]
    return fn


def consumed(lib, entry, q):
    if "spgram" in entry:
        t = C.c_uint64(99)
        assert lib.ldsp_spgram_get_info(q, None, None, None, None, C.byref(t), None) == 0
        return t.value
    sk = C.c_uint(99)
    get = lib.ldsp_chan_get_info if "chan" in entry else lib.ldsp_ddc_get_info
    assert get(q, None, None, None, C.byref(sk)) == 0
    return sk.value


def gpus(lib):
    n = C.c_int()
    assert lib.ldsp_device_count(C.byref(n)) == 0
    return n.value


def test_symbols_are_exported(lib):
    missing = [s for s in ENTRIES if not hasattr(lib, s)]
    assert not missing, missing
    with open(os.path.join(REPO, "include", "ldsp.h")) as f:
        header = f.read()
    for s in ENTRIES:
        assert s + "(" in header, s


@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_errors_need_no_gpu(lib, entry):
    """A `mem` that is neither host nor device, a NULL x with n > 0 and a NULL
    object are LDSP_EINVAL; a row stride below the column count is the sibling's
    error (LDSP_ERANGE with *ncols set; ldsp_spgram: LDSP_EINVAL).  All are
    decided on the host, with and without a GPU, and consume nothing."""
    q, destroy, rows, cols = make(lib, entry)
    ex = execute(lib, entry)
    raw = np.zeros(2 * 64, np.int16)                 # 64 (I, Q) pairs
    y = np.zeros(rows * cols * 2, np.float32)
    xp, yp = raw.ctypes.data, y.ctypes.data
    k = C.c_size_t(0)
    ld_ok = cols
    assert ex(q, xp, 64, yp, ld_ok, C.byref(k), 7, None) == LDSP_EINVAL
    assert b"mem" in lib.ldsp_last_error()
    assert ex(q, None, 64, yp, ld_ok, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert ex(None, xp, 64, yp, ld_ok, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    if "spgram" in entry:
        assert ex(q, xp, 64, yp, cols - 1, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
        assert k.value == 4                          # n counts pairs: 64 samples at hop 16
    else:
        assert ex(q, xp, 64, yp, cols - 1, C.byref(k), MEM_HOST, None) == LDSP_ERANGE
        assert k.value == cols                       # n counts pairs: 64 samples at decimation 4
        assert ex(q, xp, 64, None, ld_ok, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert consumed(lib, entry, q) == 0
    assert destroy(q) == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_n_zero_is_legal(lib, entry):
    """n = 0 with NULL buffers is no argument error: the call reports no output and succeeds
    (without a GPU it is LDSP_EHIP, as the sibling's)."""
    q, destroy, rows, cols = make(lib, entry)
    k = C.c_size_t(99)
    rc = execute(lib, entry)(q, None, 0, None, 0, C.byref(k), MEM_HOST, None)
    assert rc == (0 if gpus(lib) > 0 else LDSP_EHIP), lib.ldsp_last_error()
    assert k.value == 0
    assert consumed(lib, entry, q) == 0
    assert destroy(q) == 0


@pytest.mark.parametrize("entry", ENTRIES)
def test_execute_without_gpu_fails_loudly(lib, entry):
    if gpus(lib) > 0:
        pytest.skip("a GPU is present")
    q, destroy, rows, cols = make(lib, entry)
    raw = np.zeros(2 * 64, np.int16)
    y = np.zeros(rows * cols * 2, np.float32)
    k = C.c_size_t(0)
    assert execute(lib, entry)(q, raw.ctypes.data, 64, y.ctypes.data, cols, C.byref(k), MEM_HOST, None) == LDSP_EHIP
    assert b"no CPU fallback" in lib.ldsp_last_error()
    assert destroy(q) == 0


def objects(ld):
    return [(ld.Channelizer(8), "from_bytes"), (ld.Downconverter([0.1, -0.2], 4), "from_bytes"),
            (ld.Spectrogram(256, window_len=32, delay=16), "from_bytes"),
            (ld.Spectrogram(256, window_len=32, delay=16), "write_bytes")]


def test_python_methods_exist(ld):
    for obj, name in objects(ld):
        assert callable(getattr(obj, name)), (type(obj).__name__, name)


def test_python_methods_raise_without_gpu(ld):
    if ld.device_count() > 0:
        pytest.skip("a GPU is present")
    raw = np.zeros(2 * 64, np.int16)
    for obj, name in objects(ld):
        for arg in (raw, raw.tobytes(), raw.view(np.uint8), bytearray(raw.tobytes()) + b"\x01"):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                getattr(obj, name)(arg)
