"""Host side of the Downconverter without a GPU (CPU suite): construction and
defaults, the frequency words (w = rint(f 2^32) mod 2^32, ties to even) and
their round trip, the default prototype (bit-identical to the restatement's
firdes_kaiser) and its scale, user taps, num_outputs / skip against the closed
form, every argument error of ldsp_ddc_create* / _set_frequencies / _execute
(decided before any device work), retuning with a changed tuner count, the tile
hook over both tile classes, and the stand-alone C driver under ASan + UBSan.
The GPU side is tests/test_gpu_downconverter.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "python-liquiddsp_amd")
LIBPATH = os.path.join(PKG, "libldsp.so")

LDSP_EINVAL, LDSP_EHIP, LDSP_ERANGE, LDSP_EUNSUP = -1, -3, -4, -5
MEM_HOST = 0
FREQS = [0.0, 0.5, -0.5, 2.0 ** -32, -2.0 ** -33, 1.0, 0.0371, -0.31337, 2.0 ** -33, 3 * 2.0 ** -33]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIBPATH):
        pytest.fail("libldsp.so not built (run __graft_entry__.build())")
    L = C.CDLL(LIBPATH)
    L.ldsp_last_error.restype = C.c_char_p
    vp, u, f, sz = C.c_void_p, C.c_uint, C.c_float, C.c_size_t
    L.ldsp_ddc_create.argtypes = [vp, u, u, u, f, f, C.POINTER(vp)]
    L.ldsp_ddc_create_taps.argtypes = [vp, u, u, vp, u, C.POINTER(vp)]
    L.ldsp_ddc_destroy.argtypes = [vp]
    L.ldsp_ddc_reset.argtypes = [vp]
    L.ldsp_ddc_set_frequencies.argtypes = [vp, vp, u]
    L.ldsp_ddc_get_words.argtypes = [vp, vp]
    L.ldsp_ddc_get_info.argtypes = [vp, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)]
    L.ldsp_ddc_get_taps.argtypes = [vp, vp]
    L.ldsp_ddc_get_scale.argtypes = [vp, C.POINTER(f)]
    L.ldsp_ddc_set_scale.argtypes = [vp, f]
    L.ldsp_ddc_num_outputs.argtypes = [vp, sz, C.POINTER(sz)]
    L.ldsp_ddc_execute.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    L.ldsp_debug_ddc_tile.argtypes = [u, u, C.POINTER(sz)]
    L.ldsp_debug_ddc_seek.argtypes = [vp, C.c_uint64]
    return L


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def fvec(f):
    return np.atleast_1d(np.asarray(f, np.float64))


def create(lib, f, D, m=6, fc=0.0, As=60.0, C_=None):
    a = fvec(f)
    q = C.c_void_p()
    return lib.ldsp_ddc_create(a.ctypes.data, a.size if C_ is None else C_, D, m, fc, As, C.byref(q)), q


def create_taps(lib, f, D, h, L=None, C_=None):
    a, h = fvec(f), np.asarray(h, np.float32)
    q = C.c_void_p()
    return lib.ldsp_ddc_create_taps(a.ctypes.data, a.size if C_ is None else C_, D, h.ctypes.data,
                                    h.size if L is None else L, C.byref(q)), q


def info(lib, q):
    c, d, l, s = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
    assert lib.ldsp_ddc_get_info(q, C.byref(c), C.byref(d), C.byref(l), C.byref(s)) == 0
    return c.value, d.value, l.value, s.value


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def words_of(f):
    return (np.rint(fvec(f) * 2.0 ** 32).astype(np.int64) % 2 ** 32).astype(np.uint32)


# ---------------------------------------------------------------- construction
@pytest.mark.parametrize("D", [2, 5, 64, 100, 256])
def test_constructs(ld, D):
    dc = ld.Downconverter([0.1, -0.2, 0.3], D)
    assert (dc.ntuners, dc.decim, dc.skip) == (3, D, 0)
    assert len(dc.taps) == 2 * D * 6 + 1
    dc.reset()                                       # before the first call: nothing on the device yet
    one = ld.Downconverter(0.25, D)                  # a float is one tuner
    assert one.ntuners == 1 and one.words.tolist() == [1 << 30]
    assert ld.Downconverter(np.float32(-0.25), D).words.tolist() == [3 << 30]
    assert ld.Downconverter(freqs=(0.1,), decim=D, m=2, Fc=0.4 / D, As=40.0, taps=None).ntuners == 1
    assert ld.Downconverter(np.linspace(-0.5, 0.49, 64), D).ntuners == 64


# ---------------------------------------------------------------- words
def test_words(ld, lib):
    dc = ld.Downconverter(FREQS, 8)
    want = [0, 1 << 31, 1 << 31, 1, 0, 0, int(np.rint(0.0371 * 2.0 ** 32)),
            int(np.rint(-0.31337 * 2.0 ** 32)) % 2 ** 32, 0, 2]
    assert dc.words.dtype == np.uint32 and dc.words.tolist() == want
    assert np.array_equal(dc.words, words_of(FREQS))
    # the frequencies come back as w / 2^32 wrapped into [-0.5, 0.5)
    fr = dc.freqs
    assert fr.dtype == np.float64
    assert np.array_equal(fr, ((dc.words.astype(np.float64) / 2.0 ** 32 + 0.5) % 1.0) - 0.5)
    assert fr[1] == -0.5 and fr[2] == -0.5 and fr[5] == 0.0 and fr[3] == 2.0 ** -32
    assert abs(fr[6] - 0.0371) <= 2.0 ** -33 and abs(fr[7] + 0.31337) <= 2.0 ** -33
    # a round trip leaves the words as they are
    dc.freqs = fr
    assert dc.words.tolist() == want
    # the same through the C ABI
    rc, q = create(lib, FREQS, 8)
    assert rc == 0, lib.ldsp_last_error()
    w = np.full(len(FREQS), 77, np.uint32)
    assert lib.ldsp_ddc_get_words(q, w.ctypes.data) == 0 and w.tolist() == want
    assert lib.ldsp_ddc_destroy(q) == 0
    seeded = np.random.default_rng(11).uniform(-1.0, 1.0, 64)
    assert np.array_equal(ld.Downconverter(seeded, 4).words, words_of(seeded))


# ---------------------------------------------------------------- design
@pytest.mark.parametrize("D,m,As", [(2, 4, 60.0), (5, 6, 60.0), (64, 6, 60.0), (100, 1, 40.0), (256, 8, 80.0)])
def test_default_prototype_bitwise(ld, lib, ora, D, m, As):
    dc = ld.Downconverter([0.1, 0.2], D, m=m, As=As)
    ref = ora.firdes_kaiser(2 * D * m + 1, 0.5 / D, As, 0)
    assert dc.taps.dtype == np.float32 and dc.taps.shape == ref.shape
    assert (bits(dc.taps) == bits(ref)).all()
    assert np.float32(dc.scale) == np.float32(1.0 / np.sum(dc.taps.astype(np.float64)))
    rc, q = create(lib, [0.1, 0.2], D, m, 0.0, As)
    assert rc == 0, lib.ldsp_last_error()
    assert info(lib, q) == (2, D, 2 * D * m + 1, 0)
    assert lib.ldsp_ddc_get_info(q, None, None, None, None) == 0
    h = np.full(2 * D * m + 1, np.nan, np.float32)
    assert lib.ldsp_ddc_get_taps(q, h.ctypes.data) == 0
    assert (bits(h) == bits(ref)).all()
    s = C.c_float()
    assert lib.ldsp_ddc_get_scale(q, C.byref(s)) == 0 and np.float32(s.value) == np.float32(dc.scale)
    assert lib.ldsp_ddc_destroy(q) == 0


def test_cutoff_override(ld, ora):
    dc = ld.Downconverter(0.1, 16, m=4, Fc=0.05)
    assert (bits(dc.taps) == bits(ora.firdes_kaiser(2 * 16 * 4 + 1, 0.05, 60.0, 0))).all()
    assert np.float32(dc.scale) == np.float32(1.0 / np.sum(dc.taps.astype(np.float64)))


def test_user_taps(ld):
    h = np.random.default_rng(5).standard_normal(37).astype(np.float32)
    dc = ld.Downconverter([0.1, 0.2], 4, taps=h)
    assert (bits(dc.taps) == bits(h)).all() and dc.scale == 1.0
    dc.scale = 0.25
    assert dc.scale == 0.25
    assert len(ld.Downconverter(0.1, 8, taps=[1.0]).taps) == 1
    ld.Downconverter(0.1, 4, taps=np.ones(17 * 4, np.float32))       # 17 taps per output phase: the most supported
    ld.Downconverter(0.1, 256, taps=np.ones(17 * 256, np.float32))


# ---------------------------------------------------------------- the column schedule
@pytest.mark.parametrize("D", [2, 5, 64, 100, 256])
def test_num_outputs_and_skip(lib, D):
    rc, q = create(lib, 0.1, D)
    assert rc == 0
    rng = np.random.default_rng(100 + D)
    n = C.c_size_t(12345)
    for T in [0, 1, D - 1, D, D + 1, 2 ** 32 - 1, 2 ** 32, 2 ** 40 + 7] + [int(v) for v in rng.integers(0, 1 << 45, 8)]:
        assert lib.ldsp_debug_ddc_seek(q, T) == 0
        skip = (-T) % D
        assert info(lib, q)[3] == skip
        for c in [0, D, 1, D - 1, D + 1] + [int(v) for v in rng.integers(0, 5 * D, 8)]:
            assert lib.ldsp_ddc_num_outputs(q, c, C.byref(n)) == 0
            assert n.value == (-(-(c - skip) // D) if c > skip else 0), (T, c)
    assert lib.ldsp_ddc_reset(q) == 0 and info(lib, q)[3] == 0
    assert lib.ldsp_ddc_destroy(q) == 0


def test_num_outputs_python(ld):
    dc = ld.Downconverter(0.1, 8)
    assert [dc.num_outputs(n) for n in (0, 1, 8, 9, 43)] == [0, 1, 1, 2, 6]
    dc._seek(5)
    assert dc.skip == 3 and [dc.num_outputs(n) for n in (0, 3, 4, 11, 12)] == [0, 0, 1, 1, 2]
    dc.reset()
    assert dc.skip == 0


# ---------------------------------------------------------------- errors
def test_constructor_errors(ld):
    for D in (0, -3):
        with pytest.raises(ValueError):
            ld.Downconverter(0.1, D)
    for D in (1, 257, 1000):
        with pytest.raises(NotImplementedError):
            ld.Downconverter(0.1, D)
    with pytest.raises(ValueError):
        ld.Downconverter([], 8)
    with pytest.raises(NotImplementedError):
        ld.Downconverter(np.zeros(65), 8)
    for m in (0, -1):
        with pytest.raises(ValueError):
            ld.Downconverter(0.1, 8, m=m)
    with pytest.raises(NotImplementedError):
        ld.Downconverter(0.1, 8, m=9)
    for As in (0.0, -60.0):
        with pytest.raises(ValueError):
            ld.Downconverter(0.1, 8, As=As)
    for Fc in (0.5, 0.75):
        with pytest.raises(ValueError):
            ld.Downconverter(0.1, 8, Fc=Fc)
    for f in (np.nan, np.inf, -np.inf, 1.0000001, -1.5):
        with pytest.raises(ValueError):
            ld.Downconverter([0.1, f], 8)
    with pytest.raises(ValueError):
        ld.Downconverter(0.1, 8, taps=[])
    with pytest.raises(NotImplementedError):
        ld.Downconverter(0.1, 4, taps=np.ones(17 * 4 + 1, np.float32))
    ld.Downconverter([1.0, -1.0], 8)                 # the ends of the range are allowed


def test_create_codes(lib):
    assert create(lib, 0.1, 0)[0] == LDSP_EINVAL
    assert create(lib, 0.1, 1)[0] == LDSP_EUNSUP
    assert create(lib, 0.1, 257)[0] == LDSP_EUNSUP
    assert create(lib, 0.1, 8, C_=0)[0] == LDSP_EINVAL
    assert create(lib, np.zeros(65), 8)[0] == LDSP_EUNSUP
    assert create(lib, 0.1, 8, m=0)[0] == LDSP_EINVAL
    assert create(lib, 0.1, 8, m=9)[0] == LDSP_EUNSUP
    assert create(lib, 0.1, 8, As=0.0)[0] == LDSP_EINVAL
    assert create(lib, 0.1, 8, As=-1.0)[0] == LDSP_EINVAL
    assert create(lib, 0.1, 8, fc=0.5)[0] == LDSP_EINVAL
    for f in (np.nan, np.inf, 1.0000001, -1.5):
        assert create(lib, [0.1, f], 8)[0] == LDSP_EINVAL
    q = C.c_void_p()
    assert lib.ldsp_ddc_create(None, 1, 8, 6, 0.0, 60.0, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_ddc_create(fvec(0.1).ctypes.data, 1, 8, 6, 0.0, 60.0, None) == LDSP_EINVAL
    h = np.ones(8, np.float32)
    assert create_taps(lib, 0.1, 8, h, L=0)[0] == LDSP_EINVAL
    assert create_taps(lib, 0.1, 0, h)[0] == LDSP_EINVAL
    assert create_taps(lib, 0.1, 1, h)[0] == LDSP_EUNSUP
    assert create_taps(lib, 0.1, 257, h)[0] == LDSP_EUNSUP
    assert create_taps(lib, 0.1, 8, h, C_=0)[0] == LDSP_EINVAL
    assert create_taps(lib, np.zeros(65), 8, h)[0] == LDSP_EUNSUP
    assert create_taps(lib, [np.nan], 8, h)[0] == LDSP_EINVAL
    f = fvec(0.1)
    assert lib.ldsp_ddc_create_taps(f.ctypes.data, 1, 8, None, 8, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_ddc_create_taps(None, 1, 8, h.ctypes.data, 8, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_ddc_create_taps(f.ctypes.data, 1, 8, h.ctypes.data, 8, None) == LDSP_EINVAL
    big = np.ones(17 * 8 + 1, np.float32)
    assert create_taps(lib, 0.1, 8, big)[0] == LDSP_EUNSUP
    rc, q = create_taps(lib, 0.1, 8, big, L=big.size - 1)
    assert rc == 0 and lib.ldsp_ddc_destroy(q) == 0


def test_execute_argument_errors_need_no_gpu(lib):
    rc, q = create(lib, [0.1, 0.2, 0.3], 4)
    assert rc == 0
    x = np.zeros(64, np.complex64)
    y = np.zeros((3, 20), np.complex64)
    xp, yp = x.ctypes.data, y.ctypes.data
    k = C.c_size_t(0)
    assert lib.ldsp_ddc_execute(q, xp, 64, yp, 15, C.byref(k), MEM_HOST, None) == LDSP_ERANGE
    assert k.value == 16
    assert lib.ldsp_ddc_execute(q, xp, 64, yp, 15, None, MEM_HOST, None) == LDSP_ERANGE
    assert lib.ldsp_ddc_execute(None, xp, 64, yp, 16, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_ddc_execute(q, None, 64, yp, 16, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_ddc_execute(q, xp, 64, None, 16, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_ddc_execute(q, xp, 64, yp, 16, C.byref(k), 7, None) == LDSP_EINVAL
    # the object is untouched: the same taps, scale, words and counts as a fresh one
    rc, f = create(lib, [0.1, 0.2, 0.3], 4)
    a, b = np.zeros(49, np.float32), np.ones(49, np.float32)
    assert lib.ldsp_ddc_get_taps(q, a.ctypes.data) == 0 and lib.ldsp_ddc_get_taps(f, b.ctypes.data) == 0
    assert (bits(a) == bits(b)).all()
    sa, sb = C.c_float(), C.c_float(1.0)
    assert lib.ldsp_ddc_get_scale(q, C.byref(sa)) == 0 and lib.ldsp_ddc_get_scale(f, C.byref(sb)) == 0
    assert sa.value == sb.value
    wa, wb = np.zeros(3, np.uint32), np.ones(3, np.uint32)
    assert lib.ldsp_ddc_get_words(q, wa.ctypes.data) == 0 and lib.ldsp_ddc_get_words(f, wb.ctypes.data) == 0
    assert np.array_equal(wa, wb)
    assert info(lib, q) == info(lib, f) == (3, 4, 49, 0)
    assert lib.ldsp_ddc_num_outputs(q, 64, C.byref(k)) == 0 and k.value == 16
    assert lib.ldsp_ddc_num_outputs(q, 64, None) == LDSP_EINVAL
    assert lib.ldsp_ddc_num_outputs(None, 64, C.byref(k)) == LDSP_EINVAL
    assert lib.ldsp_ddc_get_taps(q, None) == LDSP_EINVAL
    assert lib.ldsp_ddc_get_words(q, None) == LDSP_EINVAL
    assert lib.ldsp_ddc_get_scale(q, None) == LDSP_EINVAL
    assert lib.ldsp_ddc_reset(None) == LDSP_EINVAL
    assert lib.ldsp_debug_ddc_seek(None, 0) == LDSP_EINVAL
    assert lib.ldsp_ddc_destroy(q) == 0 and lib.ldsp_ddc_destroy(f) == 0


# ---------------------------------------------------------------- retuning
def test_set_frequencies_changes_the_tuner_count(ld, lib):
    rc, q = create(lib, [0.1, 0.2, 0.3], 8)
    assert rc == 0
    five = fvec([0.0, 0.5, -0.25, 0.0371, 2.0 ** -32])
    assert lib.ldsp_ddc_set_frequencies(q, five.ctypes.data, 5) == 0
    assert info(lib, q)[0] == 5
    w = np.zeros(5, np.uint32)
    assert lib.ldsp_ddc_get_words(q, w.ctypes.data) == 0 and np.array_equal(w, words_of(five))
    assert lib.ldsp_ddc_set_frequencies(q, five.ctypes.data, 1) == 0 and info(lib, q)[0] == 1
    # a rejected list leaves the old one
    assert lib.ldsp_ddc_set_frequencies(q, five.ctypes.data, 0) == LDSP_EINVAL
    assert lib.ldsp_ddc_set_frequencies(q, np.zeros(65).ctypes.data, 65) == LDSP_EUNSUP
    assert lib.ldsp_ddc_set_frequencies(q, fvec([0.1, np.nan]).ctypes.data, 2) == LDSP_EINVAL
    assert lib.ldsp_ddc_set_frequencies(q, None, 2) == LDSP_EINVAL
    assert lib.ldsp_ddc_set_frequencies(None, five.ctypes.data, 2) == LDSP_EINVAL
    assert info(lib, q) == (1, 8, 97, 0)
    assert lib.ldsp_ddc_destroy(q) == 0
    dc = ld.Downconverter([0.1, 0.2, 0.3], 8)
    dc.freqs = five
    assert dc.ntuners == 5 and np.array_equal(dc.words, words_of(five))
    dc.freqs = 0.25
    assert dc.ntuners == 1 and dc.words.tolist() == [1 << 30]
    for bad in ([], np.zeros(65), [2.0]):
        with pytest.raises((ValueError, NotImplementedError)):
            dc.freqs = bad
    assert dc.ntuners == 1 and dc.words.tolist() == [1 << 30]


# ---------------------------------------------------------------- no GPU
def test_call_raises_without_gpu(ld):
    if ld.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ld.Downconverter(0.1, 4)(np.zeros(64, np.complex64))


# ---------------------------------------------------------------- the tile hook
# both classes the kernel distinguishes: 64 columns per workgroup, or 32 where the span of 64 does not fit the LDS
TILES = [(2, 1, 64), (2, 25, 64), (5, 61, 64), (8, 3, 64), (64, 769, 64), (64, 17 * 64, 64), (100, 1201, 64),
         (128, 1537, 64), (220, 17 * 220, 64), (232, 17 * 232, 32), (256, 3073, 32), (256, 4097, 32),
         (256, 17 * 256, 32), (256, 1, 64), (256, 1025, 64)]


def test_tile_hook(lib, ld):
    f = C.c_size_t()
    for D, L, want in TILES:
        assert lib.ldsp_debug_ddc_tile(D, L, C.byref(f)) == 0
        assert f.value == want, (D, L)
        assert ld.Downconverter(0.1, D, taps=np.ones(L, np.float32)).tile == want
    assert ld.Downconverter(0.1, 256, m=8).tile == 32 and ld.Downconverter(0.1, 64).tile == 64
    assert lib.ldsp_debug_ddc_tile(0, 8, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_ddc_tile(8, 0, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_ddc_tile(1, 8, C.byref(f)) == LDSP_EUNSUP
    assert lib.ldsp_debug_ddc_tile(257, 8, C.byref(f)) == LDSP_EUNSUP
    assert lib.ldsp_debug_ddc_tile(8, 17 * 8 + 1, C.byref(f)) == LDSP_EUNSUP
    assert lib.ldsp_debug_ddc_tile(8, 8, None) == LDSP_EINVAL


# ---------------------------------------------------------------- the C driver under ASan + UBSan
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:")


def test_ddc_driver_asan_ubsan():
    r = subprocess.run(["make", "-s", "-j8", "-C", PKG, "ddc_asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(PKG, "build", "ddc_driver_asan")
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the driver is not instrumented"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert not any(k in out for k in REPORTS), out[-4000:]
    assert "all checks passed" in r.stdout
