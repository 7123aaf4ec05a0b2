"""Host side of the AMBank without a GPU (CPU suite): the exported
ldsp_ambank_* symbols, construction and defaults, the designed prototypes and
their difference d (bit-identical to the restatement's firdes_kaiser normalised
the same way), user taps, num_outputs / skip over ragged call lengths against
the closed form, every argument error of ldsp_ambank_create* / _execute
(decided before any device work), the Python shape and dtype errors, the tile
hook, and the stand-alone C driver of the same host code under ASan + UBSan
(tests/sanitize/ambank_driver.c).  The GPU side is tests/test_gpu_ambank.py."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "python-liquiddsp_amd")
LIBPATH = os.path.join(PKG, "libldsp.so")
HEADER = os.path.join(REPO, "include", "ldsp.h")

LDSP_EINVAL, LDSP_ERANGE, LDSP_EUNSUP = -1, -4, -5
MEM_HOST = 0
CARRIER = 0.016


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIBPATH):
        pytest.fail("libldsp.so not built (run __graft_entry__.build())")
    L = C.CDLL(LIBPATH)
    L.ldsp_last_error.restype = C.c_char_p
    vp, u, f, d, sz = C.c_void_p, C.c_uint, C.c_float, C.c_double, C.c_size_t
    L.ldsp_ambank_create.argtypes = [u, u, d, d, u, f, f, C.POINTER(vp)]
    L.ldsp_ambank_create_taps.argtypes = [u, u, vp, u, vp, u, f, C.POINTER(vp)]
    L.ldsp_ambank_destroy.argtypes = [vp]
    L.ldsp_ambank_reset.argtypes = [vp]
    L.ldsp_ambank_get_info.argtypes = [vp, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)]
    L.ldsp_ambank_get_taps.argtypes = [vp, vp, vp, vp]
    L.ldsp_ambank_get_threshold.argtypes = [vp, C.POINTER(f)]
    L.ldsp_ambank_set_threshold.argtypes = [vp, f]
    L.ldsp_ambank_num_outputs.argtypes = [vp, sz, C.POINTER(sz)]
    L.ldsp_ambank_execute.argtypes = [vp, vp, sz, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    L.ldsp_ambank_get_carrier_level.argtypes = [vp, vp]
    L.ldsp_debug_ambank_tile.argtypes = [u, u, C.POINTER(sz)]
    return L


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def create(lib, C_=3, D=5, audio=0.0, carrier=CARRIER, L=0, As=60.0, thr=0.0):
    q = C.c_void_p()
    return lib.ldsp_ambank_create(C_, D, audio, carrier, L, As, thr, C.byref(q)), q


def create_taps(lib, h, g, C_=3, D=5, thr=0.0, L=None, Lg=None):
    h, g = np.asarray(h, np.float32), np.asarray(g, np.float32)
    q = C.c_void_p()
    return lib.ldsp_ambank_create_taps(C_, D, h.ctypes.data, h.size if L is None else L, g.ctypes.data,
                                       g.size if Lg is None else Lg, thr, C.byref(q)), q


def info(lib, q):
    c, d, l, s = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
    assert lib.ldsp_ambank_get_info(q, C.byref(c), C.byref(d), C.byref(l), C.byref(s)) == 0
    return c.value, d.value, l.value, s.value


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def designed(ora, L, fc, As):
    """firdes_kaiser with every tap divided in double by the double sum of the float32 design."""
    h = ora.firdes_kaiser(L, np.float32(fc), As, 0)
    return (h.astype(np.float64) / np.sum(h.astype(np.float64))).astype(np.float32)


def band(h, g):
    """d = (float)((double)h - (double)g), rounded once."""
    return (np.asarray(h, np.float32).astype(np.float64) - np.asarray(g, np.float32).astype(np.float64)).astype(np.float32)


# ---------------------------------------------------------------- symbols
def test_library_exports_what_the_header_declares(lib):
    with open(HEADER) as f:
        names = sorted(set(re.findall(r"\b(ldsp_(?:debug_)?ambank_\w+)\s*\(", f.read())))
    want = {"ldsp_ambank_create", "ldsp_ambank_create_taps", "ldsp_ambank_destroy", "ldsp_ambank_reset",
            "ldsp_ambank_get_info", "ldsp_ambank_get_taps", "ldsp_ambank_get_threshold", "ldsp_ambank_set_threshold",
            "ldsp_ambank_num_outputs", "ldsp_ambank_execute", "ldsp_ambank_get_carrier_level", "ldsp_debug_ambank_tile"}
    assert want == set(names), sorted(want ^ set(names))
    for n in names:
        assert hasattr(lib, n), n


# ---------------------------------------------------------------- construction
def test_defaults(ld):
    am = ld.AMBank(16)
    assert (am.nchan, am.decim, am.skip, am.tile) == (16, 1, 0, 64)
    assert am.threshold == 0.0
    assert am.ntaps == len(am.taps) == len(am.carrier_taps) == 2 * math.ceil(2 / 0.004) + 1 == 1001
    assert am.taps.dtype == am.carrier_taps.dtype == am.band_taps.dtype == np.float32
    assert am.carrier_level.dtype == np.float32 and (am.carrier_level == 0).all() and am.carrier_level.shape == (16,)
    assert am.carrier_present.dtype == bool and not am.carrier_present.any()
    am.reset()                                       # before the first call: nothing on the device yet
    am.threshold = 0.25
    assert am.threshold == 0.25
    am.threshold = 0.0
    kw = ld.AMBank(nchan=256, decim=32, audio=0.01, carrier=0.005, ntaps=1025, As=40.0, threshold=0.02, taps=None,
                   carrier_taps=None)
    assert (kw.nchan, kw.decim, kw.ntaps, kw.threshold) == (256, 32, 1025, np.float32(0.02))
    assert ld.AMBank(1, ntaps=1).ntaps == 1
    assert ld.AMBank(2, 4, carrier=2.0 / 512).ntaps == 1025   # the lowest carrier cut-off with a default length


@pytest.mark.parametrize("D,audio", [(1, 0.45), (2, 0.25), (4, 0.125), (32, 0.5 / 32)])
def test_default_audio_cutoff(ld, ora, D, audio):
    am = ld.AMBank(2, D, ntaps=129)
    assert (bits(am.taps) == bits(designed(ora, 129, audio, 60.0))).all()
    assert (bits(am.taps) == bits(ld.AMBank(2, D, audio=audio, ntaps=129).taps)).all()


# ---------------------------------------------------------------- design
@pytest.mark.parametrize("D,audio,carrier,L,As", [(4, None, 0.004, None, 60.0), (5, 0.1, 0.016, None, 60.0),
                                                  (1, 0.3, 0.05, 33, 80.0), (8, 0.0625, 0.01, 1025, 40.0)])
def test_designed_prototypes_bitwise(ld, lib, ora, D, audio, carrier, L, As):
    am = ld.AMBank(2, D, audio=audio, carrier=carrier, ntaps=L, As=As)
    n = L or 2 * math.ceil(2 / carrier) + 1
    fa = audio or (0.45 if D == 1 else 0.5 / D)
    h, g = designed(ora, n, fa, As), designed(ora, n, carrier, As)
    d = band(h, g)
    assert am.ntaps == n
    assert am.taps.shape == h.shape and (bits(am.taps) == bits(h)).all()
    assert am.carrier_taps.shape == g.shape and (bits(am.carrier_taps) == bits(g)).all()
    assert am.band_taps.shape == d.shape and (bits(am.band_taps) == bits(d)).all()
    assert abs(np.sum(am.taps.astype(np.float64)) - 1) < 1e-6 and abs(np.sum(am.carrier_taps.astype(np.float64)) - 1) < 1e-6
    assert abs(np.sum(am.band_taps.astype(np.float64))) < 1e-6            # d has no DC gain: the carrier is taken out
    rc, q = create(lib, 2, D, audio or 0.0, carrier, L or 0, As)
    assert rc == 0, lib.ldsp_last_error()
    a, b, c = (np.full(n, np.nan, np.float32) for _ in range(3))
    assert lib.ldsp_ambank_get_taps(q, a.ctypes.data, b.ctypes.data, c.ctypes.data) == 0
    assert (bits(a) == bits(h)).all() and (bits(b) == bits(g)).all() and (bits(c) == bits(d)).all()
    assert lib.ldsp_ambank_get_taps(q, None, None, None) == 0
    assert lib.ldsp_ambank_destroy(q) == 0


def test_user_taps(ld):
    rng = np.random.default_rng(5)
    h, g = rng.standard_normal(37).astype(np.float32), rng.standard_normal(37).astype(np.float32)
    am = ld.AMBank(2, 4, taps=h, carrier_taps=g)
    assert (bits(am.taps) == bits(h)).all() and (bits(am.carrier_taps) == bits(g)).all()
    assert (bits(am.band_taps) == bits(band(h, g))).all()
    one = ld.AMBank(1, 8, taps=[1.0], carrier_taps=[0.5])
    assert one.ntaps == 1 and one.carrier_taps[0] == 0.5 and one.band_taps[0] == 0.5
    ld.AMBank(1, 1, taps=np.ones(1025, np.float32), carrier_taps=np.ones(1025, np.float32))   # the longest


# ---------------------------------------------------------------- the column schedule
def model(T, D, K):
    skip = (-T) % D
    ncols = -(-(K - skip) // D) if K > skip else 0
    return skip, ncols


@pytest.mark.parametrize("D", [1, 3, 32])
def test_num_outputs_and_skip_over_ragged_calls(ld, D):
    """Stepping the stream needs a device, so the sequence is checked through a bank's own
    bookkeeping where one is present and through the closed form at T = 0 otherwise."""
    am = ld.AMBank(2, D, ntaps=3)
    rng = np.random.default_rng(100 + D)
    lens = [0, 1, D - 1, D, D + 1, 0, 3 * D + 2] + [int(v) for v in rng.integers(0, 5 * D, 8)]
    T = 0
    for K in lens:
        skip, ncols = model(T, D, K)
        assert am.skip == skip
        for k in (0, 1, D - 1, D, D + 1, K):
            assert am.num_outputs(k) == model(T, D, k)[1], (T, k)
        if ld.device_count() == 0:
            continue                                 # the stream cannot advance: T stays 0
        y = am(np.zeros((2, K), np.complex64))
        assert y.shape == (2, ncols)
        T += K
    am.reset()
    assert am.skip == 0


# ---------------------------------------------------------------- errors
def test_constructor_errors(ld):
    for C_ in (0, -1, 257):
        with pytest.raises(ValueError):
            ld.AMBank(C_, 5)
    for D in (0, -3, 33, 1000):
        with pytest.raises(ValueError):
            ld.AMBank(3, D)
    for carrier in (0.0, -0.004, 0.1, 0.2, 0.6, np.nan, np.inf):     # 0.1 is the default audio cut-off at D = 5
        with pytest.raises(ValueError):
            ld.AMBank(3, 5, carrier=carrier)
    for audio in (0.0, -0.1, CARRIER, 0.01, 0.5001, 1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            ld.AMBank(3, 5, audio=audio, carrier=CARRIER)
    assert ld.AMBank(3, 5, audio=0.5, carrier=CARRIER).ntaps == 251
    for n in (0, -1, 1026):
        with pytest.raises(ValueError):
            ld.AMBank(3, 5, ntaps=n)
    for As in (0.0, -60.0, np.nan):
        with pytest.raises(ValueError):
            ld.AMBank(3, 5, As=As)
    for thr in (-0.01, np.nan):
        with pytest.raises(ValueError):
            ld.AMBank(3, 5, threshold=thr)
    with pytest.raises(NotImplementedError):
        ld.AMBank(3, 5, carrier=0.003)               # default L = 1335
    assert ld.AMBank(3, 5, carrier=0.003, ntaps=1025).ntaps == 1025
    ones = np.ones(8, np.float32)
    for kw in (dict(taps=ones), dict(carrier_taps=ones), dict(taps=ones, carrier_taps=ones[:7]),
               dict(taps=[], carrier_taps=[]), dict(taps=ones, carrier_taps=ones, ntaps=8),
               dict(taps=np.ones(1026), carrier_taps=np.ones(1026))):
        with pytest.raises(ValueError):
            ld.AMBank(3, 5, **kw)
    am = ld.AMBank(3, 5)
    for thr in (-1.0, np.nan):
        with pytest.raises(ValueError):
            am.threshold = thr
    assert am.threshold == 0.0


def test_create_codes(lib):
    nan = float("nan")
    for kw in (dict(C_=0), dict(C_=257), dict(D=0), dict(D=33), dict(carrier=0.0), dict(carrier=-0.1), dict(carrier=0.1),
               dict(carrier=0.5), dict(carrier=nan), dict(audio=-0.1), dict(audio=CARRIER), dict(audio=0.51),
               dict(audio=nan), dict(L=1026), dict(As=0.0), dict(As=nan), dict(thr=-0.5), dict(thr=nan),
               dict(D=1, carrier=0.45)):
        assert create(lib, **kw)[0] == LDSP_EINVAL, kw
    assert create(lib, carrier=0.003)[0] == LDSP_EUNSUP
    assert create(lib, carrier=0.0039)[0] == LDSP_EUNSUP
    assert create(lib, carrier=0.003, C_=0)[0] == LDSP_EINVAL         # a value out of range comes first
    assert lib.ldsp_ambank_create(3, 5, 0.0, CARRIER, 0, 60.0, 0.0, None) == LDSP_EINVAL
    h = np.ones(8, np.float32)
    q = C.c_void_p()
    for kw in (dict(C_=0), dict(C_=257), dict(D=0), dict(D=33), dict(thr=-1.0), dict(thr=nan), dict(L=0),
               dict(L=0, Lg=0), dict(Lg=7), dict(L=7), dict(L=1026, Lg=1026)):
        assert create_taps(lib, h, h, **kw)[0] == LDSP_EINVAL, kw
    assert lib.ldsp_ambank_create_taps(3, 5, None, 8, h.ctypes.data, 8, 0.0, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_ambank_create_taps(3, 5, h.ctypes.data, 8, None, 8, 0.0, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_ambank_create_taps(3, 5, h.ctypes.data, 8, h.ctypes.data, 8, 0.0, None) == LDSP_EINVAL
    for C_, D, L in ((1, 1, 1), (256, 32, 1025)):    # the ends of the ranges are allowed
        rc, q = create(lib, C_=C_, D=D, carrier=0.004, L=L)
        assert rc == 0 and lib.ldsp_ambank_destroy(q) == 0
    rc, q = create(lib, C_=2, D=4, carrier=0.004)
    assert rc == 0 and info(lib, q) == (2, 4, 1001, 0)
    assert lib.ldsp_ambank_get_info(q, None, None, None, None) == 0
    assert lib.ldsp_ambank_destroy(q) == 0


def test_execute_argument_errors_need_no_gpu(lib):
    rc, q = create(lib, 3, 4)
    assert rc == 0
    x = np.zeros((3, 64), np.complex64)
    y = np.zeros((3, 20), np.float32)
    xp, yp = x.ctypes.data, y.ctypes.data
    k = C.c_size_t(0)
    assert lib.ldsp_ambank_execute(q, xp, 64, 64, yp, 15, C.byref(k), MEM_HOST, None) == LDSP_ERANGE
    assert k.value == 16
    assert lib.ldsp_ambank_execute(q, xp, 64, 64, yp, 15, None, MEM_HOST, None) == LDSP_ERANGE
    assert lib.ldsp_ambank_execute(q, xp, 63, 64, yp, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_ambank_execute(None, xp, 64, 64, yp, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_ambank_execute(q, None, 64, 64, yp, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_ambank_execute(q, xp, 64, 64, None, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_ambank_execute(q, xp, 64, 64, yp, 20, C.byref(k), 7, None) == LDSP_EINVAL
    # the object is untouched: the same geometry, threshold and level as a fresh one
    rc, f = create(lib, 3, 4)
    assert info(lib, q) == info(lib, f) == (3, 4, 251, 0)
    t = C.c_float(-1.0)
    assert lib.ldsp_ambank_get_threshold(q, C.byref(t)) == 0 and t.value == 0.0
    assert lib.ldsp_ambank_set_threshold(q, -0.5) == LDSP_EINVAL
    assert lib.ldsp_ambank_set_threshold(q, float("nan")) == LDSP_EINVAL
    assert lib.ldsp_ambank_set_threshold(q, 0.05) == 0
    assert lib.ldsp_ambank_get_threshold(q, C.byref(t)) == 0 and np.float32(t.value) == np.float32(0.05)
    lv = np.full(3, np.nan, np.float32)
    assert lib.ldsp_ambank_get_carrier_level(q, lv.ctypes.data) == 0 and (lv == 0).all()
    assert lib.ldsp_ambank_get_carrier_level(q, None) == LDSP_EINVAL
    assert lib.ldsp_ambank_get_carrier_level(None, lv.ctypes.data) == LDSP_EINVAL
    assert lib.ldsp_ambank_num_outputs(q, 64, C.byref(k)) == 0 and k.value == 16
    assert lib.ldsp_ambank_num_outputs(q, 64, None) == LDSP_EINVAL
    assert lib.ldsp_ambank_num_outputs(None, 64, C.byref(k)) == LDSP_EINVAL
    assert lib.ldsp_ambank_get_taps(None, None, None, None) == LDSP_EINVAL
    assert lib.ldsp_ambank_get_info(None, None, None, None, None) == LDSP_EINVAL
    assert lib.ldsp_ambank_get_threshold(q, None) == LDSP_EINVAL
    assert lib.ldsp_ambank_get_threshold(None, C.byref(t)) == LDSP_EINVAL
    assert lib.ldsp_ambank_set_threshold(None, 0.1) == LDSP_EINVAL
    assert lib.ldsp_ambank_reset(None) == LDSP_EINVAL
    assert lib.ldsp_ambank_reset(q) == 0
    assert lib.ldsp_ambank_destroy(q) == 0 and lib.ldsp_ambank_destroy(f) == 0
    assert lib.ldsp_ambank_destroy(None) == 0


def test_python_shape_and_dtype_errors_need_no_gpu(ld):
    am = ld.AMBank(3, 4)
    for bad in (np.zeros((2, 64), np.complex64), np.zeros((4, 64), np.complex64), np.zeros(64, np.complex64),
                np.zeros((3, 4, 4), np.complex64)):
        with pytest.raises(ValueError):
            am(bad)
    for dt in (np.complex128, np.float32, np.int16):  # other numeric dtypes are cast, as the other banks': the shape decides
        with pytest.raises(ValueError):
            am(np.zeros((2, 64), dt))
    assert am.skip == 0
    if ld.device_count() == 0:                       # a well-formed call without a device is an error, not a fallback
        for dt in (np.complex64, np.complex128):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                am(np.zeros((3, 64), dt))


# ---------------------------------------------------------------- the tile hook
def test_tile_hook(lib, ld):
    """64 columns per workgroup at every (D, L): the widest span, D = 32 with L = 1025, takes 24 KiB of LDS."""
    f = C.c_size_t()
    for D, L in ((1, 1), (1, 1025), (5, 251), (8, 363), (32, 1), (32, 1025)):
        assert lib.ldsp_debug_ambank_tile(D, L, C.byref(f)) == 0
        assert f.value == 64, (D, L)
        assert ld.AMBank(1, D, ntaps=L).tile == 64
    assert lib.ldsp_debug_ambank_tile(0, 8, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_ambank_tile(33, 8, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_ambank_tile(8, 0, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_ambank_tile(8, 1026, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_ambank_tile(8, 8, None) == LDSP_EINVAL


# ---------------------------------------------------------------- the C driver under ASan + UBSan
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:")


def test_ambank_driver_asan_ubsan():
    """The host code of the C ABI (creation, design, argument checks, num_outputs) in a stand-alone
    instrumented program; no GPU and nothing loaded into Python."""
    r = subprocess.run(["make", "-s", "-j8", "-C", PKG, "ambank_asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(PKG, "build", "ambank_driver_asan")
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the driver is not instrumented"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert not any(k in out for k in REPORTS), out[-4000:]
    assert "all checks passed" in r.stdout
