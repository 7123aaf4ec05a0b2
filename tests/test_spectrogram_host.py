"""Host side of the Spectrogram without a GPU (CPU suite): construction and
defaults, the named windows against their formulas, the output schedule of
first calls, freqs and the empty psd, every argument error of
ldsp_spgram_create* / _execute (decided before any device work) and the tile
hook.  The GPU side is tests/test_gpu_spectrogram.py."""
import ctypes as C
import os

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
LIBPATH = os.path.join(REPO, "python-liquiddsp_amd", "libldsp.so")

LDSP_EINVAL, LDSP_EHIP, LDSP_EUNSUP = -1, -3, -5
MEM_HOST, MEM_DEVICE = 0, 1
WIN = {"rect": 0, "hann": 1, "hamming": 2, "blackmanharris": 3}
SIZES = (256, 512, 1024, 2048, 4096)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIBPATH):
        pytest.fail("libldsp.so not built (run __graft_entry__.build())")
    L = C.CDLL(LIBPATH)
    L.ldsp_last_error.restype = C.c_char_p
    vp, u, sz, u64 = C.c_void_p, C.c_uint, C.c_size_t, C.c_uint64
    L.ldsp_spgram_create.argtypes = [u, C.c_int, u, u, u, C.POINTER(vp)]
    L.ldsp_spgram_create_window.argtypes = [u, vp, u, u, u, C.POINTER(vp)]
    for f in (L.ldsp_spgram_destroy, L.ldsp_spgram_reset, L.ldsp_spgram_clear):
        f.argtypes = [vp]
    L.ldsp_spgram_get_info.argtypes = [vp] + [C.POINTER(u)] * 4 + [C.POINTER(u64)] * 2
    L.ldsp_spgram_get_window.argtypes = [vp, vp]
    L.ldsp_spgram_num_outputs.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(sz)]
    L.ldsp_spgram_execute.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    L.ldsp_spgram_get_psd.argtypes = [vp, vp, C.POINTER(u64)]
    L.ldsp_debug_spgram_tile.argtypes = [u, C.POINTER(sz)]
    return L


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def create(lib, N, wtype=1, W=None, d=None, A=1):
    W = N if W is None else W
    d = max(W // 2, 1) if d is None else d
    q = C.c_void_p()
    return lib.ldsp_spgram_create(N, wtype, W, d, A, C.byref(q)), q


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def window_f64(name, W):
    """The issue's formulas in float64, normalised to sum w^2 = 1."""
    if W == 1:
        return np.ones(1)
    t = np.arange(W, dtype=np.float64) / (W - 1)
    c1, c2, c3 = np.cos(2 * np.pi * t), np.cos(4 * np.pi * t), np.cos(6 * np.pi * t)
    w = {"rect": np.ones(W), "hann": 0.5 - 0.5 * c1, "hamming": 0.53836 - 0.46164 * c1,
         "blackmanharris": 0.35875 - 0.48829 * c1 + 0.14128 * c2 - 0.01168 * c3}[name]
    with np.errstate(invalid="ignore"):                # hann of two taps: 0 / 0
        return w / np.sqrt(np.sum(w * w))


# ---------------------------------------------------------------- construction
def test_defaults(ld):
    s = ld.Spectrogram(1024)
    assert (s.nfft, s.window_len, s.delay, s.average) == (1024, 1024, 512, 1)
    assert (s.num_samples, s.num_transforms) == (0, 0)
    assert ld.Spectrogram(512, window_len=200).delay == 100
    assert ld.Spectrogram(256, window_len=1).delay == 1
    s = ld.Spectrogram(nfft=2048, window="rect", window_len=300, delay=7, average=3)
    assert (s.nfft, s.window_len, s.delay, s.average) == (2048, 300, 7, 3)
    s.reset()                                        # before the first call: nothing on the device yet
    s.clear()


# ---------------------------------------------------------------- windows
@pytest.mark.parametrize("name", sorted(WIN))
@pytest.mark.parametrize("W", [1, 2, 255, 4096])
def test_named_window(ld, lib, name, W):
    ref = window_f64(name, W)
    s = ld.Spectrogram(4096, window=name, window_len=W)
    w = s.window
    assert w.dtype == np.float32 and w.shape == (W,)
    if name == "hann" and W == 2:
        # both taps of a two-point Hann window are zero: the formula's 0 / 0, here as there
        assert np.isnan(ref).all() and np.isnan(w).all()
    else:
        # within one float32 ulp of the float64 formula (the rounding itself is half an ulp)
        ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64)
        assert np.all(np.abs(w.astype(np.float64) - ref) <= ulp), np.max(np.abs(w - ref) / ulp)
        assert abs(np.sum(w.astype(np.float64) ** 2) - 1.0) <= 1e-6
    # the same window through the C ABI
    rc, q = create(lib, 4096, WIN[name], W, 1, 1)
    assert rc == 0, lib.ldsp_last_error()
    No, Wo, do, Ao = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
    T, S = C.c_uint64(9), C.c_uint64(9)
    assert lib.ldsp_spgram_get_info(q, C.byref(No), C.byref(Wo), C.byref(do), C.byref(Ao), C.byref(T), C.byref(S)) == 0
    assert (No.value, Wo.value, do.value, Ao.value, T.value, S.value) == (4096, W, 1, 1, 0, 0)
    h = np.full(W, 7.0, np.float32)
    assert lib.ldsp_spgram_get_window(q, h.ctypes.data) == 0
    assert np.array_equal(h.view(np.uint32), w.view(np.uint32))
    assert lib.ldsp_spgram_destroy(q) == 0


def test_user_window_bitwise(ld, lib, rng):
    w = rng.standard_normal(300).astype(np.float32)
    s = ld.Spectrogram(1024, window=w, window_len=300, delay=7)
    assert s.window.dtype == np.float32 and (bits(s.window) == bits(w)).all()
    # float64 in: cast to float32, not normalised
    w64 = rng.standard_normal(256)
    assert (bits(ld.Spectrogram(256, window=w64).window) == bits(w64.astype(np.float32))).all()
    with pytest.raises(ValueError):
        ld.Spectrogram(1024, window=w, window_len=299)
    q = C.c_void_p()
    assert lib.ldsp_spgram_create_window(1024, w.ctypes.data, 300, 7, 3, C.byref(q)) == 0
    h = np.zeros(300, np.float32)
    assert lib.ldsp_spgram_get_window(q, h.ctypes.data) == 0 and (bits(h) == bits(w)).all()
    assert lib.ldsp_spgram_destroy(q) == 0


# ---------------------------------------------------------------- schedule
@pytest.mark.parametrize("N,W,d,A", [(256, 256, 128, 1), (1024, 300, 7, 3), (4096, 4096, 4096, 5)])
def test_num_outputs_fresh(ld, lib, N, W, d, A):
    s = ld.Spectrogram(N, window_len=W, delay=d, average=A)
    rc, q = create(lib, N, 1, W, d, A)
    assert rc == 0
    for n in (0, 1, d - 1, d, d + 1, A * d - 1, A * d, 5 * A * d + 3):
        want = (n // d, (n // d) // A)
        assert s.num_outputs(n) == want, n
        nt, nr = C.c_size_t(99), C.c_size_t(99)
        assert lib.ldsp_spgram_num_outputs(q, n, C.byref(nt), C.byref(nr)) == 0
        assert (nt.value, nr.value) == want
    assert lib.ldsp_spgram_destroy(q) == 0


# ---------------------------------------------------------------- freqs, empty psd
@pytest.mark.parametrize("N", SIZES)
def test_freqs_and_empty_psd(ld, lib, N):
    s = ld.Spectrogram(N)
    k = np.arange(N, dtype=np.float64)
    f = s.freqs
    assert f.dtype == np.float64 and np.array_equal(f, ((k / N + 0.5) % 1.0) - 0.5)
    assert f[0] == 0.0 and f[N // 2] == -0.5 and f[N - 1] == -1.0 / N
    p = s.psd
    assert p.dtype == np.float64 and p.shape == (N,) and not p.any()
    assert s.num_transforms == 0
    rc, q = create(lib, N)
    assert rc == 0
    buf = np.full(N, 3.0)
    S = C.c_uint64(5)
    assert lib.ldsp_spgram_get_psd(q, buf.ctypes.data, C.byref(S)) == 0
    assert S.value == 0 and not buf.any()
    assert lib.ldsp_spgram_destroy(q) == 0


# ---------------------------------------------------------------- errors
BAD = [
    # N, W, d, A, code
    (1000, 1000, 500, 1, LDSP_EINVAL),       # not a power of two
    (0, 1, 1, 1, LDSP_EINVAL),
    (768, 768, 384, 1, LDSP_EINVAL),
    (128, 128, 64, 1, LDSP_EUNSUP),          # a power of two below 256
    (8192, 8192, 4096, 1, LDSP_EUNSUP),      # and above 4096
    (1024, 0, 1, 1, LDSP_EINVAL),            # W = 0
    (1024, 1025, 512, 1, LDSP_EINVAL),       # W > N
    (1024, 1024, 0, 1, LDSP_EINVAL),         # d = 0
    (1024, 300, 301, 1, LDSP_EUNSUP),        # d > W
    (1024, 1024, 512, 0, LDSP_EINVAL),       # A = 0
]


@pytest.mark.parametrize("N,W,d,A,code", BAD)
def test_create_errors(ld, lib, N, W, d, A, code):
    q = C.c_void_p()
    assert lib.ldsp_spgram_create(N, 1, W, d, A, C.byref(q)) == code
    assert not q.value and lib.ldsp_last_error()
    w = np.ones(max(W, 1), np.float32)
    assert lib.ldsp_spgram_create_window(N, w.ctypes.data, W, d, A, C.byref(q)) == code
    exc = ValueError if code == LDSP_EINVAL else NotImplementedError
    with pytest.raises(exc):
        ld.Spectrogram(N, window_len=W, delay=d, average=A)
    with pytest.raises(exc):
        ld.Spectrogram(N, window=w[:W] if W else w[:0], window_len=W, delay=d, average=A)


def test_create_other_errors(ld, lib):
    q = C.c_void_p()
    for wt in (-1, 4, 99):
        assert lib.ldsp_spgram_create(1024, wt, 1024, 512, 1, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_spgram_create(1024, 1, 1024, 512, 1, None) == LDSP_EINVAL
    assert lib.ldsp_spgram_create_window(1024, None, 1024, 512, 1, C.byref(q)) == LDSP_EINVAL
    w = np.ones(4, np.float32)
    assert lib.ldsp_spgram_create_window(1024, w.ctypes.data, 4, 2, 1, None) == LDSP_EINVAL
    with pytest.raises(ValueError):
        ld.Spectrogram(1024, window="kaiser")
    for kw in ({"nfft": -1024}, {"nfft": 1024, "window_len": -1}, {"nfft": 1024, "delay": -1},
               {"nfft": 1024, "average": -1}):
        with pytest.raises(ValueError):
            ld.Spectrogram(**kw)


def test_null_handles(lib):
    rc, q = create(lib, 1024)
    assert rc == 0
    sz = C.c_size_t()
    assert lib.ldsp_spgram_num_outputs(None, 64, C.byref(sz), C.byref(sz)) == LDSP_EINVAL
    assert lib.ldsp_spgram_get_window(q, None) == LDSP_EINVAL
    assert lib.ldsp_spgram_get_window(None, None) == LDSP_EINVAL
    assert lib.ldsp_spgram_get_psd(q, None, None) == LDSP_EINVAL
    assert lib.ldsp_spgram_get_info(None, None, None, None, None, None, None) == LDSP_EINVAL
    assert lib.ldsp_spgram_get_info(q, None, None, None, None, None, None) == 0
    assert lib.ldsp_spgram_reset(None) == LDSP_EINVAL
    assert lib.ldsp_spgram_clear(None) == LDSP_EINVAL
    assert lib.ldsp_debug_spgram_tile(1024, None) == LDSP_EINVAL
    assert lib.ldsp_spgram_reset(q) == 0 and lib.ldsp_spgram_clear(q) == 0
    assert lib.ldsp_spgram_destroy(q) == 0
    assert lib.ldsp_spgram_destroy(None) == 0


def test_execute_argument_errors_need_no_device(lib):
    """NULL x, a bad mem and a short row stride are refused on the host: the
    same codes with and without a GPU, and the stream position stays at 0."""
    rc, q = create(lib, 256, 1, 256, 128, 1)
    assert rc == 0
    x = np.zeros(1024, np.complex64)
    y = np.zeros((8, 256), np.float32)
    nr = C.c_size_t(99)
    ex = lib.ldsp_spgram_execute
    assert ex(None, x.ctypes.data, 1024, y.ctypes.data, 256, C.byref(nr), MEM_HOST, None) == LDSP_EINVAL
    assert ex(q, None, 1024, y.ctypes.data, 256, C.byref(nr), MEM_HOST, None) == LDSP_EINVAL
    assert nr.value == 8                              # the count is still reported
    assert ex(q, x.ctypes.data, 1024, y.ctypes.data, 256, C.byref(nr), 7, None) == LDSP_EINVAL
    assert ex(q, x.ctypes.data, 1024, y.ctypes.data, 255, C.byref(nr), MEM_HOST, None) == LDSP_EINVAL
    assert ex(q, x.ctypes.data, 1024, y.ctypes.data, 0, C.byref(nr), MEM_DEVICE, None) == LDSP_EINVAL
    T, S = C.c_uint64(9), C.c_uint64(9)
    assert lib.ldsp_spgram_get_info(q, None, None, None, None, C.byref(T), C.byref(S)) == 0
    assert (T.value, S.value) == (0, 0)
    assert lib.ldsp_spgram_destroy(q) == 0


# ---------------------------------------------------------------- no GPU
def test_call_raises_without_gpu(ld):
    if ld.device_count() > 0:
        pytest.skip("a GPU is present")
    s = ld.Spectrogram(256)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s(np.zeros(64, np.complex64))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        s.write(np.zeros(64, np.complex64))
    assert (s.num_samples, s.num_transforms) == (0, 0)


# ---------------------------------------------------------------- tile hook
def test_tile_hook(ld, lib):
    t = C.c_size_t()
    for N in SIZES:
        assert lib.ldsp_debug_spgram_tile(N, C.byref(t)) == 0
        assert t.value >= 1 and t.value == ld.Spectrogram(N).tile
    assert lib.ldsp_debug_spgram_tile(1000, C.byref(t)) == LDSP_EINVAL
    assert lib.ldsp_debug_spgram_tile(128, C.byref(t)) == LDSP_EUNSUP
    assert lib.ldsp_debug_spgram_tile(8192, C.byref(t)) == LDSP_EUNSUP
