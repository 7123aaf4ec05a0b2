"""Host side of the SSBBank without a GPU (CPU suite): the exported
ldsp_ssbbank_* symbols, construction and defaults, the designed prototype
(bit-identical to the restatement's firdes_kaiser normalised the same way), the
rows' complex taps g against the definition with the phase psi in exact integer
arithmetic, user taps, the BFO words, num_outputs / skip over ragged call
lengths against the closed form, the bfo and sideband setters, every argument
error of ldsp_ssbbank_create* / _set_* / _execute (decided before any device
work), the Python shape and dtype errors, the tile hook, and the stand-alone C
driver of the same host code under ASan + UBSan
(tests/sanitize/ssbbank_driver.c).  The GPU side is tests/test_gpu_ssbbank.py.

Row taps: the library forms cos and sin with the C library's double functions,
this file with numpy's; the two may differ in the last bit of a double, which
can move the float32 rounding of p[j] cos by one ulp.  The gate is therefore
1 ulp per component, and the test prints how many components are not bitwise
equal (none with the C library and the numpy this was written against)."""
import ctypes as C
import math
import os
import re
import subprocess

import numpy as np
import pytest

from bank_prototypes import row_taps

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
    vp, u, f, d, sz = C.c_void_p, C.c_uint, C.c_float, C.c_double, C.c_size_t
    L.ldsp_ssbbank_create.argtypes = [u, u, d, d, u, f, vp, vp, C.POINTER(vp)]
    L.ldsp_ssbbank_create_taps.argtypes = [u, u, vp, u, d, d, vp, vp, C.POINTER(vp)]
    L.ldsp_ssbbank_destroy.argtypes = [vp]
    L.ldsp_ssbbank_reset.argtypes = [vp]
    L.ldsp_ssbbank_get_info.argtypes = [vp, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(u)]
    L.ldsp_ssbbank_get_band.argtypes = [vp, C.POINTER(d), C.POINTER(d)]
    L.ldsp_ssbbank_get_taps.argtypes = [vp, vp, vp]
    L.ldsp_ssbbank_get_words.argtypes = [vp, vp]
    L.ldsp_ssbbank_get_bfo.argtypes = [vp, vp]
    L.ldsp_ssbbank_set_bfo.argtypes = [vp, vp]
    L.ldsp_ssbbank_get_sideband.argtypes = [vp, vp]
    L.ldsp_ssbbank_set_sideband.argtypes = [vp, vp]
    L.ldsp_ssbbank_num_outputs.argtypes = [vp, sz, C.POINTER(sz)]
    L.ldsp_ssbbank_execute.argtypes = [vp, vp, sz, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    L.ldsp_debug_ssbbank_tile.argtypes = [u, u, C.POINTER(sz)]
    L.ldsp_debug_ssbbank_seek.argtypes = [vp, C.c_uint64]
    return L


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def lists(C_, bfo=None, side=None):
    b = np.zeros(C_, np.float64) if bfo is None else np.asarray(bfo, np.float64)
    s = np.ones(C_, np.int32) if side is None else np.asarray(side, np.int32)
    return b, s


def create(lib, C_=3, D=2, lo=0.025, hi=0.0, L=0, As=60.0, bfo=None, side=None):
    b, s = lists(max(C_, 1), bfo, side)
    q = C.c_void_p()
    return lib.ldsp_ssbbank_create(C_, D, lo, hi, L, As, b.ctypes.data, s.ctypes.data, C.byref(q)), q


def create_taps(lib, p, C_=3, D=2, lo=0.025, hi=0.0, L=None, bfo=None, side=None):
    p = np.asarray(p, np.float32)
    b, s = lists(max(C_, 1), bfo, side)
    q = C.c_void_p()
    return lib.ldsp_ssbbank_create_taps(C_, D, p.ctypes.data, p.size if L is None else L, lo, hi, b.ctypes.data,
                                        s.ctypes.data, C.byref(q)), q


def info(lib, q):
    c, d, l, s = C.c_uint(), C.c_uint(), C.c_uint(), C.c_uint()
    assert lib.ldsp_ssbbank_get_info(q, C.byref(c), C.byref(d), C.byref(l), C.byref(s)) == 0
    return c.value, d.value, l.value, s.value


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def designed(ora, L, fc, As):
    """firdes_kaiser with every tap divided in double by the double sum of the float32 design."""
    h = ora.firdes_kaiser(L, np.float32(fc), As, 0)
    return (h.astype(np.float64) / np.sum(h.astype(np.float64))).astype(np.float32)


def word(bfo):
    """rint(bfo 2^32) mod 2^32 in exact integer arithmetic (the product is exact; round-half-even)."""
    return int(np.rint(np.float64(bfo) * 4294967296.0)) % (1 << 32)


def ulps(a, b):
    """Distance in float32 steps per component of two complex64 arrays."""
    fa, fb = (np.ascontiguousarray(v).view(np.float32).view(np.int32).astype(np.int64) for v in (a, b))
    fa, fb = (np.where(v < 0, -(v & 0x7FFFFFFF), v) for v in (fa, fb))
    return np.abs(fa - fb)


# ---------------------------------------------------------------- symbols
def test_library_exports_what_the_header_declares(lib):
    with open(HEADER) as f:
        names = sorted(set(re.findall(r"\b(ldsp_(?:debug_)?ssbbank_\w+)\s*\(", f.read())))
    want = {"ldsp_ssbbank_create", "ldsp_ssbbank_create_taps", "ldsp_ssbbank_destroy", "ldsp_ssbbank_reset",
            "ldsp_ssbbank_get_info", "ldsp_ssbbank_get_band", "ldsp_ssbbank_get_taps", "ldsp_ssbbank_get_words",
            "ldsp_ssbbank_get_bfo", "ldsp_ssbbank_set_bfo", "ldsp_ssbbank_get_sideband", "ldsp_ssbbank_set_sideband",
            "ldsp_ssbbank_num_outputs", "ldsp_ssbbank_execute", "ldsp_debug_ssbbank_tile", "ldsp_debug_ssbbank_seek"}
    assert want == set(names), sorted(want ^ set(names))
    for n in names:
        assert hasattr(lib, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", LIBPATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(ldsp_(?:debug_)?ssbbank_\w+)\b", out))
    assert exported == want, sorted(exported ^ want)


# ---------------------------------------------------------------- construction
def test_defaults(ld):
    sb = ld.SSBBank(16)
    assert (sb.nchan, sb.decim, sb.skip, sb.tile) == (16, 1, 0, 128)
    assert (sb.lo, sb.hi, sb.ntaps) == (0.025, 0.5 - 0.025, 81)
    assert sb.taps.dtype == np.float32 and sb.taps.shape == (81,)
    assert sb.row_taps.dtype == np.complex64 and sb.row_taps.shape == (16, 81)
    assert sb.bfo.dtype == np.float64 and (sb.bfo == 0).all() and sb.bfo.shape == (16,)
    assert sb.words.dtype == np.uint32 and (sb.words == 0).all()
    assert sb.sideband == ["usb"] * 16
    sb.reset()                                       # before the first call: nothing on the device yet
    for D, hi in ((1, 0.475), (2, 0.225), (4, 0.1)):
        sb = ld.SSBBank(2, D)
        assert (sb.lo, sb.hi, sb.ntaps) == (0.025, 0.5 / D - 0.025, 81), D
    for lo, L in ((0.0625, 33), (0.025, 81), (0.01, 201), (1 / 512, 1025)):
        sb = ld.SSBBank(2, lo=lo)
        assert sb.ntaps == L == 2 * math.ceil(1 / lo) + 1 and sb.hi == 0.5 - lo
    kw = ld.SSBBank(nchan=256, decim=32, lo=0.002, hi=0.015, bfo=0.25, sideband="lsb", ntaps=1025, As=40.0, taps=None)
    assert (kw.nchan, kw.decim, kw.ntaps, kw.lo, kw.hi) == (256, 32, 1025, 0.002, 0.015)
    assert (kw.bfo == 0.25).all() and kw.sideband == ["lsb"] * 256 and (kw.words == 1 << 30).all()
    assert ld.SSBBank(1, ntaps=1).ntaps == 1
    per = ld.SSBBank(3, 2, bfo=[0.0, 0.1, -0.3], sideband=["usb", "lsb", "usb"])
    assert per.bfo.tolist() == [0.0, 0.1, -0.3] and per.sideband == ["usb", "lsb", "usb"]
    per = ld.SSBBank(3, 2, bfo=np.array([0.0, 0.1, -0.3]), sideband=("lsb", "lsb", "usb"))
    assert per.sideband == ["lsb", "lsb", "usb"]


# ---------------------------------------------------------------- design
DESIGNS = [(1, 0.0625, 0.4, None, 60.0), (2, 0.025, None, None, 60.0), (4, 0.01, 0.1, None, 60.0),
           (5, 0.004, 0.1, 501, 60.0), (32, 0.002, 0.015, 1001, 40.0), (3, 1 / 32, 0.16, 65, 80.0)]


@pytest.mark.parametrize("D,lo,hi,L,As", DESIGNS)
def test_designed_prototype_bitwise(ld, lib, ora, D, lo, hi, L, As):
    sb = ld.SSBBank(2, D, lo=lo, hi=hi, ntaps=L, As=As)
    n = L or 2 * math.ceil(1 / lo) + 1
    fh = hi if hi is not None else 0.5 / D - lo
    p = designed(ora, n, (fh - lo) / 2, As)
    assert sb.ntaps == n and sb.hi == fh
    assert sb.taps.shape == p.shape and (bits(sb.taps) == bits(p)).all()
    assert abs(np.sum(sb.taps.astype(np.float64)) - 1) < 1e-6
    rc, q = create(lib, 2, D, lo, hi or 0.0, L or 0, As)
    assert rc == 0, lib.ldsp_last_error()
    a = np.full(n, np.nan, np.float32)
    g = np.full((2, n), np.nan, np.complex64)
    assert lib.ldsp_ssbbank_get_taps(q, a.ctypes.data, g.ctypes.data) == 0
    assert (bits(a) == bits(p)).all() and (bits(g) == bits(sb.row_taps)).all()
    assert lib.ldsp_ssbbank_get_taps(q, None, None) == 0
    assert lib.ldsp_ssbbank_destroy(q) == 0


@pytest.mark.parametrize("D,lo,hi,L,As", DESIGNS)
def test_row_taps_against_the_definition(ld, D, lo, hi, L, As):
    rng = np.random.default_rng(11 + D)
    C_ = 7
    bfo = np.concatenate([[0.0, -0.5, 0.5, 0.3], rng.uniform(-0.5, 0.5, C_ - 4)])
    side = ["usb", "lsb"] * 3 + ["usb"]
    sb = ld.SSBBank(C_, D, lo=lo, hi=hi, bfo=bfo, sideband=side, ntaps=L, As=As)
    want = row_taps(sb.taps, sb.lo, sb.hi, sb.words, [1 if s == "usb" else -1 for s in side])
    got = sb.row_taps
    off = ulps(got, want)
    print(f"D={D} L={sb.ntaps}: {int((off != 0).sum())} of {off.size} components not bitwise equal, worst {int(off.max())} ulp")
    assert off.max() <= 1
    # the band-pass sits on the chosen sideband: its response at the band's centre above the BFO is 1, below it small
    fm = (sb.lo + sb.hi) / 2
    j = np.arange(sb.ntaps)
    for c in (0, 3, 4):
        s = 1 if side[c] == "usb" else -1
        f_on, f_off = bfo[c] + s * fm, bfo[c] - s * fm
        # S = sum g[j] x[n - j] with x = exp(2 pi i f t): gain sum g[j] exp(-2 pi i f j)
        H = lambda f: abs(np.sum(got[c].astype(np.complex128) * np.exp(-2j * np.pi * f * j)))
        assert abs(H(f_on) - 1) < 2e-3, (c, H(f_on))
        assert H(f_off) < 10 ** (-As / 20) * 3, (c, H(f_off))


def test_user_taps(ld, lib):
    rng = np.random.default_rng(5)
    p = rng.standard_normal(37).astype(np.float32)
    sb = ld.SSBBank(2, 4, lo=0.01, hi=0.1, bfo=[0.2, -0.1], sideband=["lsb", "usb"], taps=p)
    assert sb.ntaps == 37 and (bits(sb.taps) == bits(p)).all() and (sb.lo, sb.hi) == (0.01, 0.1)
    assert ulps(sb.row_taps, row_taps(p, 0.01, 0.1, sb.words, [-1, 1])).max() <= 1
    even = rng.standard_normal(36).astype(np.float32)  # an even length: the tap phase counts in 2^-33 turns
    sb = ld.SSBBank(3, 4, lo=0.01, hi=0.1, bfo=[0.2, -0.1, 0.0], sideband=["lsb", "usb", "usb"], taps=even)
    assert sb.ntaps == 36 and (bits(sb.taps) == bits(even)).all()
    assert ulps(sb.row_taps, row_taps(even, 0.01, 0.1, sb.words, [-1, 1, 1])).max() <= 1
    one = ld.SSBBank(1, 8, lo=0.01, taps=[0.5])       # L = 1: psi = 0, g = p
    assert one.ntaps == 1 and one.row_taps[0, 0] == 0.5 and one.hi == 0.0625 - 0.01
    ld.SSBBank(1, 1, taps=np.ones(1025, np.float32))  # the longest
    rc, q = create_taps(lib, p, 2, 4, 0.01, 0.1)
    assert rc == 0 and info(lib, q) == (2, 4, 37, 0)
    lo, hi = C.c_double(), C.c_double()
    assert lib.ldsp_ssbbank_get_band(q, C.byref(lo), C.byref(hi)) == 0 and (lo.value, hi.value) == (0.01, 0.1)
    assert lib.ldsp_ssbbank_get_band(q, None, None) == 0
    assert lib.ldsp_ssbbank_destroy(q) == 0


def test_words(ld):
    bfo = [0.5, -0.5, 0.0, -0.25, 0.25, -1e-10, 1e-10, -0.1, 0.1, 0.5 - 2.0 ** -33, -(2.0 ** -33), 3 * 2.0 ** -33]
    sb = ld.SSBBank(len(bfo), 2, bfo=bfo)
    w = sb.words
    assert w.tolist() == [word(f) for f in bfo]
    assert w[0] == w[1] == 1 << 31 and w[2] == 0 and w[3] == 3 << 30 and w[4] == 1 << 30
    assert w[5] == 0 and w[6] == 0                    # below half a step of the grid
    assert int(w[7]) + int(w[8]) == 1 << 32
    assert w[9] == 1 << 31 and w[10] == 0 and w[11] == 2   # ties go to the even word
    assert sb.bfo.tolist() == bfo                     # the BFOs read back as given


# ---------------------------------------------------------------- the column schedule
def model(T, D, K):
    skip = (-T) % D
    ncols = -(-(K - skip) // D) if K > skip else 0
    return skip, ncols


@pytest.mark.parametrize("D", [1, 3, 32])
def test_num_outputs_and_skip_over_ragged_calls(ld, lib, D):
    """Stepping the stream needs a device, so without one the sequence is taken through the seek hook,
    which sets the stream position on the host."""
    sb = ld.SSBBank(2, D, lo=0.002, hi=0.015, ntaps=3)
    rng = np.random.default_rng(100 + D)
    lens = [0, 1, D - 1, D, D + 1, 0, 3 * D + 2] + [int(v) for v in rng.integers(0, 5 * D, 8)]
    T = 0
    for K in lens:
        skip, ncols = model(T, D, K)
        assert sb.skip == skip
        for k in (0, 1, D - 1, D, D + 1, K):
            assert sb.num_outputs(k) == model(T, D, k)[1], (T, k)
        if ld.device_count() == 0:
            T += K
            sb._seek(T)
            continue
        y = sb(np.zeros((2, K), np.complex64))
        assert y.shape == (2, ncols)
        T += K
    for T in (2 ** 32 - 1, 2 ** 32 + 5, 3 * 2 ** 32 + 5, 2 ** 63 + 11):
        sb._seek(T)
        assert sb.skip == (-T) % D and sb.num_outputs(100) == model(T, D, 100)[1]
    sb.reset()
    assert sb.skip == 0


# ---------------------------------------------------------------- setters
def test_setters_round_trip(ld, lib):
    sb = ld.SSBBank(4, 2, bfo=[0.0, 0.1, -0.2, 0.3], sideband=["usb", "lsb", "usb", "lsb"])
    g0 = sb.row_taps.copy()
    sb.bfo = [0.3, -0.2, 0.1, 0.0]
    assert sb.bfo.tolist() == [0.3, -0.2, 0.1, 0.0] and sb.words.tolist() == [word(f) for f in (0.3, -0.2, 0.1, 0.0)]
    assert sb.sideband == ["usb", "lsb", "usb", "lsb"]                     # untouched
    fresh = ld.SSBBank(4, 2, bfo=[0.3, -0.2, 0.1, 0.0], sideband=["usb", "lsb", "usb", "lsb"])
    assert (bits(sb.row_taps) == bits(fresh.row_taps)).all() and not (bits(sb.row_taps) == bits(g0)).all()
    sb.sideband = ["lsb", "lsb", "usb", "usb"]
    assert sb.sideband == ["lsb", "lsb", "usb", "usb"] and sb.bfo.tolist() == [0.3, -0.2, 0.1, 0.0]
    fresh = ld.SSBBank(4, 2, bfo=[0.3, -0.2, 0.1, 0.0], sideband=["lsb", "lsb", "usb", "usb"])
    assert (bits(sb.row_taps) == bits(fresh.row_taps)).all()
    sb.bfo = -0.125                                   # a scalar: every row
    sb.sideband = "usb"
    assert (sb.bfo == -0.125).all() and sb.sideband == ["usb"] * 4 and (sb.words == 7 << 29).all()
    for bad in ([0.1, 0.2], [0.1] * 5, 0.6, -0.51, np.nan, np.inf, [0.0, 0.0, np.nan, 0.0]):
        with pytest.raises(ValueError):
            sb.bfo = bad
    for bad in (["usb"], ["usb"] * 5, "dsb", "USB", 1, ["usb", "lsb", "am", "usb"], None):
        with pytest.raises(ValueError):
            sb.sideband = bad
    assert (sb.bfo == -0.125).all() and sb.sideband == ["usb"] * 4         # a refused list changes nothing
    # the C ABI
    rc, q = create(lib, 3, 2, bfo=[0.0, 0.1, -0.2], side=[1, -1, 1])
    assert rc == 0
    b, s, w = np.full(3, np.nan), np.zeros(3, np.int32), np.zeros(3, np.uint32)
    assert lib.ldsp_ssbbank_get_bfo(q, b.ctypes.data) == 0 and b.tolist() == [0.0, 0.1, -0.2]
    assert lib.ldsp_ssbbank_get_sideband(q, s.ctypes.data) == 0 and s.tolist() == [1, -1, 1]
    nb, ns = np.array([0.5, -0.5, 0.25]), np.array([-1, -1, 1], np.int32)
    assert lib.ldsp_ssbbank_set_bfo(q, nb.ctypes.data) == 0 and lib.ldsp_ssbbank_set_sideband(q, ns.ctypes.data) == 0
    assert lib.ldsp_ssbbank_get_bfo(q, b.ctypes.data) == 0 and b.tolist() == [0.5, -0.5, 0.25]
    assert lib.ldsp_ssbbank_get_sideband(q, s.ctypes.data) == 0 and s.tolist() == [-1, -1, 1]
    assert lib.ldsp_ssbbank_get_words(q, w.ctypes.data) == 0 and w.tolist() == [1 << 31, 1 << 31, 1 << 30]
    for bad in (np.array([0.0, 0.6, 0.0]), np.array([0.0, np.nan, 0.0]), np.array([-0.75, 0.0, 0.0])):
        assert lib.ldsp_ssbbank_set_bfo(q, bad.ctypes.data) == LDSP_EINVAL
    for bad in ([0, 1, 1], [1, 2, 1], [1, 1, -2]):
        assert lib.ldsp_ssbbank_set_sideband(q, np.array(bad, np.int32).ctypes.data) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_set_bfo(q, None) == LDSP_EINVAL and lib.ldsp_ssbbank_set_sideband(q, None) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_set_bfo(None, nb.ctypes.data) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_set_sideband(None, ns.ctypes.data) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_get_bfo(q, b.ctypes.data) == 0 and b.tolist() == [0.5, -0.5, 0.25]
    assert lib.ldsp_ssbbank_get_sideband(q, s.ctypes.data) == 0 and s.tolist() == [-1, -1, 1]
    assert lib.ldsp_ssbbank_destroy(q) == 0


# ---------------------------------------------------------------- errors
def test_constructor_errors(ld):
    for C_ in (0, -1, 257):
        with pytest.raises(ValueError):
            ld.SSBBank(C_, 2)
    for D in (0, -3, 33, 1000):
        with pytest.raises(ValueError):
            ld.SSBBank(3, D, lo=0.002, hi=0.01)
    for lo in (0.0, -0.025, 0.125, 0.2, 0.6, np.nan, np.inf):              # 0.125: the default hi equals lo at D = 2
        with pytest.raises(ValueError):
            ld.SSBBank(3, 2, lo=lo)
    for hi in (0.0, -0.1, 0.025, 0.01, 0.2501, 1.0, np.nan, np.inf):
        with pytest.raises(ValueError):
            ld.SSBBank(3, 2, hi=hi)
    assert ld.SSBBank(3, 2, hi=0.25).hi == 0.25
    with pytest.raises(ValueError):
        ld.SSBBank(3, 32)                             # the default hi, 0.5 / 32 - 0.025, is below lo
    for n in (0, -1, 1026):
        with pytest.raises(ValueError):
            ld.SSBBank(3, 2, ntaps=n)
    for As in (0.0, -60.0, np.nan):
        with pytest.raises(ValueError):
            ld.SSBBank(3, 2, As=As)
    for bfo in (0.51, -0.6, np.nan, np.inf, [0.0, 0.1], [0.0] * 4, [0.0, np.nan, 0.0]):
        with pytest.raises(ValueError):
            ld.SSBBank(3, 2, bfo=bfo)
    for side in ("am", "", 1, None, ["usb"], ["usb"] * 4, ["usb", "lsb", "x"]):
        with pytest.raises(ValueError):
            ld.SSBBank(3, 2, sideband=side)
    with pytest.raises(NotImplementedError):
        ld.SSBBank(3, 4, lo=0.0019)                   # default L = 2 * 527 + 1
    assert ld.SSBBank(3, 4, lo=0.0019, ntaps=1025).ntaps == 1025
    ones = np.ones(8, np.float32)
    for kw in (dict(taps=[]), dict(taps=ones, ntaps=8), dict(taps=np.ones(1026))):
        with pytest.raises(ValueError):
            ld.SSBBank(3, 2, **kw)


def test_create_codes(lib):
    nan = float("nan")
    for kw in (dict(C_=0), dict(C_=257), dict(D=0), dict(D=33), dict(lo=0.0), dict(lo=-0.1), dict(lo=0.125), dict(lo=0.3),
               dict(lo=nan), dict(hi=-0.1), dict(hi=0.025), dict(hi=0.02), dict(hi=0.26), dict(hi=nan), dict(L=1026),
               dict(As=0.0), dict(As=nan), dict(D=32), dict(bfo=[0.0, 0.6, 0.0]), dict(bfo=[nan, 0.0, 0.0]),
               dict(side=[1, 0, 1]), dict(side=[1, 1, 3])):
        assert create(lib, **kw)[0] == LDSP_EINVAL, kw
    assert create(lib, D=4, lo=0.0019)[0] == LDSP_EUNSUP
    assert create(lib, D=4, lo=0.00195)[0] == LDSP_EUNSUP
    assert create(lib, D=4, lo=0.0019, C_=0)[0] == LDSP_EINVAL            # a value out of range comes first
    assert create(lib, D=4, lo=0.0019, bfo=[0.0, 0.7, 0.0])[0] == LDSP_EINVAL
    b, s = lists(3)
    q = C.c_void_p()
    assert lib.ldsp_ssbbank_create(3, 2, 0.025, 0.0, 0, 60.0, b.ctypes.data, s.ctypes.data, None) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_create(3, 2, 0.025, 0.0, 0, 60.0, None, s.ctypes.data, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_create(3, 2, 0.025, 0.0, 0, 60.0, b.ctypes.data, None, C.byref(q)) == LDSP_EINVAL
    p = np.ones(8, np.float32)
    for kw in (dict(C_=0), dict(C_=257), dict(D=0), dict(D=33), dict(L=0), dict(L=1026), dict(lo=0.0), dict(lo=nan),
               dict(hi=0.3), dict(hi=0.01), dict(bfo=[0.0, -0.6, 0.0]), dict(side=[1, -1, 0])):
        assert create_taps(lib, p, **kw)[0] == LDSP_EINVAL, kw
    assert lib.ldsp_ssbbank_create_taps(3, 2, None, 8, 0.025, 0.0, b.ctypes.data, s.ctypes.data, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_create_taps(3, 2, p.ctypes.data, 8, 0.025, 0.0, None, s.ctypes.data, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_create_taps(3, 2, p.ctypes.data, 8, 0.025, 0.0, b.ctypes.data, None, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_create_taps(3, 2, p.ctypes.data, 8, 0.025, 0.0, b.ctypes.data, s.ctypes.data, None) == LDSP_EINVAL
    for C_, D, lo, L in ((1, 1, 0.025, 1), (256, 32, 0.002, 1025)):       # the ends of the ranges are allowed
        rc, q = create(lib, C_=C_, D=D, lo=lo, L=L)
        assert rc == 0 and lib.ldsp_ssbbank_destroy(q) == 0
    rc, q = create(lib, C_=2, D=4, lo=1 / 512)
    assert rc == 0 and info(lib, q) == (2, 4, 1025, 0)
    assert lib.ldsp_ssbbank_get_info(q, None, None, None, None) == 0
    assert lib.ldsp_ssbbank_destroy(q) == 0


def test_execute_argument_errors_need_no_gpu(lib):
    rc, q = create(lib, 3, 4)
    assert rc == 0
    x = np.zeros((3, 64), np.complex64)
    y = np.zeros((3, 20), np.float32)
    xp, yp = x.ctypes.data, y.ctypes.data
    k = C.c_size_t(0)
    assert lib.ldsp_ssbbank_execute(q, xp, 64, 64, yp, 15, C.byref(k), MEM_HOST, None) == LDSP_ERANGE
    assert k.value == 16
    assert lib.ldsp_ssbbank_execute(q, xp, 64, 64, yp, 15, None, MEM_HOST, None) == LDSP_ERANGE
    assert lib.ldsp_ssbbank_execute(q, xp, 63, 64, yp, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_execute(None, xp, 64, 64, yp, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_execute(q, None, 64, 64, yp, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_execute(q, xp, 64, 64, None, 20, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_execute(q, xp, 64, 64, yp, 20, C.byref(k), 7, None) == LDSP_EINVAL
    # the object is untouched: the same geometry as a fresh one, no input consumed
    rc, f = create(lib, 3, 4)
    assert info(lib, q) == info(lib, f) == (3, 4, 81, 0)
    assert lib.ldsp_ssbbank_num_outputs(q, 64, C.byref(k)) == 0 and k.value == 16
    assert lib.ldsp_ssbbank_num_outputs(q, 64, None) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_num_outputs(None, 64, C.byref(k)) == LDSP_EINVAL
    w = np.zeros(3, np.uint32)
    assert lib.ldsp_ssbbank_get_words(q, None) == LDSP_EINVAL and lib.ldsp_ssbbank_get_words(None, w.ctypes.data) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_get_bfo(q, None) == LDSP_EINVAL and lib.ldsp_ssbbank_get_sideband(q, None) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_get_bfo(None, w.ctypes.data) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_get_sideband(None, w.ctypes.data) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_get_taps(None, None, None) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_get_info(None, None, None, None, None) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_get_band(None, None, None) == LDSP_EINVAL
    assert lib.ldsp_ssbbank_reset(None) == LDSP_EINVAL
    assert lib.ldsp_debug_ssbbank_seek(None, 5) == LDSP_EINVAL
    assert lib.ldsp_debug_ssbbank_seek(q, 5) == 0 and info(lib, q)[3] == 3
    assert lib.ldsp_ssbbank_reset(q) == 0 and info(lib, q)[3] == 0
    assert lib.ldsp_ssbbank_destroy(q) == 0 and lib.ldsp_ssbbank_destroy(f) == 0
    assert lib.ldsp_ssbbank_destroy(None) == 0


def test_python_shape_and_dtype_errors_need_no_gpu(ld):
    sb = ld.SSBBank(3, 4)
    for bad in (np.zeros((2, 64), np.complex64), np.zeros((4, 64), np.complex64), np.zeros(64, np.complex64),
                np.zeros((3, 4, 4), np.complex64)):
        with pytest.raises(ValueError):
            sb(bad)
    for dt in (np.complex128, np.float32, np.int16):  # other numeric dtypes are cast, as the other banks': the shape decides
        with pytest.raises(ValueError):
            sb(np.zeros((2, 64), dt))
    assert sb.skip == 0
    if ld.device_count() == 0:                       # a well-formed call without a device is an error, not a fallback
        for dt in (np.complex64, np.complex128):
            with pytest.raises(RuntimeError, match="no CPU fallback"):
                sb(np.zeros((3, 64), dt))


# ---------------------------------------------------------------- the tile hook
def test_tile_hook(lib, ld):
    """128 columns per workgroup at every (D, L): the widest span, D = 32 with L = 1025, takes 48.25 KiB of LDS."""
    f = C.c_size_t()
    for D, L in ((1, 1), (1, 1025), (5, 501), (8, 363), (32, 1), (32, 1025)):
        assert lib.ldsp_debug_ssbbank_tile(D, L, C.byref(f)) == 0
        assert f.value == 128, (D, L)
        assert ld.SSBBank(1, D, lo=0.002, hi=0.015, ntaps=L).tile == 128
    assert lib.ldsp_debug_ssbbank_tile(0, 8, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_ssbbank_tile(33, 8, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_ssbbank_tile(8, 0, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_ssbbank_tile(8, 1026, C.byref(f)) == LDSP_EINVAL
    assert lib.ldsp_debug_ssbbank_tile(8, 8, None) == LDSP_EINVAL


# ---------------------------------------------------------------- the C driver under ASan + UBSan
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:")


def test_ssbbank_driver_asan_ubsan():
    """The host code of the C ABI (creation, design, the row taps, setters, getters, argument checks,
    num_outputs) in a stand-alone instrumented program; no GPU and nothing loaded into Python."""
    r = subprocess.run(["make", "-s", "-j8", "-C", PKG, "ssbbank_asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(PKG, "build", "ssbbank_driver_asan")
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the driver is not instrumented"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert not any(k in out for k in REPORTS), out[-4000:]
    assert "all checks passed" in r.stdout
