"""Host side of the AGCBank without a GPU (CPU suite): the exported ldsp_agcbank_* symbols,
defaults and get_info, the dB -> unit conversion bit for bit, num_outputs (tracked and
emitted blocks) against the closed form over ragged call sequences, every argument error
of create and execute (decided before any device work), execute without a device, the
tracker's partitioned evaluation (csrc/agc_track.hpp through ldsp_debug_agcbank_track, the
code the kernel runs per lane, wave and pass) against the serial recurrence and the closed
form in numpy, exactly, and the stand-alone C driver of the same host code under ASan +
UBSan (tests/sanitize/agcbank_driver.c).  The GPU side is tests/test_gpu_agcbank.py."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import agcbank_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "python-liquiddsp_amd")
LIBPATH = os.path.join(PKG, "libldsp.so")
HEADER = os.path.join(REPO, "include", "ldsp.h")

LDSP_EINVAL, LDSP_EHIP, LDSP_ERANGE = -1, -3, -4
MEM_HOST = 0


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIBPATH):
        pytest.fail("libldsp.so not built (run __graft_entry__.build())")
    L = C.CDLL(LIBPATH)
    L.ldsp_last_error.restype = C.c_char_p
    vp, u, d, sz, i64 = C.c_void_p, C.c_uint, C.c_double, C.c_size_t, C.c_int64
    L.ldsp_agcbank_create.argtypes = [u, u, vp, u, d, u, d, C.c_int, C.POINTER(vp)]
    L.ldsp_agcbank_destroy.argtypes = [vp]
    L.ldsp_agcbank_reset.argtypes = [vp]
    L.ldsp_agcbank_get_info.argtypes = [vp, C.POINTER(u), C.POINTER(u), C.POINTER(u), C.POINTER(d), C.POINTER(d), vp,
                                        C.POINTER(C.c_int), C.POINTER(u)]
    L.ldsp_agcbank_num_outputs.argtypes = [vp, sz, C.POINTER(sz), C.POINTER(sz)]
    L.ldsp_agcbank_execute.argtypes = [vp, vp, sz, sz, vp, sz, vp, vp, sz, C.POINTER(sz), C.c_int, vp]
    L.ldsp_agcbank_get_state.argtypes = [vp, vp, vp, vp]
    L.ldsp_debug_agcbank_units.argtypes = [d, C.POINTER(i64)]
    L.ldsp_debug_agcbank_track.argtypes = [vp, sz, u, i64, sz, vp, vp, vp]
    return L


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def create(lib, C_=3, B=256, target=-12.0, max_gain=60.0, hang=8, decay=0.5, cplx=0, ntarget=None):
    t = np.atleast_1d(np.asarray(target, np.float64))
    q = C.c_void_p()
    rc = lib.ldsp_agcbank_create(C_, B, t.ctypes.data, t.size if ntarget is None else ntarget, max_gain, hang, decay, cplx,
                                 C.byref(q))
    return rc, q


def info(lib, q, C_):
    c, b, h, cx, f = C.c_uint(), C.c_uint(), C.c_uint(), C.c_int(), C.c_uint()
    dec, mg = C.c_double(), C.c_double()
    t = np.full(C_, np.nan)
    assert lib.ldsp_agcbank_get_info(q, C.byref(c), C.byref(b), C.byref(h), C.byref(dec), C.byref(mg), t.ctypes.data,
                                     C.byref(cx), C.byref(f)) == 0
    return c.value, b.value, h.value, dec.value, mg.value, t.tolist(), cx.value, f.value


# ---------------------------------------------------------------- symbols
def test_library_exports_what_the_header_declares(lib):
    with open(HEADER) as f:
        names = sorted(set(re.findall(r"\b(ldsp_(?:debug_)?agcbank_\w+)\s*\(", f.read())))
    want = {"ldsp_agcbank_create", "ldsp_agcbank_destroy", "ldsp_agcbank_reset", "ldsp_agcbank_get_info",
            "ldsp_agcbank_num_outputs", "ldsp_agcbank_execute", "ldsp_agcbank_get_state", "ldsp_debug_agcbank_units",
            "ldsp_debug_agcbank_track"}
    assert want == set(names), sorted(want ^ set(names))
    for n in names:
        assert hasattr(lib, n), n
    out = subprocess.run(["nm", "-D", "--defined-only", LIBPATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(ldsp_(?:debug_)?agcbank_\w+)\b", out))
    assert exported == want, sorted(exported ^ want)


# ---------------------------------------------------------------- construction
def test_defaults_and_info(ld, lib):
    ag = ld.AGCBank(16)
    assert (ag.nchan, ag.block, ag.hang, ag.decay, ag.max_gain, ag.complex, ag.fill) == (16, 256, 8, 0.5, 60.0, False, 0)
    assert ag.target.dtype == np.float64 and ag.target.tolist() == [-12.0] * 16
    assert ag.peak_q is None and ag.gain_q is None and ag.gain_db is None
    level, peaks, gains = ag.state                    # before the first call: the initial state
    assert level.dtype == np.int32 and (level == M.FLOOR).all() and level.shape == (16,)
    assert peaks.shape == (16, 8) and (peaks == M.FLOOR).all()
    assert gains.dtype == np.float32 and gains.shape == (16, 2) and (gains == 0).all()
    ag.reset()                                        # nothing on the device yet
    kw = ld.AGCBank(nchan=3, block=100, target=[-6.0, -12.0, 0.0], max_gain=40.0, hang=0, decay=0.0, complex=True)
    assert (kw.nchan, kw.block, kw.hang, kw.decay, kw.max_gain, kw.complex) == (3, 100, 0, 0.0, 40.0, True)
    assert kw.target.tolist() == [-6.0, -12.0, 0.0] and kw.state[1].shape == (3, 0)
    for C_, B, H in ((1, 16, 0), (256, 4096, 255)):   # the ends of the ranges are allowed
        rc, q = create(lib, C_, B, hang=H, decay=1e4)
        assert rc == 0, lib.ldsp_last_error()
        assert info(lib, q, C_) == (C_, B, H, 1e4, 60.0, [-12.0] * C_, 0, 0)
        assert lib.ldsp_agcbank_get_info(q, None, None, None, None, None, None, None, None) == 0
        assert lib.ldsp_agcbank_destroy(q) == 0
    rc, q = create(lib, 2, 64, target=[-3.0, 3.0], cplx=1)
    assert rc == 0 and info(lib, q, 2) == (2, 64, 8, 0.5, 60.0, [-3.0, 3.0], 1, 0)
    lv, pk, gn = np.zeros(2, np.int32), np.zeros((2, 8), np.int32), np.ones((2, 2), np.float32)
    assert lib.ldsp_agcbank_get_state(q, lv.ctypes.data, pk.ctypes.data, gn.ctypes.data) == 0
    assert (lv == M.FLOOR).all() and (pk == M.FLOOR).all() and (gn == 0).all()
    assert lib.ldsp_agcbank_get_state(q, None, None, None) == 0
    assert lib.ldsp_agcbank_get_state(None, None, None, None) == LDSP_EINVAL
    assert lib.ldsp_agcbank_destroy(q) == 0


def test_units_bit_for_bit(lib):
    rng = np.random.default_rng(3)
    vals = [0.0, -0.0, 0.5, -0.5, 1.0, 3.0, 6.0, -6.0, -12.0, 30.0, 60.0, 0.01, 0.1, 0.25, 20 * np.log10(2.0),
            10 * np.log10(2.0), 180.0, -180.0, 385.3, 1e-7, 3.5885e-7 / 2, 3.5885e-7 * 1.5, 1e9, -1e9]
    vals += rng.uniform(-200, 200, 200).tolist()
    u = C.c_int64()
    for v in vals:
        assert lib.ldsp_debug_agcbank_units(v, C.byref(u)) == 0
        assert u.value == M.units(v), v
    assert M.units(20 * np.log10(2.0)) == 1 << 24
    for bad in (np.nan, np.inf, -np.inf, 2e9):
        assert lib.ldsp_debug_agcbank_units(bad, C.byref(u)) == LDSP_EINVAL
    assert lib.ldsp_debug_agcbank_units(1.0, None) == LDSP_EINVAL


# ---------------------------------------------------------------- the block schedule
@pytest.mark.parametrize("B", [16, 100, 4096])
def test_num_outputs_over_ragged_calls(ld, lib, B):
    """Stepping the stream needs a device; without one only the fresh object's counts are checked,
    for every K of the sequence."""
    ag = ld.AGCBank(2, B)
    rng = np.random.default_rng(B)
    lens = [0, 1, B - 1, B, 2 * B, 0, B - 1, 1, 3 * B + 2] + [int(v) for v in rng.integers(0, 3 * B, 8)]
    rc, q = create(lib, 2, B)
    assert rc == 0
    nt, ne = C.c_size_t(), C.c_size_t()
    T = 0
    for K in lens:
        for k in (0, 1, B - 1, B, B + 1, 2 * B, 2 * B + 1, K):
            t0, e0 = M.counts(T, B)
            t1, e1 = M.counts(T + k, B)
            assert ag.num_outputs(k) == (e1 - e0) * B, (T, k)
            if T == 0:
                assert lib.ldsp_agcbank_num_outputs(q, k, C.byref(nt), C.byref(ne)) == 0
                assert (nt.value, ne.value) == (t1, e1)
        if ld.device_count() == 0:
            break
        y = ag(np.zeros((2, K), np.float32))
        t0, e0 = M.counts(T, B)
        T += K
        t1, e1 = M.counts(T, B)
        assert y.shape == (2, (e1 - e0) * B) and ag.peak_q.shape == ag.gain_q.shape == (2, t1 - t0)
        assert ag.fill == T - e1 * B
    assert lib.ldsp_agcbank_num_outputs(q, 5, C.byref(nt), None) == 0
    assert lib.ldsp_agcbank_num_outputs(q, 5, None, C.byref(ne)) == 0
    assert lib.ldsp_agcbank_num_outputs(q, 5, None, None) == LDSP_EINVAL
    assert lib.ldsp_agcbank_num_outputs(None, 5, C.byref(nt), C.byref(ne)) == LDSP_EINVAL
    assert lib.ldsp_agcbank_destroy(q) == 0


# ---------------------------------------------------------------- errors
def test_create_codes(lib):
    nan, inf = float("nan"), float("inf")
    for kw in (dict(C_=0), dict(C_=257), dict(B=15), dict(B=4097), dict(B=0), dict(hang=256), dict(hang=1 << 20),
               dict(decay=-0.1), dict(decay=nan), dict(decay=inf), dict(max_gain=nan), dict(max_gain=inf),
               dict(max_gain=181.0), dict(max_gain=-181.0), dict(target=nan), dict(target=-inf), dict(target=200.0),
               dict(target=[-12.0, -12.0]), dict(target=[-12.0] * 4), dict(target=[-12.0, nan, -12.0]),
               dict(ntarget=0), dict(cplx=2), dict(cplx=-1)):
        rc, q = create(lib, **kw)
        assert rc == LDSP_EINVAL, kw
        assert lib.ldsp_last_error(), kw
    t = np.array([-12.0])
    q = C.c_void_p()
    assert lib.ldsp_agcbank_create(3, 256, t.ctypes.data, 1, 60.0, 8, 0.5, 0, None) == LDSP_EINVAL
    assert lib.ldsp_agcbank_create(3, 256, None, 1, 60.0, 8, 0.5, 0, C.byref(q)) == LDSP_EINVAL
    assert lib.ldsp_agcbank_reset(None) == LDSP_EINVAL
    assert lib.ldsp_agcbank_get_info(None, None, None, None, None, None, None, None, None) == LDSP_EINVAL
    assert lib.ldsp_agcbank_destroy(None) == 0


def test_constructor_errors(ld):
    for kw in (dict(nchan=0), dict(nchan=-1), dict(nchan=257), dict(block=15), dict(block=-16), dict(block=4097),
               dict(hang=-1), dict(hang=256), dict(decay=-1.0), dict(decay=np.nan), dict(max_gain=np.inf),
               dict(target=np.nan), dict(target=[]), dict(target=[-12.0, -6.0]), dict(target=[-12.0] * 4)):
        args = dict(nchan=3)
        args.update(kw)
        with pytest.raises(ValueError):
            ld.AGCBank(**args)
    ag = ld.AGCBank(3)
    for name in ("nchan", "block", "hang", "decay", "max_gain", "target", "fill", "state", "peak_q", "gain_q", "gain_db"):
        with pytest.raises(AttributeError):
            setattr(ag, name, 1)
    for bad in (np.zeros((2, 64), np.float32), np.zeros((4, 64), np.float32), np.zeros(64, np.float32),
                np.zeros((3, 4, 4), np.float32)):
        with pytest.raises(ValueError):
            ag(bad)
    assert ag.fill == 0


def test_execute_argument_errors_need_no_gpu(lib, ld):
    rc, q = create(lib, 3, 16)
    assert rc == 0
    x = np.zeros((3, 64), np.float32)
    y = np.zeros((3, 48), np.float32)
    pq, gq = np.zeros((3, 4), np.int32), np.zeros((3, 4), np.int32)
    xp, yp, pp, gp = x.ctypes.data, y.ctypes.data, pq.ctypes.data, gq.ctypes.data
    nw = C.c_size_t(0)
    ex = lib.ldsp_agcbank_execute
    for args, code in (((q, xp, 64, 64, yp, 47, pp, gp, 4, C.byref(nw), MEM_HOST, None), LDSP_ERANGE),
                       ((q, xp, 64, 64, yp, 48, pp, gp, 3, C.byref(nw), MEM_HOST, None), LDSP_ERANGE),
                       ((q, xp, 64, 64, yp, 47, pp, gp, 4, None, MEM_HOST, None), LDSP_ERANGE),
                       ((q, xp, 63, 64, yp, 48, pp, gp, 4, C.byref(nw), MEM_HOST, None), LDSP_EINVAL),
                       ((None, xp, 64, 64, yp, 48, pp, gp, 4, C.byref(nw), MEM_HOST, None), LDSP_EINVAL),
                       ((q, None, 64, 64, yp, 48, pp, gp, 4, C.byref(nw), MEM_HOST, None), LDSP_EINVAL),
                       ((q, xp, 64, 64, None, 48, pp, gp, 4, C.byref(nw), MEM_HOST, None), LDSP_EINVAL),
                       ((q, xp, 64, 64, yp, 48, None, gp, 4, C.byref(nw), MEM_HOST, None), LDSP_EINVAL),
                       ((q, xp, 64, 64, yp, 48, pp, None, 4, C.byref(nw), MEM_HOST, None), LDSP_EINVAL),
                       ((q, xp, 64, 64, yp, 48, pp, gp, 4, C.byref(nw), 7, None), LDSP_EINVAL)):
        nw.value = 0
        assert ex(*args) == code, args
        assert lib.ldsp_last_error()
        if args[0] is not None and args[9] is not None:
            assert nw.value == 48
    # the object is untouched: no input consumed
    assert info(lib, q, 3)[-1] == 0
    nt, ne = C.c_size_t(), C.c_size_t()
    assert lib.ldsp_agcbank_num_outputs(q, 64, C.byref(nt), C.byref(ne)) == 0 and (nt.value, ne.value) == (4, 3)
    rc = ex(q, xp, 64, 64, yp, 48, pp, gp, 4, C.byref(nw), MEM_HOST, None)
    if ld.device_count() == 0:                        # a well-formed call without a device is an error, not a fallback
        assert rc == LDSP_EHIP and lib.ldsp_last_error()
        assert info(lib, q, 3)[-1] == 0
        with pytest.raises(RuntimeError):
            ld.AGCBank(3, 16)(x)
    else:
        assert rc == 0 and nw.value == 48 and info(lib, q, 3)[-1] == 16
    assert lib.ldsp_agcbank_reset(q) == 0 and info(lib, q, 3)[-1] == 0
    assert lib.ldsp_agcbank_destroy(q) == 0


# ---------------------------------------------------------------- the tracker
def run_track(lib, pq, H, d, width, cuts):
    """The stream cut at `cuts`, each piece through the hook with the carried level and peaks."""
    pq = np.ascontiguousarray(pq, np.int32)
    level = np.array([M.FLOOR], np.int32)
    tail = np.full(max(H, 1), M.FLOOR, np.int32)
    out = np.empty(pq.size, np.int32)
    edges = [0] + list(cuts) + [pq.size]
    for a, b in zip(edges[:-1], edges[1:]):
        piece = np.ascontiguousarray(pq[a:b])
        L = np.empty(max(b - a, 1), np.int32)
        rc = lib.ldsp_debug_agcbank_track(piece.ctypes.data, b - a, H, d, width, level.ctypes.data, tail.ctypes.data,
                                          L.ctypes.data)
        assert rc == 0, lib.ldsp_last_error()
        out[a:b] = L[:b - a]
    return out, int(level[0]), tail[:H]


DECAYS = [0, 1, M.units(0.5), M.units(30.0)]


@pytest.mark.parametrize("H", [0, 1, 7, 255])
@pytest.mark.parametrize("d", DECAYS)
def test_partitioned_tracker_is_exact(lib, H, d):
    rng = np.random.default_rng(1000 * H + d % 997)
    n = 700
    burst = np.full(n, M.FLOOR, np.int64)
    burst[0] = M.CEIL                                  # the decay crosses every partition
    rand = rng.integers(-30 * M.Q, 2 * M.Q, n)
    rand[rng.random(n) < 0.7] -= 20 * M.Q              # mostly quiet, with bursts
    sparse = np.where(rng.random(n) < 0.02, rng.integers(-10 * M.Q, 0, n), M.FLOOR)
    edge = np.array([M.CEIL, M.FLOOR, M.CEIL, M.CEIL, M.FLOOR] * (n // 5), np.int64)
    for name, pq in (("burst", burst), ("random", rand), ("sparse", sparse), ("edge", edge)):
        serial = M.track_serial(pq, H, d)[0]
        closed = M.track_closed(pq, H, d)[0]
        assert (serial == closed).all(), name          # the two forms of the definition agree
        for width in (1, 3, 64, 257):
            cuts = sorted(int(v) for v in rng.integers(0, n + 1, 6)) + [n]    # an empty last call too
            got, level, tail = run_track(lib, pq, H, d, width, cuts)
            assert (got == serial).all(), (name, width, int(np.argmax(got != serial)))
            assert level == serial[-1]
            assert (tail == np.concatenate([np.full(H, M.FLOOR), pq])[pq.size:]).all()
    if d == 1:
        assert serial.min() >= M.FLOOR and M.track_serial(burst, H, d)[0, -1] == M.CEIL - (n - 1 - H)


def test_tracker_hook_errors(lib):
    pq = np.zeros(8, np.int32)
    lv, tl, L = np.array([M.FLOOR], np.int32), np.full(4, M.FLOOR, np.int32), np.zeros(8, np.int32)
    f = lib.ldsp_debug_agcbank_track
    ok = (pq.ctypes.data, 8, 4, 5, 3, lv.ctypes.data, tl.ctypes.data, L.ctypes.data)
    assert f(*ok) == 0
    for i, bad in ((0, None), (2, 256), (3, -1), (3, (1 << 31) + 1), (4, 0), (5, None), (6, None), (7, None)):
        args = list(ok)
        args[i] = bad
        assert f(*args) == LDSP_EINVAL, i
    hi = np.full(8, M.CEIL + 1, np.int32)
    assert f(hi.ctypes.data, 8, 4, 5, 3, lv.ctypes.data, tl.ctypes.data, L.ctypes.data) == LDSP_EINVAL
    assert f(None, 0, 0, 5, 3, lv.ctypes.data, None, None) == 0          # nothing to track


# ---------------------------------------------------------------- the C driver under ASan + UBSan
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:")


def test_agcbank_driver_asan_ubsan():
    """The host code of the C ABI (creation, getters, argument checks, num_outputs, the no-device
    execute path, the partitioned tracker) in a stand-alone instrumented program; no GPU and
    nothing loaded into Python."""
    r = subprocess.run(["make", "-s", "-j8", "-C", PKG, "agcbank_asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(PKG, "build", "agcbank_driver_asan")
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the driver is not instrumented"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert not any(k in out for k in REPORTS), out[-4000:]
    assert "all checks passed" in r.stdout
