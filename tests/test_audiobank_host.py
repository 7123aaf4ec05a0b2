"""Host side of the AudioBank without a GPU (CPU suite): the exported
ldsp_audiobank_* symbols, construction, defaults and properties, every argument
error of ldsp_audiobank_create / _execute (decided before any device work), the
de-emphasis coefficients against DeemphasisFilter's, the prototype and step
against the restatement's resamp_rrrf, and the output counts over a stream cut
into calls.  The GPU side is tests/test_gpu_audiobank.py."""
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
    vp, u, f, d, sz, u32 = C.c_void_p, C.c_uint, C.c_float, C.c_double, C.c_size_t, C.c_uint32
    L.ldsp_audiobank_create.argtypes = [u, f, u, f, f, u, f, d, C.c_int, C.POINTER(vp)]
    L.ldsp_audiobank_destroy.argtypes = [vp]
    L.ldsp_audiobank_reset.argtypes = [vp]
    L.ldsp_audiobank_get_info.argtypes = [vp, C.POINTER(u), C.POINTER(u), C.POINTER(u32), C.POINTER(u32), C.POINTER(u)]
    L.ldsp_audiobank_get_taps.argtypes = [vp, vp, u, C.POINTER(u)]
    L.ldsp_audiobank_get_coefs.argtypes = [vp, C.POINTER(f), C.POINTER(f), C.POINTER(f), C.POINTER(d)]
    L.ldsp_audiobank_get_scale.argtypes = [vp, C.POINTER(f)]
    L.ldsp_audiobank_set_scale.argtypes = [vp, f]
    L.ldsp_audiobank_num_outputs.argtypes = [vp, sz, C.POINTER(sz)]
    L.ldsp_audiobank_execute.argtypes = [vp, vp, sz, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    L.ldsp_debug_audiobank_tile.argtypes = [vp, C.POINTER(sz)]
    return L


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def create(lib, C_=3, rate=0.192, m=20, fc=0.0864, As=60.0, npfb=13, sr=250e3, tau=75e-6, pcm16=0):
    q = C.c_void_p()
    return lib.ldsp_audiobank_create(C_, rate, m, fc, As, npfb, sr, tau, pcm16, C.byref(q)), q


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def default_fc(rate):
    return np.float32(0.45 * min(float(np.float32(rate)), 1.0))


# ---------------------------------------------------------------- symbols
def test_library_exports_what_the_header_declares(lib):
    with open(HEADER) as f:
        names = sorted(set(re.findall(r"\b(ldsp_(?:debug_)?audiobank_\w+)\s*\(", f.read())))
    want = {"ldsp_audiobank_" + n for n in ("create", "destroy", "reset", "get_info", "get_taps", "get_coefs",
                                            "get_scale", "set_scale", "num_outputs", "execute")}
    want.add("ldsp_debug_audiobank_tile")
    assert want <= set(names), sorted(want - set(names))
    for n in names:
        assert hasattr(lib, n), n


# ---------------------------------------------------------------- construction
def test_defaults_and_properties(ld):
    ab = ld.AudioBank(16, 0.192)
    assert (ab.nchan, ab.len, ab.nfilter, ab.phase, ab.pcm16, ab.scale) == (16, 20, 16, 0, False, 1.0)
    assert np.float32(ab.rate) == np.float32(0.192)
    assert ab.step == int(round(float(np.float32(1 << 24) / np.float32(0.192))))
    assert ab.deemphasis is None and ab.tau == 0.0
    b0, a = ab.coefs
    assert (np.float32(b0), np.float32(a)) == (np.float32(1), np.float32(0))
    assert ab.taps.dtype == np.float32 and ab.taps.shape == (2 * 20 * 16 + 1,)
    assert 1 <= ab.tile <= 256
    ab.scale = 0.25
    assert ab.scale == 0.25
    ab.reset()                                       # before the first call: nothing on the device yet
    for name in ("nchan", "rate", "len", "nfilter", "step", "phase", "taps", "deemphasis", "tau", "coefs", "pcm16",
                 "tile"):
        with pytest.raises(AttributeError):
            setattr(ab, name, getattr(ab, name))
    de = ld.AudioBank(nchan=256, rate=0.5, len=12, Fc=0.2, As=70.0, nfilter=32, deemphasis=48e3, tau=50e-6, pcm16=True)
    assert (de.nchan, de.len, de.nfilter, de.deemphasis, de.tau, de.pcm16) == (256, 12, 32, 48e3, 50e-6, True)
    assert ld.AudioBank(1, 1 / 32, 32, nfilter=128).tile < 256        # the span of 256 outputs would not fit
    assert ld.AudioBank(1, 4.0, 1, nfilter=4096).nfilter == 4096     # the ends of the ranges are allowed


@pytest.mark.parametrize("sr", [48e3, 250e3, 400e3])
def test_coefs_are_deemphasis_filters(ld, ora, sr):
    b, a = ora.deemphasis_coefs(sr)
    b0, a1 = ld.AudioBank(2, 0.5, deemphasis=sr).coefs
    assert isinstance(b0, np.float32) and isinstance(a1, np.float32)
    assert bits(b0) == bits(b[0]) and bits(a1) == bits(np.float32(-a[1]))


def test_coefs_at_another_time_constant(ld):
    b0, a = ld.AudioBank(2, 0.5, deemphasis=200e3, tau=50e-6).coefs
    want = np.float32(np.exp(-1.0 / (50e-6 * float(np.float32(200e3)))))
    assert bits(a) == bits(want) and bits(b0) == bits(np.float32(1.0 - float(want)))


@pytest.mark.parametrize("rate,m,npfb", [(0.192, 20, 13), (0.12, 32, 16), (1 / 32, 7, 64), (1.0, 20, 13), (2.5, 4, 16)])
def test_design_is_the_restatements(ld, ora, rate, m, npfb):
    ab = ld.AudioBank(2, rate, m, nfilter=npfb)
    ref = ora.Resampler(rate, m, default_fc(rate), 60.0, npfb, cplx=False)
    assert ab.nfilter == ref.npfb and ab.step == ref.step and ab.phase == ref.phase == 0
    assert ab.taps.shape == ref.prototype.shape and (bits(ab.taps) == bits(ref.prototype)).all()
    rr = ora.Resampler(rate, m, 0.3, 80.0, npfb, cplx=False)
    ab = ld.AudioBank(2, rate, m, Fc=0.3, As=80.0, nfilter=npfb, deemphasis=100e3)
    assert (bits(ab.taps) == bits(rr.prototype)).all()


@pytest.mark.parametrize("rate", [0.192, 1 / 32, 2.5])
def test_num_outputs_over_a_cut_stream(ld, ora, rate):
    """The restatement steps through the stream; the bank can follow it only where a device is
    present, and answers for the start of the stream (phase 0) otherwise."""
    ab = ld.AudioBank(2, rate, 7, nfilter=16)
    fresh = lambda: ora.Resampler(rate, 7, default_fc(rate), 60.0, 16, cplx=False)
    ref = fresh()
    for K in (0, 1, 3, 1000, 4097, 1, 0, 3):
        if ld.device_count() == 0:
            assert ab.num_outputs(K) == len(fresh()(np.zeros(K, np.float32)))
            continue
        want = len(ref(np.zeros(K, np.float32)))
        assert ab.num_outputs(K) == want
        y = ab(np.zeros((2, K), np.float32))
        assert y.shape == (2, want) and ab.phase == ref.phase


# ---------------------------------------------------------------- errors
def test_constructor_errors(ld):
    for kw in (dict(nchan=0), dict(nchan=-1), dict(nchan=257), dict(rate=0.0), dict(rate=-0.5), dict(rate=np.nan),
               dict(len=0), dict(len=-2), dict(Fc=0.0), dict(Fc=0.5), dict(Fc=-0.1), dict(As=0.0), dict(As=-60.0),
               dict(nfilter=0), dict(nfilter=-4), dict(deemphasis=250e3, tau=0.0), dict(deemphasis=250e3, tau=-75e-6),
               dict(deemphasis=0.0), dict(deemphasis=-48e3)):
        with pytest.raises(ValueError):
            ld.AudioBank(**{"nchan": 3, "rate": 0.192, **kw})
    for kw in (dict(rate=1 / 33), dict(rate=4.01), dict(len=33), dict(len=32, nfilter=129), dict(len=1, nfilter=4097),
               dict(deemphasis=427e3), dict(deemphasis=250e3, tau=129e-6)):
        with pytest.raises(NotImplementedError):
            ld.AudioBank(**{"nchan": 3, "rate": 0.192, **kw})
    ld.AudioBank(3, 0.192, deemphasis=426e3)         # 31.95 samples
    ld.AudioBank(3, 0.192, tau=0.0)                  # no de-emphasis: tau is not looked at


def test_create_codes(lib):
    for kw in (dict(C_=0), dict(C_=257), dict(rate=0.0), dict(rate=-1.0), dict(rate=float("nan")), dict(m=0),
               dict(fc=0.0), dict(fc=0.5), dict(As=0.0), dict(npfb=0), dict(tau=0.0), dict(tau=-1e-6)):
        assert create(lib, **kw)[0] == LDSP_EINVAL, kw
    for kw in (dict(rate=0.03), dict(rate=4.5), dict(m=33), dict(m=32, npfb=129), dict(m=1, npfb=4097),
               dict(sr=427e3), dict(tau=129e-6)):
        assert create(lib, **kw)[0] == LDSP_EUNSUP, kw
    assert lib.ldsp_audiobank_create(3, 0.192, 20, 0.0864, 60.0, 13, 250e3, 75e-6, 0, None) == LDSP_EINVAL
    for kw in (dict(C_=1, rate=1 / 32), dict(C_=256, rate=4.0), dict(m=32, npfb=128), dict(m=1, npfb=4096),
               dict(sr=0.0, tau=0.0), dict(sr=-1.0, tau=-1.0), dict(pcm16=1)):
        rc, q = create(lib, **kw)
        assert rc == 0, (kw, lib.ldsp_last_error())
        assert lib.ldsp_audiobank_destroy(q) == 0


def test_getters_and_execute_argument_errors_need_no_gpu(lib, ora):
    rc, q = create(lib)
    assert rc == 0
    c, npfb, sub = C.c_uint(), C.c_uint(), C.c_uint()
    step, phase = C.c_uint32(), C.c_uint32(7)
    assert lib.ldsp_audiobank_get_info(q, C.byref(c), C.byref(npfb), C.byref(step), C.byref(phase), C.byref(sub)) == 0
    assert (c.value, npfb.value, phase.value, sub.value) == (3, 16, 0, 40)
    assert lib.ldsp_audiobank_get_info(q, None, None, None, None, None) == 0
    n = C.c_uint()
    assert lib.ldsp_audiobank_get_taps(q, None, 0, C.byref(n)) == 0 and n.value == 641
    h = np.zeros(641, np.float32)
    assert lib.ldsp_audiobank_get_taps(q, h.ctypes.data, 640, None) == LDSP_EINVAL
    assert lib.ldsp_audiobank_get_taps(q, h.ctypes.data, 641, None) == 0
    assert (bits(h) == bits(ora.Resampler(0.192, 20, 0.0864, 60.0, 13, cplx=False).prototype)).all()
    b0, a, sr, tau = C.c_float(), C.c_float(), C.c_float(), C.c_double()
    assert lib.ldsp_audiobank_get_coefs(q, C.byref(b0), C.byref(a), C.byref(sr), C.byref(tau)) == 0
    b, aa = ora.deemphasis_coefs(250e3)
    assert (np.float32(b0.value), np.float32(a.value), sr.value, tau.value) == (b[0], -aa[1], 250e3, 75e-6)
    assert lib.ldsp_audiobank_get_coefs(q, None, None, None, None) == 0
    s = C.c_float()
    assert lib.ldsp_audiobank_get_scale(q, C.byref(s)) == 0 and s.value == 1.0
    assert lib.ldsp_audiobank_set_scale(q, 0.5) == 0
    assert lib.ldsp_audiobank_get_scale(q, C.byref(s)) == 0 and s.value == 0.5
    assert lib.ldsp_audiobank_get_scale(q, None) == LDSP_EINVAL
    t = C.c_size_t()
    assert lib.ldsp_debug_audiobank_tile(q, C.byref(t)) == 0 and t.value == 256
    assert lib.ldsp_debug_audiobank_tile(q, None) == LDSP_EINVAL
    assert lib.ldsp_debug_audiobank_tile(None, C.byref(t)) == LDSP_EINVAL

    x = np.zeros((3, 100), np.float32)
    y = np.zeros((3, 32), np.float32)
    xp, yp = x.ctypes.data, y.ctypes.data
    k = C.c_size_t(0)
    assert lib.ldsp_audiobank_num_outputs(q, 100, C.byref(k)) == 0 and k.value == 20
    assert lib.ldsp_audiobank_num_outputs(q, 100, None) == LDSP_EINVAL
    assert lib.ldsp_audiobank_num_outputs(None, 100, C.byref(k)) == LDSP_EINVAL
    k.value = 0
    assert lib.ldsp_audiobank_execute(q, xp, 100, 100, yp, 19, C.byref(k), MEM_HOST, None) == LDSP_ERANGE
    assert k.value == 20
    assert lib.ldsp_audiobank_execute(q, xp, 100, 100, yp, 19, None, MEM_HOST, None) == LDSP_ERANGE
    assert lib.ldsp_audiobank_execute(q, xp, 99, 100, yp, 32, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_audiobank_execute(None, xp, 100, 100, yp, 32, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_audiobank_execute(q, None, 100, 100, yp, 32, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_audiobank_execute(q, xp, 100, 100, None, 32, C.byref(k), MEM_HOST, None) == LDSP_EINVAL
    assert lib.ldsp_audiobank_execute(q, xp, 100, 100, yp, 32, C.byref(k), 7, None) == LDSP_EINVAL
    # nothing was consumed: the schedule is where it was
    assert lib.ldsp_audiobank_get_info(q, None, None, None, C.byref(phase), None) == 0 and phase.value == 0
    assert lib.ldsp_audiobank_num_outputs(q, 100, C.byref(k)) == 0 and k.value == 20
    assert lib.ldsp_audiobank_reset(None) == LDSP_EINVAL
    assert lib.ldsp_audiobank_reset(q) == 0
    assert lib.ldsp_audiobank_destroy(q) == 0
    assert lib.ldsp_audiobank_destroy(None) == 0


def test_python_shape_errors_need_no_gpu(ld):
    ab = ld.AudioBank(3, 0.192)
    for bad in (np.zeros((2, 64), np.float32), np.zeros((4, 64), np.float32), np.zeros(64, np.float32),
                np.zeros((3, 4, 4), np.float32)):
        with pytest.raises(ValueError):
            ab(bad)
    assert ab.phase == 0


def test_call_raises_without_gpu(ld):
    if ld.device_count() > 0:
        pytest.skip("a GPU is present")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ld.AudioBank(2, 0.192, deemphasis=250e3)(np.zeros((2, 64), np.float32))
