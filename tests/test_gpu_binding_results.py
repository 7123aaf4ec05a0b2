"""What the Python binding hands back, for every registered class and module
function that takes samples: one table, each entry called once with a numpy
input and once with the same data as a device tensor, on fresh objects.  Both
results must have the type (numpy array / torch tensor), dtype, shape, device,
contiguity and memory kind the binding has always chosen, and the same bits.
Sizes are small and odd: 4 099 samples (no multiple of a tile or a decimation)
and [4, 1 031] row images.  The device-only paths of the row images (strided
views) have their own cases; the messages that need no device are in
tests/test_binding_errors_host.py, the device-mismatch ones in
tests/test_gpu_dist.py."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, ROWS, K = 4099, 4, 1031
c64, f32, i16 = np.complex64, np.float32, np.int16
H = np.hanning(31).astype(f32)
B2, A2 = [0.2, 0.3, 0.2], [1.0, -0.4, 0.1]


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


@pytest.fixture(scope="module")
def torch():
    import torch
    return torch


@pytest.fixture(scope="module")
def data():
    rng = np.random.default_rng(2024)
    c = (0.3 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))).astype(c64)
    rows = (0.3 * (rng.standard_normal((ROWS, K)) + 1j * rng.standard_normal((ROWS, K)))).astype(c64)
    d = {"c": c, "f": np.ascontiguousarray(c.real), "f_even": np.ascontiguousarray(c.real[:N - 1]),   # decim: pairs
         "raw": rng.integers(-2000, 2000, 2 * N).astype(i16),
         "rows_c": rows, "rows_f": np.ascontiguousarray(rows.real)}
    for v in d.values():
        v.setflags(write=False)
    return d


def chan_cols(L):
    return L.Channelizer(4).num_outputs(N)


def ddc(L):
    return L.Downconverter([0.1, -0.2, 0.3], 5)


def spg_rows(L):
    return L.Spectrogram(256).num_outputs(N)[1]


# (id, input, result dtype, result shape (a tuple, a function of the module, or None: whatever num_outputs gave), call)
CASES = [
    ("RealFIRFilter", "f", f32, (N,), lambda L, x: L.RealFIRFilter(H)(x)),
    ("ComplexFIRFilter", "c", c64, (N,), lambda L, x: L.ComplexFIRFilter(H)(x)),
    ("RealDCBlocker", "f", f32, (N,), lambda L, x: L.RealDCBlocker(7)(x)),
    ("RealKaiserBessel", "f", f32, (N,), lambda L, x: L.RealKaiserBessel(25, 0.2)(x)),
    ("CIIRFilter", "c", c64, (N,), lambda L, x: L.CIIRFilter(B2, A2)(x)),
    ("RIIRFilter", "f", f32, (N,), lambda L, x: L.RIIRFilter(B2, A2)(x)),
    ("CLowpassIIR", "c", c64, (N,), lambda L, x: L.CLowpassIIR("butter", 4, 0.1)(x)),
    ("CHighpassIIR", "c", c64, (N,), lambda L, x: L.CHighpassIIR("butter", 4, 0.1)(x)),
    ("CBandpassIIR", "c", c64, (N,), lambda L, x: L.CBandpassIIR("butter", 2, 0.1, 0.2)(x)),
    ("CBandstopIIR", "c", c64, (N,), lambda L, x: L.CBandstopIIR("butter", 2, 0.1, 0.2)(x)),
    ("RLowpassIIR", "f", f32, (N,), lambda L, x: L.RLowpassIIR("butter", 4, 0.1)(x)),
    ("RHighpassIIR", "f", f32, (N,), lambda L, x: L.RHighpassIIR("butter", 4, 0.1)(x)),
    ("RBandpassIIR", "f", f32, (N,), lambda L, x: L.RBandpassIIR("butter", 2, 0.1, 0.2)(x)),
    ("RBandstopIIR", "f", f32, (N,), lambda L, x: L.RBandstopIIR("butter", 2, 0.1, 0.2)(x)),
    ("ComplexIIRFilter", "c", c64, (N,), lambda L, x: L.ComplexIIRFilter("cheby2", order=8, Fc=0.05)(x)),
    ("RealIIRFilter", "f", f32, (N,), lambda L, x: L.RealIIRFilter()(x)),
    ("ComplexIIRFilter.from_bytes", "raw", c64, (N,), lambda L, x: L.ComplexIIRFilter().from_bytes(x)),
    ("DeemphasisFilter", "f", f32, (N,), lambda L, x: L.DeemphasisFilter(48000)(x)),
    ("NCO", "c", c64, (N,), lambda L, x: nco(L)(x)),
    ("NCO.mix_up", "c", c64, (N,), lambda L, x: nco(L).mix_up(x)),
    ("NCO.mix_down", "c", c64, (N,), lambda L, x: nco(L).mix_down(x)),
    ("AGC", "c", c64, (N,), lambda L, x: L.AGC()(x)),
    ("AmpModem", "c", f32, (N,), lambda L, x: L.AmpModem(0.5, "dsb", True)(x)),
    ("BroadcastAM", "c", f32, (N,), lambda L, x: L.BroadcastAM()(x)),
    ("FreqDem", "c", f32, (N,), lambda L, x: L.FreqDem(0.25)(x)),
    ("FMStereo", "c", f32, None, lambda L, x: L.FMStereo(600000.0, 48000.0)(x)),
    ("Delay[c64]", "c", c64, (N,), lambda L, x: L.Delay(5)(x)),
    ("Delay[f32]", "f", f32, (N,), lambda L, x: L.Delay(5)(x)),
    ("SSBDemod[usb]", "c", f32, (N,), lambda L, x: L.SSBDemod("usb")(x)),
    ("SSBDemod[lsb]", "c", f32, (N,), lambda L, x: L.SSBDemod("lsb")(x)),
    ("HilbertTransform[c64]", "c", f32, (2 * N,), lambda L, x: L.HilbertTransform()(x)),
    ("HilbertTransform[f32]", "f_even", c64, (N // 2,), lambda L, x: L.HilbertTransform()(x)),
    ("HilbertTransform.interp", "c", f32, (2 * N,), lambda L, x: L.HilbertTransform().interp(x)),
    ("HilbertTransform.decim", "f_even", c64, (N // 2,), lambda L, x: L.HilbertTransform().decim(x)),
    ("HilbertTransform.r2c", "f", c64, (N,), lambda L, x: L.HilbertTransform().r2c(x)),
    ("HilbertTransform.c2r", "c", f32, (N,), lambda L, x: L.HilbertTransform().c2r(x)),
    ("RResampler", "f", f32, None, lambda L, x: L.RResampler(0.37)(x)),
    ("CResampler", "c", c64, None, lambda L, x: L.CResampler(0.37)(x)),
    ("RealResampler", "f", f32, None, lambda L, x: L.RealResampler(1.7, Fc=0.2)(x)),
    ("ComplexResampler", "c", c64, None, lambda L, x: L.ComplexResampler(0.024, Fc=0.024)(x)),
    ("mix_down_filter", "c", c64, (N,), lambda L, x: L.mix_down_filter(nco(L), L.ComplexFIRFilter(H), x)),
    ("mix_up_filter", "c", c64, (N,), lambda L, x: L.mix_up_filter(nco(L), L.ComplexFIRFilter(H), x)),
    ("filter_resample[c64]", "c", c64, None,
     lambda L, x: L.filter_resample(L.ComplexIIRFilter(), L.ComplexResampler(0.37, Fc=0.2), x)),
    ("filter_resample[f32]", "f", f32, None,
     lambda L, x: L.filter_resample(L.RealIIRFilter(), L.RealResampler(0.37, Fc=0.2), x)),
    ("bytes_to_iq", "raw", c64, (N,), lambda L, x: L.bytes_to_iq(x)),
    ("Channelizer", "c", c64, lambda L: (4, chan_cols(L)), lambda L, x: L.Channelizer(4)(x)),
    ("Channelizer.from_bytes", "raw", c64, lambda L: (4, chan_cols(L)), lambda L, x: L.Channelizer(4).from_bytes(x)),
    ("Downconverter", "c", c64, lambda L: (3, ddc(L).num_outputs(N)), lambda L, x: ddc(L)(x)),
    ("Downconverter.from_bytes", "raw", c64, lambda L: (3, ddc(L).num_outputs(N)), lambda L, x: ddc(L).from_bytes(x)),
    ("Spectrogram", "c", f32, lambda L: (spg_rows(L), 256), lambda L, x: L.Spectrogram(256)(x)),
    ("Spectrogram.from_bytes", "raw", f32, lambda L: (spg_rows(L), 256), lambda L, x: L.Spectrogram(256).from_bytes(x)),
    ("Spectrogram.write", "c", None, None, lambda L, x: L.Spectrogram(256).write(x)),
    ("Spectrogram.write_bytes", "raw", None, None, lambda L, x: L.Spectrogram(256).write_bytes(x)),
    ("FMBank", "rows_c", f32, lambda L: (ROWS, L.FMBank(ROWS, 0.25, 2).num_outputs(K)),
     lambda L, x: L.FMBank(ROWS, 0.25, 2)(x)),
    ("FMBank[decim=1]", "rows_c", f32, (ROWS, K), lambda L, x: L.FMBank(ROWS, 0.25)(x)),
    ("AudioBank", "rows_f", f32, lambda L: (ROWS, L.AudioBank(ROWS, 0.37).num_outputs(K)),
     lambda L, x: L.AudioBank(ROWS, 0.37, deemphasis=48000.0)(x)),
    ("AudioBank[pcm16]", "rows_f", i16, lambda L: (ROWS, L.AudioBank(ROWS, 0.37).num_outputs(K)),
     lambda L, x: L.AudioBank(ROWS, 0.37, pcm16=True)(x)),
    ("Synthesizer", "rows_c", c64, lambda L: (L.Synthesizer(ROWS).num_outputs(K),), lambda L, x: L.Synthesizer(ROWS)(x)),
]


def nco(L):
    o = L.NCO("nco")
    o.freq = 0.3
    return o


def is_pinned(a):
    """A host result taken from the page-locked pool: its base is the capsule that returns the block."""
    return type(a.base).__name__ == "PyCapsule"


def check_pair(torch, h, d, xd, dtype, shape):
    """One host result h and its device twin d."""
    assert type(h) is np.ndarray and isinstance(d, torch.Tensor)
    assert h.dtype == dtype and d.dtype == getattr(torch, np.dtype(dtype).name)
    assert d.device == xd.device
    assert h.flags.c_contiguous and h.flags.writeable and d.is_contiguous()
    if shape is not None:
        assert h.shape == shape
    assert tuple(d.shape) == h.shape
    if h.ndim == 1:
        assert is_pinned(h) == (h.nbytes >= 64 << 10)
    else:
        assert not is_pinned(h)
    assert h.tobytes() == d.cpu().numpy().tobytes()


@pytest.mark.parametrize("name,key,dtype,shape,call", CASES, ids=[c[0] for c in CASES])
def test_host_and_device_results(ld, torch, data, name, key, dtype, shape, call):
    x = data[key]
    xd = torch.from_numpy(x.copy()).to("cuda:0")
    xh = x.tobytes() if name == "bytes_to_iq" else x
    h, d = call(ld, xh), call(ld, xd)
    torch.cuda.synchronize()
    if callable(shape):
        shape = shape(ld)
    if dtype is None:                                  # Spectrogram.write: the transforms taken
        assert type(h) is int and type(d) is int and h == d == ld.Spectrogram(256).num_outputs(N)[0]
    elif isinstance(h, tuple):                         # HilbertTransform.c2r: (lower, upper)
        assert isinstance(d, tuple) and len(h) == len(d) == 2
        for a, b in zip(h, d):
            check_pair(torch, a, b, xd, dtype, shape)
        assert h[0].tobytes() != h[1].tobytes()
    else:
        check_pair(torch, h, d, xd, dtype, shape)


def test_host_result_memory_kind(ld, data):
    # from 64 KB up a 1-D host result comes from the page-locked pool; a 2-D one never does
    x = np.resize(data["c"], 8192)
    y = ld.ComplexFIRFilter(H)(x)
    assert y.nbytes == 64 << 10 and is_pinned(y) and y.flags.writeable
    assert not is_pinned(ld.ComplexFIRFilter(H)(x[:8191]))
    rows = ld.Channelizer(4)(np.resize(data["c"], 65536))
    assert rows.nbytes >= 64 << 10 and rows.base is None
    img = ld.FMBank(ROWS, 0.25)(np.resize(data["rows_c"], (ROWS, 8192)))
    assert img.nbytes >= 64 << 10 and img.base is None


def test_many_calls_match_the_separate_host_calls(ld, torch, data):
    xs = [np.roll(data["c"], 7 * i) for i in range(3)]
    xd = [torch.from_numpy(x).to("cuda:0") for x in xs]
    for make, dtype in ((lambda: ld.AGC(), c64), (lambda: ld.AmpModem(0.5, "dsb", True), f32),
                        (lambda: ld.ComplexIIRFilter(), c64), (lambda: ld.RealIIRFilter(), f32)):
        ins = xs if dtype is not f32 or make().__class__ is ld.AmpModem else [np.ascontiguousarray(x.real) for x in xs]
        ind = xd if ins is xs else [torch.from_numpy(x).to("cuda:0") for x in ins]
        host = [make()(x) for x in ins]
        dev = ld.execute_many([make() for _ in ins], ind)
        assert isinstance(dev, list) and len(dev) == 3
        for h, d, x in zip(host, dev, ind):
            check_pair(torch, h, d, x, dtype, (N,))
    host = [ld.filter_resample(ld.ComplexIIRFilter(), ld.ComplexResampler(0.37, Fc=0.2), x) for x in xs]
    dev = ld.filter_resample_many([ld.ComplexIIRFilter() for _ in xs], [ld.ComplexResampler(0.37, Fc=0.2) for _ in xs], xd)
    assert isinstance(dev, list) and len(dev) == 3
    for h, d, x in zip(host, dev, xd):
        check_pair(torch, h, d, x, c64, None)


# ---------------------------------------------------------------- device-only paths of the row images
@pytest.mark.parametrize("name", ["FMBank", "AudioBank"])
def test_strided_views_are_refused_and_leave_the_state(ld, torch, data, name):
    make = (lambda: ld.FMBank(ROWS, 0.25, 2)) if name == "FMBank" else (lambda: ld.AudioBank(ROWS, 0.37))
    x = torch.from_numpy(data["rows_c" if name == "FMBank" else "rows_f"].copy()).to("cuda:0")
    wide = torch.cat([x, x], dim=1)
    obj, fresh = make(), make()
    assert torch.equal(obj(x[:, :500]), fresh(x[:, :500]))
    with pytest.raises(ValueError) as e:
        obj(wide[:, ::2])                              # columns two samples apart
    assert str(e.value) == f"{name}: the input's columns must be one sample apart (stride(1) == 1)"
    with pytest.raises(ValueError) as e:
        obj(x[0].expand(ROWS, K))                      # every row the same memory
    assert str(e.value) == f"{name}: the input's row stride must be at least its number of columns"
    with pytest.raises(ValueError) as e:
        obj(x.t().contiguous().t())                    # [ROWS, K] stored column by column
    assert str(e.value) == f"{name}: the input's columns must be one sample apart (stride(1) == 1)"
    # rows further apart than their length are read in place
    a, b = obj(wide[:, 500:K]), fresh(x[:, 500:].contiguous())
    torch.cuda.synchronize()
    assert a.shape == b.shape and torch.equal(a, b)


def test_synthesizer_copies_a_transposed_view(ld, torch, data):
    x = torch.from_numpy(data["rows_c"].copy()).to("cuda:0")
    xt = x.t().contiguous().t()
    assert xt.shape == x.shape and xt.stride() == (1, ROWS) and torch.equal(xt, x)
    wide = torch.cat([x, x], dim=1)[:, :K]             # rows 2 K apart: read in place
    same = x[0].expand(ROWS, K)                        # every row the same memory: copied too
    for view, dense in ((xt, x), (wide, x), (same, same.contiguous())):
        y, want = ld.Synthesizer(ROWS)(view), ld.Synthesizer(ROWS)(dense)
        torch.cuda.synchronize()
        assert y.dtype == torch.complex64 and y.shape == want.shape and y.is_contiguous()
        assert torch.equal(y, want)
