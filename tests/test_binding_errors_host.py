"""The validations the Python binding performs itself, without a GPU (CPU suite):
the exception type and the full message of every one that can be reached
without a device.  The binding builds every call from one input builder, one
output allocator and one invoker (pybind/liquiddsp_module.cpp); the messages
here are what callers saw before that, written out literally.  A host call that
passes them ends in the C ABI's "no CPU fallback" RuntimeError where there is
no device, so the shape errors are shown to come first.  Device-only messages
(strides, the current device) are in tests/test_gpu_binding_results.py and
tests/test_gpu_dist.py."""
import numpy as np
import pytest


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


def raises(exc, msg, fn, *a, **kw):
    with pytest.raises(exc) as e:
        fn(*a, **kw)
    assert type(e.value) is exc and str(e.value) == msg, (type(e.value), str(e.value))


ONES = np.ones(8, np.float32)


# ---------------------------------------------------------------- constructors
def test_bank_constructor_errors(ld):
    V = ValueError
    raises(V, "Channelizer: nchan must be a power of two, at least 4", ld.Channelizer, -4)
    raises(V, "Channelizer: decim must be nchan or nchan // 2", ld.Channelizer, 8, decim=-1)
    raises(V, "Channelizer: m must be >= 1", ld.Channelizer, 8, m=-1)
    raises(V, "Synthesizer: nchan must be a power of two, at least 4", ld.Synthesizer, -4)
    raises(V, "Synthesizer: interp must be nchan or nchan // 2", ld.Synthesizer, 8, interp=-1)
    raises(V, "Synthesizer: m must be >= 1", ld.Synthesizer, 8, m=-1)
    raises(V, "Downconverter: decim must be at least 2", ld.Downconverter, [0.1], -2)
    raises(V, "Downconverter: m must be >= 1", ld.Downconverter, [0.1], 4, m=-1)
    raises(V, "FMBank: nchan must lie in 1 .. 256", ld.FMBank, -1, 0.25)
    raises(V, "FMBank: decim must lie in 1 .. 64", ld.FMBank, 2, 0.25, -1)
    raises(V, "FMBank: m must be >= 1", ld.FMBank, 2, 0.25, 4, m=-1)
    raises(V, "AudioBank: nchan must lie in 1 .. 256", ld.AudioBank, -1, 0.5)
    raises(V, "AudioBank: len must be >= 1", ld.AudioBank, 2, 0.5, len=-1)
    raises(V, "AudioBank: nfilter must be >= 1", ld.AudioBank, 2, 0.5, nfilter=-1)
    raises(V, "AudioBank: deemphasis (the rows' sample rate) must be > 0", ld.AudioBank, 2, 0.5, deemphasis=0.0)
    raises(V, "Spectrogram: nfft must be a power of two", ld.Spectrogram, -256)
    raises(V, "Spectrogram: window_len must lie in 1 .. nfft", ld.Spectrogram, 256, window_len=-1)
    raises(V, "Spectrogram: delay must be at least 1", ld.Spectrogram, 256, delay=-1)
    raises(V, "Spectrogram: average must be at least 1", ld.Spectrogram, 256, average=-1)
    # with taps the m and Fc arguments are not looked at
    assert ld.Channelizer(8, m=-1, Fc=7.0, taps=ONES).nchan == 8
    assert ld.FMBank(2, 0.25, 4, m=-1, Fc=7.0, taps=ONES).decim == 4


def test_other_constructor_errors(ld):
    V = ValueError
    raises(V, "firhilb: m must be >= 2", ld.HilbertTransform, -1)
    raises(V, "Delay: nd must be >= 0", ld.Delay, -1)
    d = ld.Delay(3)
    raises(V, "Delay: nd must be >= 0", setattr, d, "delay", -2)
    assert d.delay == 3
    raises(V, "BroadcastAM: slen must be >= 1", ld.BroadcastAM, 0)
    for cls in (ld.RealResampler, ld.ComplexResampler):
        raises(V, "resampler: len must be >= 1", cls, 0.5, 0, 0.2)
        raises(V, "resampler: nfilter must be >= 1", cls, 0.5, 20, 0.2, 60.0, 0)
    raises(V, "RealDCBlocker: slen must be >= 1", ld.RealDCBlocker, 0)
    raises(V, "RealKaiserBessel: flen must be >= 1", ld.RealKaiserBessel, 0, 0.1)
    raises(V, "iirfilt: order must be >= 1", ld.CLowpassIIR, "butter", 0, 0.1)
    raises(V, "iirfilt: order must be >= 1", ld.RBandpassIIR, "butter", 0, 0.1, 0.2)
    raises(V, "iirfilt: order must be >= 1", ld.ComplexIIRFilter, order=0)
    raises(V, "iirfilt: order must be >= 1", ld.RealIIRFilter, order=0)
    f = ld.ComplexFIRFilter(ONES)
    raises(V, "mode must be 'fast', 'direct' or 'exact'", setattr, f, "mode", "quick")
    assert f.mode == "fast"


@pytest.mark.parametrize("Fc", [0.0, -0.1, 0.5, 0.75, float("nan")])
def test_cutoff_out_of_range(ld, Fc):
    V = ValueError
    raises(V, "Channelizer: Fc must lie in (0, 0.5)", ld.Channelizer, 8, Fc=Fc)
    raises(V, "Synthesizer: Fc must lie in (0, 0.5)", ld.Synthesizer, 8, Fc=Fc)
    raises(V, "Downconverter: Fc must lie in (0, 0.5)", ld.Downconverter, [0.1], 4, Fc=Fc)
    raises(V, "FMBank: Fc must lie in (0, 0.5)", ld.FMBank, 2, 0.25, 4, Fc=Fc)


def test_spectrogram_window_length(ld):
    raises(ValueError, "Spectrogram: the window array's length must be window_len", ld.Spectrogram, 256,
           window=np.ones(100, np.float32))
    raises(ValueError, "Spectrogram: the window array's length must be window_len", ld.Spectrogram, 256,
           window=np.ones(256, np.float32), window_len=128)
    assert ld.Spectrogram(256, window=np.ones(128, np.float32), window_len=128).window_len == 128


# ---------------------------------------------------------------- row images on the host
def after_the_checks(ld, call, shape):
    """A call whose shape passes: the C ABI's error where there is no device, the result's shape where there is one."""
    if ld.device_count() == 0:
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()
    else:
        assert call().shape == shape


def test_row_image_errors_come_before_the_device(ld):
    V = ValueError
    c64, f32 = np.complex64, np.float32
    fb, ab, sy = ld.FMBank(3, 0.25, 4), ld.AudioBank(3, 0.5), ld.Synthesizer(4)
    for obj, name, dt, vec in ((fb, "FMBank", c64, " (1-D when nchan is 1)"), (ab, "AudioBank", f32, " (1-D when nchan is 1)"),
                               (sy, "Synthesizer", c64, "")):
        n = obj.nchan
        for bad in (np.zeros(64, dt), np.zeros((n, 4, 4), dt), np.zeros((), dt)):
            raises(V, f"{name}: the input must be 2-D, [nchan, K]{vec}", obj, bad)
        for rows in (n - 1, n + 1, 1):
            raises(V, f"{name}: the input has {rows} rows, nchan is {n}", obj, np.zeros((rows, 64), dt))
        raises(V, f"{name}: the input has 0 rows, nchan is {n}", obj, np.zeros((0, 64), dt))
        # other dtypes and lists are force-cast first, then checked alike
        raises(V, f"{name}: the input has 2 rows, nchan is {n}", obj, [[1.0, 2.0], [3.0, 4.0]])
    assert fb.skip == 0
    after_the_checks(ld, lambda: fb(np.zeros((3, 64), c64)), (3, 16))
    after_the_checks(ld, lambda: ab(np.zeros((3, 64), f32)), (3, ab.num_outputs(64)))
    after_the_checks(ld, lambda: sy(np.zeros((4, 16), c64)), (32,))


def test_one_row_banks_take_vectors(ld):
    f1, a1 = ld.FMBank(1, 0.25, 4), ld.AudioBank(1, 0.5)
    after_the_checks(ld, lambda: f1(np.zeros(64, np.complex64)), (1, 16))
    after_the_checks(ld, lambda: a1(np.zeros(64, np.float32)), (1, a1.num_outputs(64)))
    raises(ValueError, "FMBank: the input must be 2-D, [nchan, K] (1-D when nchan is 1)", f1,
           np.zeros((1, 4, 4), np.complex64))
    raises(ValueError, "AudioBank: the input has 2 rows, nchan is 1", a1, np.zeros((2, 64), np.float32))


# ---------------------------------------------------------------- 1-D calls
def test_from_bytes_needs_a_complex_filter(ld):
    raw = np.zeros(64, np.int16)
    for f in (ld.RealIIRFilter(), ld.RIIRFilter([1.0], [1.0, -0.5]), ld.RLowpassIIR("butter", 2, 0.1),
              ld.RBandstopIIR("butter", 2, 0.1, 0.2)):
        raises(ValueError, "from_bytes: int16 IQ input needs a complex filter", f.from_bytes, raw)
        raises(ValueError, "from_bytes: int16 IQ input needs a complex filter", f.from_bytes, raw.tobytes())
    after_the_checks(ld, lambda: ld.ComplexIIRFilter().from_bytes(raw), (32,))


def test_delay_and_hilbert_other_dtypes_give_none(ld):
    assert ld.Delay(2)(np.zeros(8, np.float64)) is None
    assert ld.Delay(2)(np.zeros(8, np.int16)) is None
    assert ld.HilbertTransform()(np.zeros(8, np.complex128)) is None
    with pytest.raises(AttributeError):
        ld.Delay(2)([1.0, 2.0])                       # no dtype to dispatch on


def test_filter_resample_errors(ld):
    x = np.zeros(64, np.complex64)
    cf, rf = ld.ComplexIIRFilter(), ld.RealIIRFilter()
    cr, rr = ld.ComplexResampler(0.5, Fc=0.2), ld.RealResampler(0.5, Fc=0.2)
    mixed = "filter_resample: the filter and the resampler must both be complex or both real"
    raises(ValueError, mixed, ld.filter_resample, cf, rr, x)
    raises(ValueError, mixed, ld.filter_resample, rf, cr, x)
    raises(ValueError, mixed, ld.filter_resample, ld.DeemphasisFilter(48000), ld.CResampler(0.5), x)
    raises(TypeError, "filter_resample: iir must be one of the IIR filter classes", ld.filter_resample,
           ld.ComplexFIRFilter(ONES), cr, x)
    raises(TypeError, "filter_resample: iir must be one of the IIR filter classes", ld.filter_resample, None, cr, x)
    raises(TypeError, "filter_resample: resampler must be one of the resampler classes", ld.filter_resample, cf, cf, x)
    raises(TypeError, "filter_resample: resampler must be one of the resampler classes", ld.filter_resample, cf,
           ld.FMStereo(), x)
    after_the_checks(ld, lambda: ld.filter_resample(cf, cr, x), (32,))


def test_many_calls_errors(ld):
    V = ValueError
    x = np.zeros(64, np.complex64)
    assert ld.execute_many([], []) == [] and ld.execute_many([], [x]) == []
    assert ld.filter_resample_many([], [], []) == []
    raises(V, "execute_many: one input per object", ld.execute_many, [ld.AGC(), ld.AGC()], [x])
    raises(V, "execute_many: one input per object", ld.execute_many, [ld.AGC()], [])
    for obj in (ld.AGC(), ld.AmpModem(), ld.ComplexIIRFilter(), ld.RealIIRFilter()):
        raises(V, "execute_many: device tensors only", ld.execute_many, [obj], [x])
    raises(V, "execute_many: device tensors only", ld.execute_many, [ld.AGC()], [[1.0, 2.0]])
    cf, rf = ld.ComplexIIRFilter(), ld.RealIIRFilter()
    cr, rr = ld.ComplexResampler(0.5, Fc=0.2), ld.RealResampler(0.5, Fc=0.2)
    one = "filter_resample_many: one resampler and input per filter"
    raises(V, one, ld.filter_resample_many, [cf], [cr, cr], [x])
    raises(V, one, ld.filter_resample_many, [cf], [cr], [x, x])
    raises(V, one, ld.filter_resample_many, [cf, cf], [cr], [x])
    raises(V, "filter_resample_many: mixed real and complex", ld.filter_resample_many, [rf], [cr], [x])
    raises(V, "filter_resample_many: mixed real and complex", ld.filter_resample_many, [cf], [rr], [x])
    raises(V, "filter_resample_many: device tensors only", ld.filter_resample_many, [cf], [cr], [x])
    raises(V, "filter_resample_many: device tensors only", ld.filter_resample_many, [rf], [rr], [x.real])
    raises(TypeError, "filter_resample: iir must be one of the IIR filter classes", ld.filter_resample_many,
           [ld.AGC()], [cr], [x])
    raises(TypeError, "filter_resample: resampler must be one of the resampler classes", ld.filter_resample_many,
           [cf], [ld.AGC()], [x])
