"""Golden vectors (tests/golden/golden.npz, made by tests/golden/make_golden.py
from the CPU restatement; "parity unpinned" w.r.t. a real liquid-dsp run, see
the fixture's golden.json).

  * CPU: the restatement still reproduces every stored output bit for bit and
    the stored designs (pins oracle/ against regressions).
  * GPU: the MI355X kernels reproduce the stored outputs -- bit for bit in the
    exact modes and for every kernel whose fast mode is exact (resampler, NCO,
    AGC, AmpModem, de-emphasis); the fast FIR within 1e-6 relative; the fast
    IIR (float64 scan) within 1e-6 of the float64 recursion and no further from
    it than the float32 recursion is.
"""
import json
import os

import numpy as np
import pytest

from conftest import maxrel

HERE = os.path.dirname(os.path.abspath(__file__))
G = dict(np.load(os.path.join(HERE, "golden", "golden.npz")),
         chain_x=np.load(os.path.join(HERE, "golden", "golden_chain_x.npy")))   # (a file of its own, for size)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.complex64 else np.uint32)


def same(y, ref):
    assert y.shape == ref.shape, (y.shape, ref.shape)
    eq = bits(y) == bits(ref)
    assert eq.all(), f"{(~eq).sum()} of {eq.size} differ; first at {int(np.argmin(eq))}"


def test_fixture_metadata():
    meta = json.load(open(os.path.join(HERE, "golden", "golden.json")))
    assert "unpinned" in meta["parity"]
    assert set(meta["switches"]) >= {"resampler", "nco", "dotprod", "loop_math"}


# ------------------------------------------------------------------ CPU: oracle pinned to the fixture
def test_oracle_reproduces_fir(ora):
    same(ora.firdes_kaiser(127, 0.1, 60.0, 0.0), G["fir127_h"])
    same(ora.FIRFilter(G["fir127_h"], cplx=True)(G["fir127_x"]), G["fir127_y"])
    fr = ora.FIRFilter(kaiser=(25, 0.2, 20.0, 0.0), cplx=False)
    fr.scale = 0.75
    same(fr.taps, G["firr_h"])
    same(fr(G["firr_x"]), G["firr_y"])
    dc = ora.FIRFilter(dc_blocker=(25, 20.0), cplx=False)
    same(dc.taps, G["dcblock_h"])
    same(dc(G["firr_x"]), G["dcblock_y"])


def test_oracle_reproduces_resampler_nco(ora):
    r = ora.Resampler(float(np.float32(0.024)), m=20, fc=0.024, As=60.0, npfb=13, cplx=True)
    assert r.step == int(G["resamp_step"][0]) == 699050688
    same(r(G["resamp_x"]), G["resamp_y"])
    rr = ora.Resampler(0.37, m=7, fc=0.2, As=50.0, npfb=32, cplx=False)
    same(rr(G["resampr_x"]), G["resampr_y"])
    nco = ora.NCO(0)
    nco.freq = float(2 * np.pi * 0.05)
    nco.phase = 0.4
    same(nco.mix_down(G["nco_x"]), G["nco_y"])


def test_oracle_reproduces_iir_agc_ampmodem_chain(ora):
    B, A = ora.iirdes("cheby2", "lowpass", 8, 15000 / 2e6, 0.0, 0.1, 60.0)
    same(B, G["iir_B"])
    same(A, G["iir_A"])
    f = ora.IIRFilter(sos=(G["iir_B"], G["iir_A"]), cplx=True)
    same(f(G["iir_x"]), G["iir_y"])
    f.reset()
    same(f.execute_f64(G["iir_x"]), G["iir_y64"])
    d = ora.IIRFilter(tf=(G["deemph_b"], G["deemph_a"]), cplx=False)
    same(d(G["deemph_x"]), G["deemph_y"])
    agc = ora.AGC()
    agc.lock(False)
    agc.scale = 0.01
    same(agc(G["agc_x"]), G["agc_y"])
    same(ora.AmpModem(0.5, "dsb", True)(G["agc_y"]), G["ampmodem_y"])
    same(ora.AmpModem(0.75, "dsb", False)(G["agc_y"]), G["ampmodem_costas_y"])
    same(ora.AMRadio()(G["chain_x"]), G["chain_y"])


# ------------------------------------------------------------------ GPU: kernels against the fixture
@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


@pytest.mark.gpu
def test_gpu_golden_fir(ld):
    g = ld.ComplexFIRFilter(G["fir127_h"])
    g.exact = True
    same(g(G["fir127_x"]), G["fir127_y"])
    fast = ld.ComplexFIRFilter(G["fir127_h"])
    assert maxrel(fast(G["fir127_x"]), G["fir127_y"]) <= 1e-6
    dc = ld.RealDCBlocker(25, 20.0)
    dc.exact = True
    same(dc(G["firr_x"]), G["dcblock_y"])


@pytest.mark.gpu
def test_gpu_golden_resampler_nco(ld):
    r = ld.ComplexResampler(rate=np.float32(0.024), len=20, Fc=np.float32(0.024), As=60.0, nfilter=13)
    same(np.concatenate([r(G["resamp_x"][:7001]), r(G["resamp_x"][7001:])]), G["resamp_y"])
    rr = ld.RealResampler(rate=np.float32(0.37), len=7, Fc=np.float32(0.2), As=50.0, nfilter=32)
    same(rr(G["resampr_x"]), G["resampr_y"])
    nco = ld.NCO("nco")
    nco.freq = np.float32(2 * np.pi * 0.05)
    nco.phase = np.float32(0.4)
    same(nco.mix_down(G["nco_x"]), G["nco_y"])


@pytest.mark.gpu
def test_gpu_golden_iir(ld):
    g = ld.ComplexIIRFilter(filter_type="cheby2", order=8, Fc=15000 / 2e6, Ap=0.1, As=60.0)
    B, A = g.sos()
    same(np.float32(B), G["iir_B"])
    same(np.float32(A), G["iir_A"])
    g.exact = True
    same(g(G["iir_x"]), G["iir_y"])
    # fast mode (float64 scan): SURVEY 8(d) -- within 1e-6 of the float64 truth,
    # and no further from it than the float32 recursion
    fast = ld.ComplexIIRFilter(filter_type="cheby2", order=8, Fc=15000 / 2e6, Ap=0.1, As=60.0)
    err_gpu, err_f32 = maxrel(fast(G["iir_x"]), G["iir_y64"]), maxrel(G["iir_y"], G["iir_y64"])
    assert err_gpu <= 1e-6 and err_gpu <= err_f32, (err_gpu, err_f32)
    d = ld.DeemphasisFilter(48000)
    same(d(G["deemph_x"]), G["deemph_y"])


@pytest.mark.gpu
def test_gpu_golden_agc_ampmodem_chain(ld):
    agc = ld.AGC()
    agc.lock = False
    agc.scale = 0.01
    same(agc(G["agc_x"]), G["agc_y"])
    same(ld.AmpModem(modulation=0.5, type="dsb", carrier=True)(G["agc_y"]), G["ampmodem_y"])
    same(ld.AmpModem(modulation=0.75, type="dsb", carrier=False)(G["agc_y"]), G["ampmodem_costas_y"])
    bandpass = ld.ComplexIIRFilter(filter_type="cheby2", order=8, Fc=15000 / 2000000)
    bandpass.exact = True
    resample = ld.ComplexResampler(rate=48000 / 2000000, Fc=48000 / 2000000)
    am = ld.AmpModem(modulation=0.5, type="dsb", carrier=True)
    audio = ld.DeemphasisFilter(48000)
    a2 = ld.AGC()
    a2.lock = False
    a2.scale = 0.01
    x = G["chain_x"]
    y = np.concatenate([audio(am(a2(resample(bandpass(x[i:i + 16384]))))) for i in range(0, x.size, 16384)])
    same(y, G["chain_y"])
