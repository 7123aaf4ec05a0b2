"""The kernels and dispatch branches a user reaches with a non-default
`nfilter`, `order` or tap count, against the CPU restatement (oracle/).

Every operator family picks its kernel on the host from the filter's size and
the call length; the rest of the suite runs the shapes of the AM chain.  Each
case here first asserts, through the `_dispatch` getters (the decision functions
of the execution paths themselves), that it reaches the branch it is named for;
tests/test_dispatch_host.py asserts the same without a GPU.  Parameter sets:
tests/dispatch_cases.py.

  R1/R2  k_resamp_direct and the staged k_resamp (branch tables of 64 / 80 KiB)
  R3     k_resamp_tile on inputs off a 16-byte boundary
  I1     k_iir_sect merged launches at 6 and 7 sections (the call-size sweep over
         2..7 sections is tests/test_gpu_parity.py::test_iir_exact_pipeline_call_sizes)
  I2     k_iir_seq<4>, k_iir_seq<17> (exact transfer functions)
  I3     iir_scan (fast mode, state dimension 9..16)
  I4     k_iir_spec_chunks with and without the LDS stage
  F1/F2  the NCO-fused overlap-save kernel at P = 320; the direct form with more
         than 64 KiB of LDS (the tap-count sweep is test_gpu_parity.py's)

Bars: bit-identical wherever the path is exact; for the float64 scan the
project's fast-mode bars (error against the float64 evaluation <= 1e-6 of the
output range, and no worse than the float32 restatement unless that is itself
below 1e-6); for the fast FIR the distance of the float32 restatement from the
float64 truth."""
import numpy as np
import pytest
import scipy.signal as sps

import dispatch_cases as dc
from conftest import cgauss, maxrel
from test_gpu_parity import assert_bitwise

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def _noise(rng, n, cplx):
    return cgauss(rng, n) if cplx else np.float32(rng.standard_normal(n))


def _run(f, x, cuts):
    return np.concatenate([f(x[a:b]) for a, b in zip(cuts[:-1], cuts[1:])])


# ------------------------------------------------------------------ R1 / R2
@pytest.mark.parametrize("cplx,m,nf,kernel", dc.RESAMP_SETS)
@pytest.mark.parametrize("rate", dc.RESAMP_RATES)
def test_resampler_large_tables_bitwise(ld, ora, rng, cplx, m, nf, kernel, rate):
    g = dc.resampler(ld, cplx, rate, m, nf)
    o = ora.Resampler(np.float32(rate), m, np.float32(dc.RESAMP_FC), 60.0, nf, cplx=cplx)
    cuts = dc.RESAMP_CUTS
    x = _noise(rng, cuts[-1], cplx)
    parts, kernels = [], []
    for a, b in zip(cuts[:-1], cuts[1:]):
        kern = g._dispatch(b - a)[0]
        parts.append(g(x[a:b]))
        assert kern == (kernel if len(parts[-1]) else "staged")     # no outputs: the history only
        kernels.append(kern)
    assert kernels.count(kernel) >= 2 and len(parts[-1]) > 256      # more than one workgroup
    if rate < 0.1:
        assert "staged" in kernels                                  # the decimator has calls without outputs
    ref = o(x)
    assert_bitwise(np.concatenate(parts), ref)
    g.reset()
    assert g._dispatch(len(x))[0] == kernel
    assert_bitwise(g(x), ref)


# ------------------------------------------------------------------ R3
@pytest.mark.parametrize("cplx,off", dc.MISALIGNED)
@pytest.mark.parametrize("rate", dc.MISALIGNED_RATES)
def test_resampler_tile_misaligned_input(ld, rng, cplx, off, rate):
    import torch
    cls = ld.ComplexResampler if cplx else ld.RealResampler
    kw = dict(rate=np.float32(rate), Fc=np.float32(min(rate, 0.4)))
    n, cut = 30_011, 7_777
    x = _noise(rng, n + off, cplx)
    xd = torch.from_numpy(x).cuda()[off:]
    assert xd.data_ptr() % 16 == off * x.itemsize
    g, a = cls(**kw), cls(**kw)
    ys = []
    for s, e in ((0, cut), (cut, n)):        # the second call starts in the history (a < 0)
        assert g._dispatch(e - s)[0] == "tile"
        ys.append(g(xd[s:e]).cpu().numpy())
    ref = np.concatenate([a(x[off:][:cut]), a(x[off:][cut:])])
    assert len(ref) > 512
    assert_bitwise(np.concatenate(ys), ref)


# ------------------------------------------------------------------ I1 (merged launches)
@pytest.mark.parametrize("order", dc.SECT_MANY_ORDERS)
def test_iir_sect_many_channels(ld, ora, rng, order):
    import torch
    C, cuts = 4, [0, 5000, 5001, 9_300]
    kw = dict(filter_type="cheby2", order=order, Fc=np.float32(dc.SECT_FC))

    def bank():
        fs = [ld.ComplexIIRFilter(**kw) for _ in range(C)]
        for f in fs:
            f.exact = True
            f._scan_path(1)
            assert f._dispatch(5000)[:2] == ("seq", dc.sect_tile(order))
        return fs

    many, single = bank(), bank()
    xs = [cgauss(rng, cuts[-1]) for _ in range(C)]
    xd = [torch.from_numpy(x).cuda() for x in xs]
    got = [[] for _ in range(C)]
    for a, b in zip(cuts[:-1], cuts[1:]):
        for c, y in enumerate(ld.execute_many(many, [t[a:b] for t in xd])):
            got[c].append(y.cpu().numpy())
    for c in range(C):
        assert_bitwise(np.concatenate(got[c]), _run(single[c], xs[c], cuts))
    o = ora.IIRFilter(prototype=("cheby2", "lowpass", 1, order, np.float32(dc.SECT_FC), 0.3, 0.7, 60.0))
    assert_bitwise(np.concatenate(got[0]), o(xs[0]))


# ------------------------------------------------------------------ I2
@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("N,wn,size_class", dc.SEQ_TF)
def test_iir_exact_tf_size_classes(ld, ora, rng, cplx, N, wn, size_class):
    b, a = dc.butter_tf(N, wn)
    cuts = dc.SEQ_CUTS
    x = _noise(rng, cuts[-1], cplx)
    ref = ora.IIRFilter(tf=(b, a), cplx=cplx)(x)
    cls = ld.CIIRFilter if cplx else ld.RIIRFilter
    g = cls(b, a)
    g.exact = True
    g._scan_path(1)                          # the sequential kernel, k_iir_seq<size_class>
    assert g._dispatch(cuts[-1])[:3] == ("seq", 0, size_class)
    assert_bitwise(_run(g, x, cuts), ref)
    s = cls(b, a)                            # automatic: speculative chunks, the same bits
    s.exact = True
    assert s._dispatch(cuts[-1])[0] == "spec" and s._dispatch(cuts[-1])[2] == size_class
    assert_bitwise(_run(s, x, cuts), ref)


# ------------------------------------------------------------------ I3
def _scan_case(ld, ora, kind, k, cplx):
    if kind == "proto":
        kw = dict(order=k, **dc.SCAN_PROTO)
        make = lambda: (ld.ComplexIIRFilter if cplx else ld.RealIIRFilter)(**kw)
        o = ora.IIRFilter(prototype=(kw["filter_type"], kw["band_type"], 1, k, np.float32(kw["Fc"]), kw["F0"], 0.7, 60.0),
                          cplx=cplx)
        return 2 * k, make, o
    b, a = dc.butter_tf(k, dc.SCAN_TF_WN)
    return k, (lambda: (ld.CIIRFilter if cplx else ld.RIIRFilter)(b, a)), ora.IIRFilter(tf=(b, a), cplx=cplx)


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("kind,k", [("proto", k) for k in dc.SCAN_PROTO_ORDERS] + [("tf", k) for k in dc.SCAN_TF_ORDERS])
def test_iir_scan_fallback_accuracy(ld, ora, rng, kind, k, cplx):
    """iir_scan (k_iir_scan_local, k_iir_scan_carry<D>, k_iir_scan_final) for
    every state dimension the blocked scan leaves to it, D = 9..16, over cuts
    that cross the 64-sample chunk and the change of plan (one to several chunks
    per carry thread) at 65 536 samples.  Odd D had no carry kernel
    (LDSP_EUNSUP) before this test."""
    D, make, o = _scan_case(ld, ora, kind, k, cplx)
    cuts = dc.SCAN_CUTS
    x = _noise(rng, cuts[-1], cplx)
    truth = o.execute_f64(x)
    o.reset()
    y32 = o(x)
    err_liquid = maxrel(y32, truth)
    g = make()
    g._scan_path(1)
    for n in np.diff(cuts):
        assert g._dispatch(int(n))[0] == "scan"
    err_gpu = maxrel(_run(g, x, cuts), truth)
    print(f"I3 {kind} {k} D={D} cplx={cplx}: scan {err_gpu:.3g} restatement {err_liquid:.3g}")
    assert err_gpu <= 1e-6, err_gpu
    assert err_gpu <= err_liquid or err_liquid < 1e-6, (err_gpu, err_liquid)
    # automatic path (the float64 scans or, for these fast-decaying filters, the
    # exact speculative chunks): no filter raises, and the fast-mode bar holds
    for n in dc.SCAN_AUTO_SIZES:
        err_auto = maxrel(make()(x[:n]), truth[:n])
        print(f"I3 {kind} {k} D={D} cplx={cplx}: auto n={n} {err_auto:.3g}")
        assert err_auto <= max(maxrel(y32[:n], truth[:n]), 1e-6), (n, err_auto)


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("order", dc.SCAN_PROTO_ORDERS)
def test_iir_bandpass_exact_bitwise(ld, ora, rng, order, cplx):
    """The same bandpass prototypes in exact mode (5..8 sections, k_iir_sect):
    design and recursion bit-identical to the restatement.  The float64 scan
    above first showed the orders 6 and 7 a float32 rounding error away from the
    float64 truth: one SOS coefficient of each was 1 ulp off the restatement's
    (the band transform's complex square root)."""
    kw = dict(order=order, **dc.SCAN_PROTO)
    g = (ld.ComplexIIRFilter if cplx else ld.RealIIRFilter)(**kw)
    o = ora.IIRFilter(prototype=(kw["filter_type"], kw["band_type"], 1, order, np.float32(kw["Fc"]), kw["F0"], 0.7, 60.0),
                      cplx=cplx)
    for got, ref in zip(g.sos(), o.sos()):
        assert_bitwise(np.float32(got).reshape(-1), ref.reshape(-1))
    g.exact = True
    g._scan_path(1)
    assert g._dispatch(5000)[:2] == ("seq", 1024 if order <= 6 else 512)
    x = _noise(rng, 9_000, cplx)
    assert_bitwise(np.concatenate([g(x[:5000]), g(x[5000:])]), o(x))


# ------------------------------------------------------------------ I4
@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("name,W,staged,size_class", dc.SPEC_CASES)
def test_iir_spec_stage_variants_bitwise(ld, ora, rng, cplx, name, W, staged, size_class):
    cuts = dc.SPEC_CUTS
    x = _noise(rng, cuts[-1], cplx)
    g = dc.spec_filter(ld, name, cplx)
    g.exact = True
    for n in np.diff(cuts):
        assert g._dispatch(int(n)) == ("spec", 0, size_class, W, staged)
    assert min(np.diff(cuts)) < W < max(np.diff(cuts)) // 4
    assert_bitwise(_run(g, x, cuts), dc.spec_oracle(ora, name, cplx)(x))


# ------------------------------------------------------------------ F1 (fused) / F2
def test_mix_down_filter_fused_p320(ld, ora, rng):
    L = 321
    N, P, M = dc.fir_window(L)
    assert (N, P) == (1024, 320)
    h = ora.firdes_kaiser(L, 0.05, 60.0)
    cuts = dc.fir_hop_cuts(L) + [10 * M + 20_001]
    x = cgauss(rng, cuts[-1])

    def pair():
        nco = ld.NCO("nco")
        nco.freq = np.float32(2 * np.pi * 0.05)
        nco.phase = np.float32(0.25)
        return nco, ld.ComplexFIRFilter(h)

    n1, f1 = pair()
    n2, f2 = pair()
    assert f1._dispatch(M) == ("fft", N, P)
    y = _run(lambda v: ld.mix_down_filter(n1, f1, v), x, cuts)
    two = _run(lambda v: f2(n2.mix_down(v)), x, cuts)
    assert_bitwise(y, two)                   # same call boundaries, so the same windows
    assert n1.state() == n2.state()
    on = ora.NCO(0)
    on.freq = np.float32(2 * np.pi * 0.05)
    on.phase = np.float32(0.25)
    mixed = on.mix_down(x)                   # table NCO: bit-exact on both sides
    ref = ora.FIRFilter(h, cplx=True)(mixed)
    truth = sps.lfilter(h.astype(np.float64), 1.0, mixed.astype(np.complex128))
    err_gpu, err_ref = maxrel(y, truth), maxrel(ref, truth)
    print(f"F1 fused L={L}: gpu {err_gpu:.3g} restatement {err_ref:.3g}")
    assert err_gpu <= max(1e-6, 1.3 * err_ref), (err_gpu, err_ref)


def test_fir_direct_long_filter(ld, ora, rng):
    L, n = dc.FIR_LONG, 20_000
    h = ora.firdes_kaiser(L, 0.1, 60.0)
    x = cgauss(rng, n)
    g = ld.ComplexFIRFilter(h)
    g.mode = "direct"
    assert g._dispatch(n) == ("direct", 0, 0)
    y = np.concatenate([g(x[:7_001]), g(x[7_001:])])
    ref = ora.FIRFilter(h, cplx=True)(x)
    truth = sps.lfilter(h.astype(np.float64), 1.0, x.astype(np.complex128))
    err_gpu, err_ref = maxrel(y, truth), maxrel(ref, truth)
    print(f"F2 direct L={L}: gpu {err_gpu:.3g} restatement {err_ref:.3g}")
    assert err_gpu <= max(1e-6, 1.3 * err_ref), (err_gpu, err_ref)
