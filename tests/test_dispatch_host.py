"""The dispatch getters (ldsp_debug_{fir,resamp,iir}_dispatch: pure host logic
that calls the decision functions of the execution paths) on every parameter set
of tests/dispatch_cases.py: each set must reach the kernel or template variant
its GPU test is named for.  Runs without a GPU, so the choice of shapes is
checked even where the kernels cannot be."""
import os
import sys

import numpy as np
import pytest

import dispatch_cases as dc

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-liquiddsp_amd")


@pytest.fixture(scope="module")
def ld():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import liquiddsp
    return liquiddsp


@pytest.mark.parametrize("cplx,m,nf,kernel", dc.RESAMP_SETS)
@pytest.mark.parametrize("rate", dc.RESAMP_RATES)
def test_resampler_large_table_kernels(ld, cplx, m, nf, kernel, rate):
    g = dc.resampler(ld, cplx, rate, m, nf)
    for a, b in zip(dc.RESAMP_CUTS[:-1], dc.RESAMP_CUTS[1:]):
        kern, kb = g._dispatch(b - a)       # at phase 0: every call of >= 1 sample has an output
        assert kern == kernel and kb == (256 if kernel == "direct" else 64)
    assert g._dispatch(0)[0] == "staged"    # no outputs: the history only


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("rate", dc.MISALIGNED_RATES)
def test_default_resampler_is_the_tile_kernel(ld, cplx, rate):
    cls = ld.ComplexResampler if cplx else ld.RealResampler
    kern, kb = cls(rate=np.float32(rate), Fc=np.float32(min(rate, 0.4)))._dispatch(20_000)
    assert kern == "tile" and kb in (128, 256)


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("order", dc.SECT_ORDERS)
def test_iir_sect_tiles(ld, cplx, order):
    g = (ld.ComplexIIRFilter if cplx else ld.RealIIRFilter)(filter_type="cheby2", order=order, Fc=np.float32(dc.SECT_FC))
    assert np.asarray(g.sos()[0]).shape == (dc.sect_sections(order), 3)
    g.exact = True
    g._scan_path(1)
    for n in (1, 1024, 12_289):
        path, tile, _, _, _ = g._dispatch(n)
        assert (path, tile) == ("seq", dc.sect_tile(order))


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("N,wn,size_class", dc.SEQ_TF)
def test_iir_seq_size_classes(ld, cplx, N, wn, size_class):
    b, a = dc.butter_tf(N, wn)
    g = (ld.CIIRFilter if cplx else ld.RIIRFilter)(b, a)
    g.exact = True
    for n in np.diff(dc.SEQ_CUTS):          # automatic: the speculative chunks, staged in LDS
        path, tile, z, w, staged = g._dispatch(int(n))
        assert (path, z, staged) == ("spec", size_class, True) and 0 < w <= 4096
    g._scan_path(1)
    for n in np.diff(dc.SEQ_CUTS):          # forced: k_iir_seq<size_class>, not the section kernel
        assert g._dispatch(int(n))[:3] == ("seq", 0, size_class)


def _scan_filters(ld, cplx):
    for order in dc.SCAN_PROTO_ORDERS:
        yield 2 * order, (ld.ComplexIIRFilter if cplx else ld.RealIIRFilter)(order=order, **dc.SCAN_PROTO)
    for N in dc.SCAN_TF_ORDERS:
        yield N, (ld.CIIRFilter if cplx else ld.RIIRFilter)(*dc.butter_tf(N, dc.SCAN_TF_WN))


@pytest.mark.parametrize("cplx", [True, False])
def test_iir_scan_fallback_is_forced(ld, cplx):
    dims = []
    for D, g in _scan_filters(ld, cplx):
        g._scan_path(1)
        for n in list(np.diff(dc.SCAN_CUTS)) + dc.SCAN_AUTO_SIZES:
            assert g._dispatch(int(n))[0] == "scan", (D, n)
        dims.append(D)
    assert sorted(set(dims)) == list(range(9, 17))      # every D the blocked scan leaves to iir_scan


@pytest.mark.parametrize("cplx", [True, False])
@pytest.mark.parametrize("name,W,staged,size_class", dc.SPEC_CASES)
def test_iir_spec_stage_variants(ld, cplx, name, W, staged, size_class):
    g = dc.spec_filter(ld, name, cplx)
    if name != "onepole":
        assert np.asarray(g.sos()[0]).shape == (5, 3)
    g.exact = True
    for n in np.diff(dc.SPEC_CUTS):
        assert g._dispatch(int(n)) == ("spec", 0, size_class, W, staged)


@pytest.mark.parametrize("L", dc.FIR_TAPS + [dc.FIR_LONG])
def test_fir_dispatch(ld, ora, L):
    h = ora.firdes_kaiser(L, 0.1, 60.0) if L > 1 else np.float32([0.7])
    for cplx in (True, False):
        for mode in ("fast", "direct"):
            g = (ld.ComplexFIRFilter if cplx else ld.RealFIRFilter)(h)
            g.mode = mode
            for n in (1, 4096, 70_001):
                assert g._dispatch(n) == dc.fir_expected(L, cplx, mode), (cplx, mode, n)
            assert g._dispatch(0)[0] == "direct"        # an empty call moves the history only
    g = ld.ComplexFIRFilter(h)
    g.exact = True
    assert g._dispatch(100) == ("exact", 0, 0)


def test_fir_overlap_classes_are_all_covered():
    # every overlap the FFT path supports, both window lengths, and the tap counts either side of each edge
    assert {dc.fir_window(L)[1] for L in dc.FIR_TAPS if 48 <= L <= 513} == set(range(64, 513, 64))
    assert {47, 48, 129, 130, 513, 514} <= set(dc.FIR_TAPS)
    for L in dc.FIR_TAPS:
        cuts = dc.fir_hop_cuts(L)
        M = dc.fir_window(L)[2]
        assert cuts[0] == 0 and cuts[-1] == 10 * M and {M - 1, M, M + 1} <= set(np.diff(cuts))
