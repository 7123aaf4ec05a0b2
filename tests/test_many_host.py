"""Every parameter set of tests/many_cases.py against the library's own decision
code (AGC._dispatch, AmpModem._dispatch, the IIR filters' _dispatch, _modal_info
and _modal_grid: host logic that the execute paths themselves call).  Runs
without a GPU, so a set that stops reaching the branch its GPU test in
tests/test_gpu_many_mixed.py is written for fails here.  What depends on an
object's past (an AGC turning speculative) is pinned here for fresh objects and
asserted call by call in the GPU test."""
import os
import sys

import numpy as np
import pytest

import many_cases as mc

PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-liquiddsp_amd")


@pytest.fixture(scope="module")
def ld():
    if PKG not in sys.path:
        sys.path.insert(0, PKG)
    import liquiddsp
    return liquiddsp


@pytest.mark.parametrize("bw", sorted(mc.AGC_WARMUPS))
def test_agc_thresholds(ld, bw):
    W, Wa, parmin = mc.AGC_WARMUPS[bw]
    g = ld.AGC()
    g.bandwidth = bw
    for n, want in ((0, "seq"), (mc.AGC_SMALL_MIN - 1, "seq"), (mc.AGC_SMALL_MIN, "small"), (parmin - 1, "small"),
                    (parmin, "par"), (300_007, "par")):
        path, w, wa, C, hist_len, hist_valid, spec = g._dispatch(n)
        assert (path, w, wa) == (want, W, Wa), (n, path, w, wa)
        assert hist_len == W + Wa + 256 and hist_valid == 0 and not spec     # a fresh object has no history
        assert (C == 0) == (want == "seq" or n == 0)
        if want == "par":
            assert C == 1024
        if want == "small":
            assert 32 <= C <= 256 and C % 32 == 0


def test_agc_mixed_case_paths(ld):
    gs = [mc.agc(ld, c) for c in range(len(mc.AGC_BW))]
    for n, paths in zip(mc.AGC_CALLS, mc.AGC_PATHS):
        assert [g._dispatch(n)[0] for g in gs] == paths, n
    assert len({g._dispatch(40_000)[1:3] for g in gs}) == 3          # three different (W, Wa) in one merged launch
    # the history lengths the table of speculative calls is worked out from
    assert [g._dispatch(1)[4] for g in gs] == [1536, 4756, 4756, 45_256, 4756]
    gs[mc.AGC_SETTER_CH].bandwidth = mc.AGC_SETTER_BW
    assert gs[mc.AGC_SETTER_CH]._dispatch(1)[4] not in (1536, 4756)   # another history length: the history restarts
    for n, paths in zip(mc.AGC_CALLS_AFTER, mc.AGC_PATHS_AFTER):
        assert [g._dispatch(n)[0] for g in gs] == paths, n
    # every n of the mixed tests takes each of the three paths on some bandwidth or other
    seen = {mc.agc(ld, c)._dispatch(n)[0] for c in range(5) for n in mc.SIZES if n}
    assert seen == {"seq", "small", "par"}


def test_ampmodem_paths(ld):
    for n, (car, cos) in mc.AMP_PATHS.items():
        for carrier, mod in zip(mc.AMP_CARRIER, mc.AMP_MOD):
            a = ld.AmpModem(modulation=mod, type="dsb", carrier=carrier)
            assert a._dispatch(n) == (car if carrier else cos, True), (n, carrier)
    assert set(mc.AMP_CALLS) == set(mc.AMP_PATHS)
    assert mc.AMP_PATHS[1100] == ("par", "seq")                     # lists of unequal length in one many-call
    for typ in ("usb", "lsb"):                                      # single sideband: the whole many-call falls back
        assert ld.AmpModem(modulation=0.5, type=typ, carrier=True)._dispatch(40_000)[1] is False
    a = ld.AmpModem(modulation=0.5, type="dsb", carrier=True)
    assert a._dispatch(0)[0] == "seq"


@pytest.mark.parametrize("cplx", [True, False])
def test_modal_filters_and_grids(ld, cplx):
    for order, fc, M, J in mc.MODAL_FILTERS:
        f = mc.modal_filter(ld, order, fc, cplx)
        ok, m, j, _ = f._modal_info()
        assert (ok, m, j) == (True, M, J), (order, fc)
        for n in mc.SIZES:
            if n:
                assert f._dispatch(n)[0] == "modal", (order, fc, n)
        for n, (units, grids) in mc.MODAL_GRIDS.items():
            u, onex, grid = f._modal_grid(n)
            assert (u, grid) == (units, grids[J]), (order, fc, n)
            assert onex == (units <= 16 * J) and grid == (8 * units if onex else units)
    # the groupings of the GPU test: launches = groups of (M, grid), grids off a multiple of 8 one per object
    for n, want in mc.MODAL_LAUNCHES.items():
        groups = {}
        for order, fc, M, J in mc.MODAL_FILTERS:
            g = mc.MODAL_GRIDS[n][1][J]
            groups[(M, g)] = groups.get((M, g), 0) + 1
        launches = sum(mc.ceil_div(c, 8) if g % 8 == 0 else c for (_, g), c in groups.items())
        assert launches == want, (n, groups)
    assert 147 % 8 != 0 and 1176 % 8 == 0 and 160 % 8 == 0


@pytest.mark.parametrize("cplx", [True, False])
def test_exact_cases(ld, cplx):
    cls = ld.ComplexIIRFilter if cplx else ld.RealIIRFilter
    blocks = []
    for order in mc.SECT_ORDERS:
        f = cls(filter_type="cheby2", order=order, Fc=np.float32(mc.SECT_FC))
        f.exact = True
        f._scan_path(1)
        path, tile, _, _, _ = f._dispatch(40_000)
        assert path == "seq" and tile in (512, 1024)
        blocks.append(np.asarray(f.sos()[0]).shape[0])
    assert blocks == [4, 4, 6, 7, 3] and len(set(blocks)) == mc.SECT_LAUNCHES
    for ft, order in mc.SPEC_PROTOS:
        f = cls(filter_type=ft, order=order, Fc=np.float32(mc.SPEC_FC))
        f.exact = True
        for n in mc.SPEC_CALLS + [40_000]:
            assert f._dispatch(n)[0] == "spec", (ft, n)
    for r in mc.ONEPOLE_R:
        f = (ld.CIIRFilter if cplx else ld.RIIRFilter)(np.float32([1 - r]), np.float32([1, -r]))
        f.exact = True
        for n in mc.SPEC_CALLS:
            assert f._dispatch(n)[0] == "spec", (r, n)


def test_front_cases(ld):
    for cplx in (True, False):
        for fc, rate in mc.FRONT:
            f = mc.modal_filter(ld, 8, fc, cplx)
            assert f._modal_info()[0]
            rs = mc.resampler(ld, rate, cplx)
            for n in mc.FRONT_CALLS:
                if n:
                    assert f._dispatch(n)[0] == "modal"             # the fused pass
                    assert rs._dispatch(n)[0] == "tile"
    assert len({rate for _, rate in mc.FRONT}) == 3 and mc.FRONT[0] == mc.FRONT[mc.FRONT_PRE_CH]
    assert mc.CAP_C == [1, 2, 9, 17] and max(mc.CAP_C) <= 17
