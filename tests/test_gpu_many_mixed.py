"""Many-calls (execute_many, filter_resample_many, ldsp_*_execute_many) on channels
that differ -- in configuration, in history and in signal -- and the same
irregular signals on single objects.

The many-calls rest on one recorder (csrc/batch.hpp): every object's execute is
recorded as an op list, the lists are issued round-robin by op index, and ops of
one index that name the same kernel with the same grid, block and LDS size
become one launch whose blockIdx.y picks the object's arguments.  With identical
channels every list is the same and every group merges completely; here the
lists differ in length and order, groups are partial, the per-object arguments of
a merged launch differ, and groups split at the argument cap.

Reference: for every channel a twin object built the same way and driven by
ordinary per-object calls on the same inputs, bit for bit, outputs and
afterwards state (pll_state(), AGC.gain, a further 5 000-sample call on both).
In addition the restatement (oracle): exact stages bit for bit, the fast modal
IIR within 1e-6 of its float64 evaluation.  Where a case is meant
to merge, launch counts from the profiler around one many-call prove it.

The parameter sets live in tests/many_cases.py; tests/test_many_host.py pins
the path of each against the library's dispatch getters without a GPU."""
import ctypes as C
import os

import numpy as np
import pytest

import many_cases as mc
from conftest import maxrel

pytestmark = pytest.mark.gpu

TINY = np.finfo(np.float32).tiny
FURTHER = 5000


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


# ---------------------------------------------------------------- helpers
def hbits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.complex64 else np.uint32)


def same(a, b):
    """Two device tensors, bit for bit."""
    import torch
    iv = {torch.complex64: torch.int64, torch.float32: torch.int32}
    return (a.shape == b.shape and a.dtype == b.dtype
            and torch.equal(a.contiguous().view(iv[a.dtype]), b.contiguous().view(iv[b.dtype])))


def same_host(t, ref):
    y = t.cpu().numpy()
    return y.shape == ref.shape and y.dtype == ref.dtype and np.array_equal(hbits(y), hbits(ref))


def dev(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def counted(ld, fn):
    """fn() with the profiler on: (result, {kernel name: launches})."""
    import torch
    torch.cuda.synchronize()
    ld._profile_reset()
    ld._profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
    finally:
        ld._profile_enable(False)
    return out, {k: v[0] for k, v in ld._profile_report().items()}


def subnormals(y):
    a = np.abs(np.ascontiguousarray(y).view(np.float32))
    return int(((a > 0) & (a < TINY)).sum())


def am_signal(n, c, level=0.1, mod=0.5, f=0.002, noise=0.02):
    """AM at the sample rate of the back half: three message tones, a carrier offset of either sign."""
    rng = np.random.default_rng(500 + c)
    t = np.arange(n)
    msg = (np.sin(2 * np.pi * 0.0031 * t) + np.sin(2 * np.pi * 0.0083 * t + c) + np.sin(2 * np.pi * 0.02 * t)) / 3
    s = level * (1 + mod * msg) * np.exp(1j * (2 * np.pi * f * t + 0.3 * c))
    return (s + noise * level * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64)


def wide_signal(n, c, level=1.0, cplx=True):
    """Input of the front filters: a narrowband AM station in white noise."""
    x = am_signal(n, c, level=level, f=0.0005 * (1 if c % 2 else -1), noise=1.0)
    return x if cplx else np.ascontiguousarray(x.real)


LEVELS = [0.1, 0.02, 1.0, 0.1, 0.003, 0.5]
OFFSETS = [0.002, -0.002, 0.0011, -0.0011, 0.0005, -0.0031]


# ================================================================ (a) AGC, mixed
def test_agc_mixed(ld, ora):
    """Five AGCs of three bandwidths, one locked, one at another scale, one with a
    past: over the four calls they take different paths at equal n and turn
    speculative on different calls (the tables of many_cases.py, asserted from the
    getter before every call); then a setter on one and a reset on another."""
    nC = len(mc.AGC_BW)
    total = mc.AGC_PRE_N + sum(mc.AGC_CALLS) + sum(mc.AGC_CALLS_AFTER) + FURTHER
    xh = [am_signal(total, c, level=LEVELS[c], f=OFFSETS[c]) for c in range(nC)]
    xd = [dev(x) for x in xh]
    many = [mc.agc(ld, c) for c in range(nC)]
    twin = [mc.agc(ld, c) for c in range(nC)]
    orc = [mc.agc_oracle(ora, c) for c in range(nC)]
    pos = [0] * nC
    c = mc.AGC_PRE
    for g in (many[c], twin[c]):
        g(xd[c][:mc.AGC_PRE_N])
    orc[c](xh[c][:mc.AGC_PRE_N])
    pos[c] = mc.AGC_PRE_N

    def step(n, paths, specs, count):
        d = [g._dispatch(n) for g in many]
        assert [v[0] for v in d] == paths, (n, d)
        if specs is not None:
            for c in range(nC):
                if specs[c] is not None:
                    assert d[c][6] == specs[c], (n, c, d[c])
        assert d == [g._dispatch(n) for g in twin]
        xs = [xd[c][pos[c]:pos[c] + n] for c in range(nC)]
        if count:
            got, rep = counted(ld, lambda: ld.execute_many(many, xs))
            # sizeof(AgcChunksArgs) is 104: up to 16 objects per merged launch, so one
            # launch serves all five (speculative and not, three (W, Wa) pairs)
            assert rep.get("k_agc_chunks") == mc.ceil_div(nC, 16) == 1, rep
        else:
            got = ld.execute_many(many, xs)
        for c in range(nC):
            assert same(got[c], twin[c](xs[c])), (n, c)
            assert same_host(got[c], orc[c](xh[c][pos[c]:pos[c] + n])), (n, c)
            pos[c] += n

    for k, n in enumerate(mc.AGC_CALLS):
        step(n, mc.AGC_PATHS[k], mc.AGC_SPEC[k], count=(k == len(mc.AGC_CALLS) - 1))
    for gs in (many, twin):
        gs[mc.AGC_SETTER_CH].bandwidth = mc.AGC_SETTER_BW
        gs[mc.AGC_RESET_CH].reset()
    orc[mc.AGC_SETTER_CH].bandwidth = np.float32(mc.AGC_SETTER_BW)
    orc[mc.AGC_RESET_CH].reset()
    for k, n in enumerate(mc.AGC_CALLS_AFTER):
        step(n, mc.AGC_PATHS_AFTER[k], mc.AGC_SPEC_AFTER[k], count=False)
    for c in range(nC):
        assert np.float32(many[c].gain) == np.float32(twin[c].gain) == np.float32(orc[c].gain), c
        x = xd[c][pos[c]:pos[c] + FURTHER]
        assert same(many[c](x), twin[c](x)), c


# ================================================================ (b) AmpModem, mixed
def _agcd(ora, n, c):
    """AM brought to unit level by the restatement's AGC (the modem's input in the chain)."""
    g = ora.AGC()
    g.scale = np.float32(1.0)
    return g(am_signal(n + 6000, c, level=LEVELS[c], f=OFFSETS[c]))[6000:]


def test_ampmodem_mixed(ld, ora):
    """Carrier and Costas modems alternate: at 1100 samples the carrier ones are
    chunk-parallel and the Costas ones sequential, at 3000 and 40 000 the Costas
    lists hold two launches more, so every later index is shifted."""
    nC = len(mc.AMP_CARRIER)
    total = sum(mc.AMP_CALLS) + FURTHER
    xh = [_agcd(ora, total, c) for c in range(nC)]
    xd = [dev(x) for x in xh]

    def make(cls=ld.AmpModem):
        return [cls(modulation=mc.AMP_MOD[c], type="dsb", carrier=mc.AMP_CARRIER[c]) for c in range(nC)]

    many, twin = make(), make()
    orc = [ora.AmpModem(mc.AMP_MOD[c], "dsb", mc.AMP_CARRIER[c]) for c in range(nC)]
    pos = 0
    for n in mc.AMP_CALLS:
        for c in range(nC):
            assert many[c]._dispatch(n) == (mc.AMP_PATHS[n][0 if mc.AMP_CARRIER[c] else 1], True)
        xs = [x[pos:pos + n] for x in xd]
        if n == 3000:
            got, rep = counted(ld, lambda: ld.execute_many(many, xs))
            # carrier lists: hist, cand, scan, entries; Costas lists: hist, cand, scan,
            # reflip, scan, entries.  The scans of index 2 -- flag 0 for the carrier
            # objects, 1 for the Costas ones -- are one launch for all six
            # (sizeof(PllScanArgs) is about 150: up to 16 objects), the second Costas
            # scans another; unmerged it would be 3 + 6
            assert rep.get("k_pll_scan") == 2 and rep.get("k_pll_cand") == 1, rep
            assert rep.get("k_pll_reflip") == 1 and rep.get("k_pll_walk", 0) < nC, rep
        else:
            got = ld.execute_many(many, xs)
        for c in range(nC):
            assert same(got[c], twin[c](xs[c])), (n, c)
            assert same_host(got[c], orc[c](xh[c][pos:pos + n])), (n, c)
        pos += n
    for c in range(nC):
        assert many[c].pll_state() == twin[c].pll_state(), c
        x = xd[c][pos:pos + FURTHER]
        assert same(many[c](x), twin[c](x)), c


def test_ampmodem_mixed_with_single_sideband(ld, ora):
    """One usb modem among dsb ones: the whole many-call runs object by object, same bits."""
    kinds = [("dsb", True), ("usb", True), ("dsb", False), ("dsb", True)]
    nC = len(kinds)
    sizes = [3000, 40_000]
    xh = [_agcd(ora, sum(sizes), c) for c in range(nC)]
    xd = [dev(x) for x in xh]
    many = [ld.AmpModem(modulation=0.5, type=t, carrier=car) for t, car in kinds]
    twin = [ld.AmpModem(modulation=0.5, type=t, carrier=car) for t, car in kinds]
    orc = [ora.AmpModem(0.5, t, car) for t, car in kinds]
    assert [m._dispatch(3000)[1] for m in many] == [True, False, True, True]
    pos = 0
    for n in sizes:
        xs = [x[pos:pos + n] for x in xd]
        got, rep = counted(ld, lambda: ld.execute_many(many, xs))
        assert rep.get("k_pll_walk") == nC, rep                # nothing merged: every object runs its own walk
        for c in range(nC):
            assert same(got[c], twin[c](xs[c])), (n, c)
            assert same_host(got[c], orc[c](xh[c][pos:pos + n])), (n, c)
        pos += n


# ================================================================ (c) IIR, mixed
def test_iir_modal_mixed(ld, ora):
    """Six fast-mode filters of three mode counts and five look-back depths: the
    launches of one execute_many follow the grid table of many_cases.py."""
    import torch
    nC = len(mc.MODAL_FILTERS)
    total = sum(mc.MODAL_CALLS) + FURTHER
    scale = [1.0, 1e-3, 500.0, 1.0, 0.05, 1.0]
    xh = [wide_signal(total, c, level=scale[c]) for c in range(nC)]
    xd = [dev(x) for x in xh]
    many = [mc.modal_filter(ld, o, fc) for o, fc, _, _ in mc.MODAL_FILTERS]
    twin = [mc.modal_filter(ld, o, fc) for o, fc, _, _ in mc.MODAL_FILTERS]
    outs = [[] for _ in range(nC)]
    pos = 0
    for n in mc.MODAL_CALLS:
        for c, (_, _, M, J) in enumerate(mc.MODAL_FILTERS):
            assert many[c]._dispatch(n)[0] == "modal" and many[c]._modal_grid(n)[2] == mc.MODAL_GRIDS[n][1][J]
        xs = [x[pos:pos + n] for x in xd]
        got, rep = counted(ld, lambda: ld.execute_many(many, xs))
        # sizeof(IirModalArgs) is 432: 8 objects per merged launch, more than any group here
        assert rep.get("k_iir_modal") == mc.MODAL_LAUNCHES[n], (n, rep)
        for c in range(nC):
            assert same(got[c], twin[c](xs[c])), (n, c)
            outs[c].append(got[c])
        pos += n
    for c, (o, fc, _, _) in enumerate(mc.MODAL_FILTERS):
        ref = mc.modal_oracle(ora, o, fc).execute_f64(xh[c][:pos])
        err = maxrel(torch.cat(outs[c]).cpu().numpy(), ref)
        print(f"order {o} Fc {fc}: {err:.3g}")
        assert err <= 1e-6, (c, err)
        x = xd[c][pos:pos + FURTHER]
        assert same(many[c](x), twin[c](x)), c


@pytest.mark.parametrize("forced", [True, False])
def test_iir_sect_mixed(ld, ora, forced):
    """Exact SOS cascades of orders 8, 8, 12, 14 and 5.  forced: the order-5 filter
    held on the section kernel, so k_iir_sect runs for all and splits by block
    size; otherwise it takes its automatic path, the speculative chunks, and its
    op list has another length and other kernels than the rest."""
    import torch
    nC = len(mc.SECT_ORDERS)
    sizes = [3000, 70_001, FURTHER]
    xh = [wide_signal(sum(sizes), c, level=[1.0, 500.0, 1e-3, 1.0, 0.1][c]) for c in range(nC)]
    xd = [dev(x) for x in xh]

    def make():
        fs = [mc.modal_filter(ld, o, mc.SECT_FC) for o in mc.SECT_ORDERS]
        for f in fs:
            f.exact = True
        if forced:
            fs[-1]._scan_path(1)
        return fs

    many, twin = make(), make()
    assert [f._dispatch(3000)[0] for f in many] == ["seq"] * 4 + ["seq" if forced else "spec"]
    outs = [[] for _ in range(nC)]
    pos = 0
    for n in sizes[:2]:
        xs = [x[pos:pos + n] for x in xd]
        got, rep = counted(ld, lambda: ld.execute_many(many, xs))
        # blocks of 2 x 64 x sections threads: 4, 4, 6, 7 (and 3) sections
        assert rep.get("k_iir_sect") == (mc.SECT_LAUNCHES if forced else mc.SECT_LAUNCHES - 1), rep
        assert (rep.get("k_iir_spec_chunks", 0) == 0) == forced, rep
        for c in range(nC):
            assert same(got[c], twin[c](xs[c])), (n, c)
            outs[c].append(got[c])
        pos += n
    for c, o in enumerate(mc.SECT_ORDERS):
        ref = mc.modal_oracle(ora, o, mc.SECT_FC)(xh[c][:pos])
        assert same_host(torch.cat(outs[c]), ref), c
        x = xd[c][pos:pos + FURTHER]
        assert same(many[c](x), twin[c](x)), c


def test_iir_spec_mixed(ld, ora):
    """Two de-emphasis filters and two one-poles of other warm-up lengths
    (speculative exact chunks, real): the chunk launches split by LDS stage, the
    one-wave verifier is one launch whose objects differ in W and C."""
    import torch
    total = sum(mc.SPEC_CALLS) + FURTHER
    tfs = [ora.deemphasis_coefs(fs) for fs in mc.DEEMPH_RATES] + \
          [(np.float32([1 - r]), np.float32([1, -r])) for r in mc.ONEPOLE_R]
    nC = len(tfs)
    xh = [np.ascontiguousarray(am_signal(total, c, level=[0.5, 1e-3, 500.0, 0.1][c]).real) for c in range(nC)]
    xh[1][1000:2500] = 0.0                                  # a run of exact zeros: the state decays into subnormals
    xd = [dev(x) for x in xh]

    def make():
        return [ld.DeemphasisFilter(fs) for fs in mc.DEEMPH_RATES] + \
               [ld.RIIRFilter(np.float32([1 - r]), np.float32([1, -r])) for r in mc.ONEPOLE_R]

    many, twin = make(), make()
    kinds = [f._dispatch(3000)[2:] for f in many]           # (size class, W, staged)
    assert all(f._dispatch(n)[0] == "spec" for f in many for n in mc.SPEC_CALLS)
    assert kinds[0] == kinds[1] and len(set(kinds)) == 3
    outs = [[] for _ in range(nC)]
    pos = 0
    for n in mc.SPEC_CALLS:
        xs = [x[pos:pos + n] for x in xd]
        got, rep = counted(ld, lambda: ld.execute_many(many, xs))
        assert rep.get("k_iir_spec_chunks") == 3 and rep.get("k_iir_spec_verify") == 1, rep
        for c in range(nC):
            assert same(got[c], twin[c](xs[c])), (n, c)
            outs[c].append(got[c])
        pos += n
    for c in range(nC):
        ref = ora.IIRFilter(tf=tfs[c], cplx=False)(xh[c][:pos])
        assert same_host(torch.cat(outs[c]), ref), c
        x = xd[c][pos:pos + FURTHER]
        assert same(many[c](x), twin[c](x)), c


def test_iir_exact_switched_between_calls(ld, ora):
    """One filter set to exact between two many-calls: its state is converted
    inside the recording and its list is the section kernel's, the others stay modal."""
    import torch
    cases = mc.MODAL_FILTERS[:3]
    nC, n = len(cases), 40_000
    xh = [wide_signal(2 * n + FURTHER, c) for c in range(nC)]
    xd = [dev(x) for x in xh]
    many = [mc.modal_filter(ld, o, fc) for o, fc, _, _ in cases]
    twin = [mc.modal_filter(ld, o, fc) for o, fc, _, _ in cases]
    first = ld.execute_many(many, [x[:n] for x in xd])
    ref1 = [twin[c](xd[c][:n]) for c in range(nC)]
    many[1].exact = True
    twin[1].exact = True
    assert [f._dispatch(n)[0] for f in many] == ["modal", "seq", "modal"]
    second, rep = counted(ld, lambda: ld.execute_many(many, [x[n:2 * n] for x in xd]))
    assert rep.get("k_iir_modal") == 1 and rep.get("k_iir_sect") == 1, rep
    for c in range(nC):
        assert same(first[c], ref1[c]), c
        assert same(second[c], twin[c](xd[c][n:2 * n])), c
        x = xd[c][2 * n:]
        assert same(many[c](x), twin[c](x)), c
    for c in (0, 2):
        o, fc = cases[c][:2]
        ref = mc.modal_oracle(ora, o, fc).execute_f64(xh[c][:2 * n])
        assert maxrel(torch.cat([first[c], second[c]]).cpu().numpy(), ref) <= 1e-6, c
    o, fc = cases[1][:2]
    assert maxrel(first[1].cpu().numpy(), mc.modal_oracle(ora, o, fc).execute_f64(xh[1][:n])) <= 1e-6


# ================================================================ (d) filter_resample_many, mixed
@pytest.mark.parametrize("cplx", [True, False])
def test_filter_resample_many_mixed(ld, ora, cplx):
    """Fused fronts of three rates and three filters, one with a past: the
    resampler phases and output counts differ inside one merged launch, and the
    output capacity is the largest count."""
    import torch
    nC = len(mc.FRONT)
    total = mc.FRONT_PRE_N + sum(mc.FRONT_CALLS) + FURTHER
    xh = [wide_signal(total, c, level=[1.0, 500.0, 1e-3, 1.0][c], cplx=cplx) for c in range(nC)]
    xd = [dev(x) for x in xh]

    def make():
        return ([mc.modal_filter(ld, 8, fc, cplx) for fc, _ in mc.FRONT],
                [mc.resampler(ld, rate, cplx) for _, rate in mc.FRONT])

    fm, rm = make()
    ft, rt = make()
    pos = [0] * nC
    c = mc.FRONT_PRE_CH
    pre = ld.filter_resample(fm[c], rm[c], xd[c][:mc.FRONT_PRE_N])
    assert same(pre, ld.filter_resample(ft[c], rt[c], xd[c][:mc.FRONT_PRE_N])) and pre.numel() > 0
    pos[c] = mc.FRONT_PRE_N
    outs = [[] for _ in range(nC)]
    for n in mc.FRONT_CALLS:
        xs = [xd[c][pos[c]:pos[c] + n] for c in range(nC)]
        got, rep = counted(ld, lambda: ld.filter_resample_many(fm, rm, xs))
        if n == 0:
            assert all(g.numel() == 0 for g in got) and not rep.get("k_iir_modal_rs"), rep
        else:
            # J = 7, 13, 3, 7: one grid at 35 and 2 units (one-XCD), 128 and 1024 at 128 units;
            # sizeof(IirModalArgs) is 432 (8 objects per launch)
            assert rep.get("k_iir_modal_rs") == (2 if n == 262_144 else 1), (n, rep)
            assert rep.get("k_iir_resamp_edges") == 1, (n, rep)
            counts = [g.numel() for g in got]
            assert counts[0] < counts[1] < counts[2] and counts[3] in (counts[0] - 1, counts[0], counts[0] + 1)
        for c in range(nC):
            assert same(got[c], ld.filter_resample(ft[c], rt[c], xs[c])), (n, c)
            outs[c].append(got[c])
            pos[c] += n
    for c, (fc, rate) in enumerate(mc.FRONT):
        f64 = mc.modal_oracle(ora, 8, fc, cplx).execute_f64(xh[c][:pos[c]])
        ref = mc.resampler_oracle(ora, rate, cplx)(f64)
        if c == mc.FRONT_PRE_CH:
            ref = ref[pre.numel():]                          # the outputs of its own first call
        y = torch.cat(outs[c]).cpu().numpy()
        assert y.shape == ref.shape, (c, y.shape, ref.shape)
        assert maxrel(y, ref) <= 1e-6, (c, maxrel(y, ref))
    for c in range(nC):                                      # the empty call changed no state
        x = xd[c][pos[c]:pos[c] + FURTHER]
        assert same(ld.filter_resample(fm[c], rm[c], x), ld.filter_resample(ft[c], rt[c], x)), c


# ================================================================ the whole chain
class Radio:
    """The AMRadio chain of test_gpu_many.py: fused front, AGC, AmpModem, de-emphasis."""

    def __init__(self, L, exact=False):
        self.iir = mc.modal_filter(L, 8, 0.0075)
        self.iir.exact = exact
        self.rs = mc.resampler(L, 0.024)
        self.agc = L.AGC()
        self.agc.scale = 0.01
        self.am = L.AmpModem(modulation=0.5, type="dsb", carrier=True)
        self.de = L.DeemphasisFilter(48000)

    def back(self, x):
        return self.de(self.am(self.agc(x)))

    def __call__(self, L, x):
        return self.back(L.filter_resample(self.iir, self.rs, x))


def many_front(L, radios, xs):
    return L.filter_resample_many([r.iir for r in radios], [r.rs for r in radios], xs)


def many_back(L, radios, xs):
    a = L.execute_many([r.agc for r in radios], xs)
    b = L.execute_many([r.am for r in radios], a)
    return L.execute_many([r.de for r in radios], b)


def oracle_back(ora, x, scale=0.01):
    g = ora.AGC()
    g.scale = np.float32(scale)
    am = ora.AmpModem(0.5, "dsb", True)
    de = ora.IIRFilter(tf=ora.deemphasis_coefs(48000.0), cplx=False)
    return de(am(g(x)))


# ================================================================ (e) cap splits
@pytest.mark.parametrize("nC", mc.CAP_C)
def test_cap_splits(ld, ora, nC):
    """1, 2, 9 (8 + 1) and 17 (16 + 1) channels: groups split unevenly at the
    argument cap of a merged launch, min(16, 3584 / sizeof(arguments))."""
    n = mc.CAP_N
    many = [Radio(ld) for _ in range(nC)]
    twin = [Radio(ld) for _ in range(nC)]
    xf = [wide_signal(n, c) for c in range(nC)]
    xb = [am_signal(n, c, level=LEVELS[c % 6], f=OFFSETS[c % 6]) for c in range(nC)]
    xfd, xbd = [dev(x) for x in xf], [dev(x) for x in xb]
    front, rep = counted(ld, lambda: many_front(ld, many, xfd))
    # sizeof(IirModalArgs) is 432: 3584 / 432 = 8 objects per launch
    assert rep.get("k_iir_modal_rs") == mc.ceil_div(nC, 8), rep
    a, rep = counted(ld, lambda: ld.execute_many([r.agc for r in many], xbd))
    # sizeof(AgcChunksArgs) is 104 and sizeof(DelayHistArgs) 40: 16 objects per launch
    assert rep.get("k_agc_chunks") == mc.ceil_div(nC, 16) and rep.get("k_delay_hist") == mc.ceil_div(nC, 16), rep
    b, rep = counted(ld, lambda: ld.execute_many([r.am for r in many], a))
    # the walk's arguments allow between 9 and 16 objects per launch
    assert rep.get("k_pll_walk") == (2 if nC == 17 else 1) and rep.get("k_delay_hist") == mc.ceil_div(nC, 16), rep
    back = ld.execute_many([r.de for r in many], b)
    for c in range(nC):
        assert same(front[c], ld.filter_resample(twin[c].iir, twin[c].rs, xfd[c])), c
        assert same(back[c], twin[c].back(xbd[c])), c
        assert many[c].am.pll_state() == twin[c].am.pll_state(), c
        assert np.float32(many[c].agc.gain) == np.float32(twin[c].agc.gain), c
    for c in sorted({0, nC - 1}):
        assert same_host(back[c], oracle_back(ora, xb[c])), c
        ref = mc.resampler_oracle(ora, 0.024)(mc.modal_oracle(ora, 8, 0.0075).execute_f64(xf[c]))
        assert maxrel(front[c].cpu().numpy(), ref) <= 1e-6, c
    x2f = [dev(wide_signal(FURTHER, 40 + c)) for c in range(nC)]
    x2b = [dev(am_signal(FURTHER, 40 + c)) for c in range(nC)]
    f2, b2 = many_front(ld, many, x2f), many_back(ld, many, x2b)
    for c in range(nC):
        assert same(f2[c], ld.filter_resample(twin[c].iir, twin[c].rs, x2f[c])), c
        assert same(b2[c], twin[c].back(x2b[c])), c


# ================================================================ (f) streams
def test_streams_alternate(ld, ora):
    """Even steps are many-calls on one stream, odd steps per-object calls on four
    other streams, with no host synchronisation in between: the objects' own
    cross-stream marks and waits are recorded (op kinds 1 and 2) and issued by the
    many-call."""
    import torch
    nC, n, steps = 4, 40_000, 6
    xh = [wide_signal(n * steps, c, level=[1.0, 0.05, 20.0, 1.0][c]) for c in range(nC)]
    xd = [dev(x) for x in xh]
    many = [Radio(ld) for _ in range(nC)]
    twin = [Radio(ld) for _ in range(nC)]
    s0 = torch.cuda.Stream()
    own = [torch.cuda.Stream() for _ in range(nC)]
    torch.cuda.synchronize()
    got = [[] for _ in range(nC)]
    keep = []                                                # intermediates stay alive until the end
    for k in range(steps):
        blk = [x[k * n:(k + 1) * n] for x in xd]
        if k % 2 == 0:
            with torch.cuda.stream(s0):
                f = many_front(ld, many, blk)
                a = ld.execute_many([r.agc for r in many], f)
                b = ld.execute_many([r.am for r in many], a)
                y = ld.execute_many([r.de for r in many], b)
            keep += [f, a, b]
            for c in range(nC):
                got[c].append(y[c])
        else:
            for c in range(nC):
                with torch.cuda.stream(own[c]):
                    got[c].append(many[c](ld, blk[c]))
    torch.cuda.synchronize()
    for c in range(nC):
        ref = torch.cat([twin[c](ld, xd[c][k * n:(k + 1) * n]) for k in range(steps)])
        torch.cuda.synchronize()
        assert same(torch.cat(got[c]), ref), c
        assert many[c].am.pll_state() == twin[c].am.pll_state(), c


# ================================================================ (g) error in the middle
def test_error_in_the_middle_of_a_many_call(ld):
    """ldsp_iirfilt_resamp_execute_many with channel 1's output count above cap:
    LDSP_ERANGE; channel 0 has advanced by exactly one call (its device work was
    issued), channels 1 and 2 are untouched.  The range check precedes any device
    work of the failing channel."""
    import torch
    lib = C.CDLL(os.path.join(os.path.dirname(ld.__file__), "..", "libldsp.so"))
    vp, sz = C.c_void_p, C.c_size_t
    lib.ldsp_iirfilt_create_prototype.argtypes = [C.c_int, C.c_int, C.c_uint, C.c_float, C.c_float, C.c_float,
                                                  C.c_float, C.c_int, C.POINTER(vp)]
    lib.ldsp_resamp_create.argtypes = [C.c_float, C.c_uint, C.c_float, C.c_float, C.c_uint, C.c_int, C.POINTER(vp)]
    lib.ldsp_iirfilt_resamp_execute.argtypes = [vp, vp, vp, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    lib.ldsp_iirfilt_resamp_execute_many.argtypes = [C.POINTER(vp), C.POINTER(vp), C.POINTER(vp), sz, C.POINTER(vp),
                                                     sz, C.POINTER(sz), C.c_int, vp]
    lib.ldsp_iirfilt_destroy.argtypes = [vp]
    lib.ldsp_resamp_destroy.argtypes = [vp]
    lib.ldsp_stream_synchronize.argtypes = [vp]
    nC, n1, n2, ld_out = 3, 40_000, 3000, 20_064
    rates = [0.024, 0.5, 0.024]
    LDSP_ERANGE, DEVICE = -4, 1

    def make():
        qs, rs = [], []
        for rate in rates:
            q, r = vp(), vp()
            assert lib.ldsp_iirfilt_create_prototype(2, 0, 8, 0.0075, 0.3, 0.7, 60.0, 1, C.byref(q)) == 0
            assert lib.ldsp_resamp_create(rate, 20, min(rate, 0.4), 60.0, 13, 1, C.byref(r)) == 0
            qs.append(q)
            rs.append(r)
        return qs, rs

    qm, rm = make()
    qt, rt = make()
    xd = [dev(wide_signal(n1 + n2, c)) for c in range(nC)]
    fill = complex(7, -3)

    def buffers():
        return torch.full((nC, ld_out), fill, dtype=torch.complex64, device="cuda")

    def arr(vals):
        return (vp * nC)(*vals)

    def many(off, n, cap, y):
        nout = (sz * nC)(*([99_999] * nC))
        torch.cuda.synchronize()
        rc = lib.ldsp_iirfilt_resamp_execute_many(arr([q.value for q in qm]), arr([r.value for r in rm]),
                                                  arr([x.data_ptr() + 8 * off for x in xd]), n,
                                                  arr([y[c].data_ptr() for c in range(nC)]), cap, nout, nC, None)
        assert lib.ldsp_stream_synchronize(None) == 0
        return rc, list(nout)

    def single(c, off, n, y):
        k = sz(0)
        torch.cuda.synchronize()
        assert lib.ldsp_iirfilt_resamp_execute(qt[c], rt[c], xd[c].data_ptr() + 8 * off, n, y[c].data_ptr(), ld_out,
                                               C.byref(k), DEVICE, None) == 0
        assert lib.ldsp_stream_synchronize(None) == 0
        return k.value

    y1, t1 = buffers(), buffers()
    rc, nout = many(0, n1, 1000, y1)                         # K = 960, 20 000, 960 against cap 1000
    assert rc == LDSP_ERANGE
    k0 = single(0, 0, n1, t1)
    assert nout[0] == k0 and 900 < k0 <= 1000 and 19_999 <= nout[1] <= 20_001 and nout[2] == 99_999
    assert same(y1[0], t1[0])                                # channel 0 ran, the rest of its row is untouched
    assert bool((y1[1:] == fill).all())                      # nothing written for channels 1 and 2
    y2, t2 = buffers(), buffers()
    rc, nout = many(n1, n2, ld_out, y2)
    assert rc == 0
    for c in range(nC):                                      # twins 1 and 2 never saw the failed call
        assert single(c, n1, n2, t2) == nout[c] > 0
        assert same(y2[c], t2[c]), c
    for q in qm + qt:
        assert lib.ldsp_iirfilt_destroy(q) == 0
    for r in rm + rt:
        assert lib.ldsp_resamp_destroy(r) == 0


# ================================================================ (i) irregular signals, single objects
IRREGULAR = ["zeros", "noise", "strong", "start", "stop"]
IRR_CALLS = [40_000, 1100]


@pytest.fixture(scope="module")
def irregular(ora):
    """The irregular signals and the restatement's output of every stage, computed
    once: x -> AGC -> AmpModem (carrier, Costas) -> de-emphasis, and x -> exact cheby2."""
    n = sum(IRR_CALLS)
    rng = np.random.default_rng(77)
    am = am_signal(n, 1, level=0.1)
    z = np.zeros(20_000, np.complex64)
    sig = {"zeros": np.zeros(n, np.complex64),
           "noise": (1e-7 * (rng.standard_normal(n) + 1j * rng.standard_normal(n))).astype(np.complex64),
           "strong": (am * np.float32(500)).astype(np.complex64),
           "start": np.concatenate([z, am[:n - z.size]]),
           "stop": np.concatenate([am[:n - z.size], z])}
    out = {}
    for name, x in sig.items():
        g = ora.AGC()
        g.scale = np.float32(0.01)
        d = {"x": x, "agc": g(x), "gain": g.gain}
        for mode, carrier in (("carrier", True), ("costas", False)):
            m = ora.AmpModem(0.5, "dsb", carrier)
            d[mode] = m(d["agc"])
            d[mode + "_pll"] = m.pll_state
        d["de"] = ora.IIRFilter(tf=ora.deemphasis_coefs(48000.0), cplx=False)(d["carrier"])
        d["iir"] = mc.modal_oracle(ora, 8, 0.02)(x)
        for k in ("agc", "carrier", "costas", "de", "iir"):
            assert np.isfinite(d[k].view(np.float32)).all(), (name, k)
        out[name] = d
    # what makes these signals worth running: the AGC's gain collapses into
    # subnormals when a signal arrives after silence, the filters' states decay
    # into them when it stops, and silence stays exactly zero
    assert subnormals(out["start"]["agc"]) > 1000 and subnormals(out["start"]["de"]) > 1000
    assert subnormals(out["stop"]["iir"]) > 1000
    assert not out["zeros"]["de"].any() and not out["zeros"]["agc"].any()
    return out


def _calls(fn, x):
    import torch
    xd = dev(x)
    outs, pos = [], 0
    for n in IRR_CALLS:
        outs.append(fn(xd[pos:pos + n]))
        pos += n
    return torch.cat(outs)


@pytest.mark.parametrize("name", IRREGULAR)
def test_irregular_agc(ld, irregular, name):
    d = irregular[name]
    g = ld.AGC()
    g.scale = 0.01
    assert [g._dispatch(n)[0] for n in IRR_CALLS] == ["par", "small"]
    assert same_host(_calls(g, d["x"]), d["agc"])
    assert np.float32(g.gain) == np.float32(d["gain"])


@pytest.mark.parametrize("mode", ["carrier", "costas"])
@pytest.mark.parametrize("name", IRREGULAR)
def test_irregular_ampmodem(ld, irregular, name, mode):
    d = irregular[name]
    m = ld.AmpModem(modulation=0.5, type="dsb", carrier=(mode == "carrier"))
    assert [m._dispatch(n)[0] for n in IRR_CALLS] == ["par", "par" if mode == "carrier" else "seq"]
    assert same_host(_calls(m, d["agc"]), d[mode])
    assert m.pll_state() == d[mode + "_pll"]


@pytest.mark.parametrize("name", IRREGULAR)
def test_irregular_exact_filters(ld, irregular, name):
    d = irregular[name]
    f = mc.modal_filter(ld, 8, 0.02)
    f.exact = True
    assert f._dispatch(40_000)[:2] == ("seq", 1024)          # k_iir_sect
    assert same_host(_calls(f, d["x"]), d["iir"])
    assert same_host(_calls(ld.DeemphasisFilter(48000), d["carrier"]), d["de"])


# ================================================================ (h) channelizer rows
ROW_STRONG, ROW_WEAK, ROW_START, ROW_STOP, ROW_PLAIN, ROW_NOISE = 1, 3, 5, 7, 12, 13
ROWS_ZERO = [8, 9, 10]
ROW_CUTS = [(0, 25_000), (25_000, 40_000)]
ROW_FRONT = (0.02, 0.5)                                   # cheby2 order 8 at Fc 0.02 (J = 3), resampler rate 0.5


def _row_oracle(ora, x, exact):
    f = mc.modal_oracle(ora, 8, ROW_FRONT[0])
    r = mc.resampler_oracle(ora, ROW_FRONT[1])
    g = ora.AGC()
    g.scale = np.float32(0.01)
    am = ora.AmpModem(0.5, "dsb", True)
    de = ora.IIRFilter(tf=ora.deemphasis_coefs(48000.0), cplx=False)
    front, pcm = [], []
    for a, b in ROW_CUTS:
        front.append(r(f(x[a:b]) if exact else f.execute_f64(x[a:b])))
        pcm.append(de(am(g(front[-1]))))
    return np.concatenate(front), np.concatenate(pcm)


@pytest.fixture(scope="module")
def rows(ld, ora):
    """One 16 x 40 000 capture out of Channelizer(16, 8): a strong station (times
    500), a weak one, one that starts half-way, one that stops half-way and a
    plain one, in noise at 1e-7.  After the channelizer the silent halves of the
    starting and stopping rows and three whole rows are written to exact zeros,
    and one row to noise alone (the strong station's stop-band leakage and the
    noise floor never give exact silence; a gated source does).  The restatement
    runs the exact chain on every row."""
    M, D, ncol = 16, 8, 40_000
    N = D * ncol
    rng = np.random.default_rng(2024)
    t = np.arange(N)

    def station(k, level, c):
        msg = (np.sin(2 * np.pi * 0.0031 / D * t + c) + np.sin(2 * np.pi * 0.0083 / D * t)) / 2
        return level * (1 + 0.5 * msg) * np.exp(2j * np.pi * ((k / M + (0.002 if c % 2 else -0.002) / D) * t))

    half = (t >= N // 2)
    x = (station(ROW_STRONG, 500 * 0.1, 0) + station(ROW_WEAK, 0.01 * 0.1, 1) + station(ROW_START, 1.0, 2) * half
         + station(ROW_STOP, 1.0, 3) * ~half + station(ROW_PLAIN, 0.1, 4)
         + 1e-7 * (rng.standard_normal(N) + 1j * rng.standard_normal(N))).astype(np.complex64)
    y = ld.Channelizer(M, D)(dev(x)).clone()
    assert tuple(y.shape) == (M, ncol)
    y[ROWS_ZERO] = 0
    y[ROW_START, :ncol // 2] = 0
    y[ROW_STOP, ncol // 2:] = 0
    y[ROW_NOISE] = dev((1e-7 * (rng.standard_normal(ncol) + 1j * rng.standard_normal(ncol))).astype(np.complex64))
    yh = y.cpu().numpy()
    level = np.abs(yh).max(axis=1)
    # the strong station towers over every other row (whose peaks are its start-up transient and leakage)
    assert level[ROW_STRONG] > 5 * np.delete(level, ROW_STRONG).max() and level[ROW_PLAIN] > 0
    assert 0 < level[ROW_NOISE] < 1e-6 and not level[ROWS_ZERO].any()
    ref = [_row_oracle(ora, yh[k], True) for k in range(M)]
    # the conditions that make the capture worth running, on the restatement's outputs
    for k in range(M):
        assert np.isfinite(ref[k][0].view(np.float32)).all() and np.isfinite(ref[k][1]).all(), k
    counts = {k: subnormals(ref[k][1]) for k in (ROW_START, ROW_STOP)}
    print("subnormal PCM samples:", counts)
    assert counts[ROW_START] > 0 and counts[ROW_STOP] > 0, counts
    for k in ROWS_ZERO:
        assert not ref[k][1].any(), k
    return y, yh, ref


@pytest.mark.parametrize("exact", [True, False])
def test_channelizer_rows(ld, ora, rows, exact):
    """The rows through filter_resample_many and the back half via execute_many in
    two calls, against per-channel calls; the exact chain bit for bit against the
    restatement on every row, the fast front within 1e-6 on the irregular rows."""
    import torch
    y, yh, ref = rows
    M = y.shape[0]
    many = [Radio(ld, exact) for _ in range(M)]
    twin = [Radio(ld, exact) for _ in range(M)]
    for r in many + twin:
        r.iir = mc.modal_filter(ld, 8, ROW_FRONT[0])
        r.iir.exact = exact
        r.rs = mc.resampler(ld, ROW_FRONT[1])
    front, pcm = [[] for _ in range(M)], [[] for _ in range(M)]
    for i, (a, b) in enumerate(ROW_CUTS):
        xs = [y[k, a:b] for k in range(M)]
        f, rep = counted(ld, lambda: many_front(ld, many, xs))
        if not exact:
            # sizeof(IirModalArgs) is 432: 8 objects per merged launch
            assert rep.get("k_iir_modal_rs") == mc.ceil_div(M, 8), rep
        p = many_back(ld, many, f)
        for k in range(M):
            tf = ld.filter_resample(twin[k].iir, twin[k].rs, xs[k].clone())
            assert same(f[k], tf), (i, k)
            assert same(p[k], twin[k].back(tf)), (i, k)
            front[k].append(f[k])
            pcm[k].append(p[k])
    for k in range(M):
        assert many[k].am.pll_state() == twin[k].am.pll_state(), k
        assert np.float32(many[k].agc.gain) == np.float32(twin[k].agc.gain), k
    if exact:
        for k in range(M):
            assert same_host(torch.cat(front[k]), ref[k][0]), k
            assert same_host(torch.cat(pcm[k]), ref[k][1]), k
    else:
        for k in (ROW_STRONG, ROW_WEAK, ROW_START, ROW_STOP, ROW_NOISE):
            want = _row_oracle(ora, yh[k], False)[0]
            err = maxrel(torch.cat(front[k]).cpu().numpy(), want)
            print(f"row {k}: {err:.3g}")
            assert err <= 1e-6, (k, err)
        for k in ROWS_ZERO:
            assert not torch.cat(pcm[k]).any(), k
