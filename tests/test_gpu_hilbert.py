"""SSBDemod and HilbertTransform on the GPU (reference src/demod.hpp:155-187,
src/utility.hpp:71-108 -> liquid firhilbf_c2r / r2c / decim / interp_execute),
bit for bit against the restatement's FirHilb.c2r, which yields every reference
the four operations need (M = semi-length, hq = the 2M taps, zero history):

  c2r     (lower, upper) = FirHilb.c2r(x)
  r2c     imag = FirHilb.c2r(1j * x)[0] (the delayed real part is 0 there, and the
          restatement's sum starts from +0, so it never yields -0); real = x
          delayed by 2M
  decim   the r2c reference at [1::2]
  interp  [0::2] = im x delayed by M; [1::2] = FirHilb.c2r(z)[0][1::2] with
          z[2k] = 1j * re x[k], z[2k + 1] = 0

Streams are cut into calls at the history edge (H = 4M - 1 input samples;
interp 2M - 1) and at the kernel's tile edge.  Parity unpinned, like the rest
of the oracle (firhilb.proto.c is restated from the recalled liquid source)."""
import numpy as np
import pytest

from conftest import cgauss

pytestmark = pytest.mark.gpu

R2C, C2R, DECIM, INTERP = 0, 1, 2, 3
MS = (2, 5, 25, 64)


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def assert_bitwise(y, ref):
    assert y.dtype == ref.dtype and y.shape == ref.shape, (y.dtype, ref.dtype, y.shape, ref.shape)
    eq = bits(y) == bits(ref)
    if not eq.all():
        i = int(np.argmin(eq))
        raise AssertionError(f"{(~eq).sum()} of {eq.size} words differ; first at word {i}")


def delayed(v, d):
    return np.concatenate([np.zeros(d, v.dtype), v])[:v.size]


def edges(lens, total):
    """Call boundaries: the given lengths in turn, then the rest of the stream."""
    e = [0]
    for c in lens:
        e.append(e[-1] + c)
    assert e[-1] < total, (e, total)
    return e + [total]


def ragged(fn, x, lens, per_in=1):
    """fn over x cut at edges(lens); x counts per_in samples per unit of lens."""
    e = edges(lens, x.size // per_in)
    return [fn(x[a * per_in:b * per_in]) for a, b in zip(e[:-1], e[1:])]


# ---------------------------------------------------------------- references (computed once, never modified)
N = 12_000                                       # > 1 + (H - 1) + H + (H + 1) + 3 T + 2 at M = 64 (H = 255, T = 2048)


@pytest.fixture(scope="module")
def data(ora):
    rng = np.random.default_rng(4321)
    xc = cgauss(rng, N)
    xr = rng.standard_normal(N).astype(np.float32)
    xc.setflags(write=False)
    xr.setflags(write=False)
    return xc, xr


@pytest.fixture(scope="module")
def refs(ora, data):
    xc, xr = data
    out = {}
    for m in MS:
        lo, up = ora.FirHilb(m, 60.0).c2r(xc)
        z = np.zeros(N, np.complex64)
        z.imag = xr
        r2c = np.empty(N, np.complex64)
        r2c.real = delayed(xr, 2 * m)
        r2c.imag = ora.FirHilb(m, 60.0).c2r(z)[0]
        z2 = np.zeros(2 * N, np.complex64)
        z2.imag[0::2] = xc.real
        itp = np.empty(2 * N, np.float32)
        itp[0::2] = delayed(np.ascontiguousarray(xc.imag), m)
        itp[1::2] = ora.FirHilb(m, 60.0).c2r(z2)[0][1::2]
        out[m] = {"c2r": (lo, up), "r2c": r2c, "decim": np.ascontiguousarray(r2c[1::2]), "interp": itp}
        for v in (lo, up, r2c, out[m]["decim"], itp):
            v.setflags(write=False)
    return out


def cut_lengths(ld, m, op):
    """n = 0 and 1, the history edge H - 1, H, H + 1 and the tile edge T - 1, T, T + 1."""
    H = 2 * m - 1 if op == INTERP else 4 * m - 1
    T = ld._hilbert_tile(op)
    assert T + 1 + 3 * H < N // 2
    return [0, 1, H - 1, H, H + 1, T - 1, T, T + 1, 0, 1]


# ---------------------------------------------------------------- SSBDemod
@pytest.fixture(scope="module")
def ssb_ref(ora):
    rng = np.random.default_rng(99)
    x = cgauss(rng, 6000)
    lo, up = ora.FirHilb(25, 60.0).c2r(x)
    for v in (x, lo, up):
        v.setflags(write=False)
    return x, {"lsb": lo, "usb": up}


@pytest.mark.parametrize("band", ["usb", "lsb"])
def test_ssb_one_call_ragged_and_reset(ld, ssb_ref, band):
    x, ref = ssb_ref
    g = ld.SSBDemod(band)
    y = g(x)
    assert y.dtype == np.float32
    assert_bitwise(y, ref[band])
    g.reset()
    assert_bitwise(g(x[:2500]), ref[band][:2500])            # reset() restores the first-call output
    # H = 99: the cuts land at the history edge
    g = ld.SSBDemod(band)
    assert_bitwise(np.concatenate(ragged(g, x, [1, 2, 98, 99, 100, 1])), ref[band])


def test_ssb_other_band_strings_select_the_lower_sideband(ld, ssb_ref):
    x, ref = ssb_ref
    assert_bitwise(ld.SSBDemod("USB")(x[:500]), ref["lsb"][:500])      # demod.hpp:162: band == "usb"


def test_ssb_two_streams_and_device_tensors(ld, ssb_ref):
    import torch
    x, ref = ssb_ref
    g = ld.SSBDemod("usb")
    xd = torch.from_numpy(np.array(x)).cuda()
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    cuts = [0, 1000, 1050, 3099, 3100, 5147, len(x)]
    outs = []
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        with torch.cuda.stream(streams[i % 2]):
            outs.append(g(xd[a:b]))
    torch.cuda.synchronize()
    assert all(t.is_cuda and t.dtype == torch.float32 for t in outs)
    assert_bitwise(np.concatenate([t.cpu().numpy() for t in outs]), ref["usb"])


def test_ssb_many_workgroups(ld, ora):
    rng = np.random.default_rng(5)
    x = cgauss(rng, 200_000)
    lo, up = ora.FirHilb(25, 60.0).c2r(x)
    assert_bitwise(ld.SSBDemod("usb")(x), up)
    assert_bitwise(ld.SSBDemod("lsb")(x), lo)


def test_ssb_equals_suppressed_carrier_ampmodem(ld, ssb_ref):
    # no oracle in the loop: with mod_index = 0.5 AmpModem's 0.5 * s / 0.5 is exact
    # (no denormal outputs on this input), and its suppressed-carrier usb path is the c2r alone
    x, ref = ssb_ref
    y = ld.SSBDemod("usb")(x)
    assert np.abs(y[y != 0]).min() > 1e-30
    assert_bitwise(y, ld.AmpModem(modulation=0.5, type="usb", carrier=False)(x))


# ---------------------------------------------------------------- HilbertTransform
@pytest.mark.parametrize("m", MS)
def test_c2r(ld, data, refs, m):
    xc, _ = data
    lo, up = refs[m]["c2r"]
    y = ld.HilbertTransform(m).c2r(xc)
    assert isinstance(y, tuple) and len(y) == 2
    assert_bitwise(y[0], lo)
    assert_bitwise(y[1], up)
    h = ld.HilbertTransform(m)
    parts = ragged(h.c2r, xc, cut_lengths(ld, m, C2R))
    assert_bitwise(np.concatenate([p[0] for p in parts]), lo)
    assert_bitwise(np.concatenate([p[1] for p in parts]), up)


@pytest.mark.parametrize("m", MS)
def test_r2c(ld, data, refs, m):
    _, xr = data
    assert_bitwise(ld.HilbertTransform(m).r2c(xr), refs[m]["r2c"])
    h = ld.HilbertTransform(m)
    assert_bitwise(np.concatenate(ragged(h.r2c, xr, cut_lengths(ld, m, R2C))), refs[m]["r2c"])


@pytest.mark.parametrize("m", MS)
def test_decim(ld, data, refs, m):
    _, xr = data
    ref = refs[m]["decim"]
    y = ld.HilbertTransform(m)(xr)                            # float32 -> decim
    assert y.dtype == np.complex64 and y.size == N // 2
    assert_bitwise(y, ref)
    # the cuts rounded to even lengths (n = 0 and 2 for the shortest)
    lens = [2 * ((c + 1) // 2) for c in cut_lengths(ld, m, DECIM)]
    h = ld.HilbertTransform(m)
    assert_bitwise(np.concatenate(ragged(h.decim, xr, lens)), ref)


@pytest.mark.parametrize("m", MS)
def test_interp(ld, data, refs, m):
    xc, _ = data
    ref = refs[m]["interp"]
    y = ld.HilbertTransform(m)(xc)                            # complex64 -> interp
    assert y.dtype == np.float32 and y.size == 2 * N
    assert_bitwise(y, ref)
    h = ld.HilbertTransform(m)
    assert_bitwise(np.concatenate(ragged(h.interp, xc, cut_lengths(ld, m, INTERP))), ref)


def test_decim_odd_length_leaves_the_state_untouched(ld, data, refs):
    _, xr = data
    ref = refs[5]["decim"]
    h = ld.HilbertTransform(5)
    a = h.decim(xr[:1000])
    with pytest.raises(ValueError):
        h.decim(xr[1000:1333])
    with pytest.raises(ValueError):
        h(xr[1000:1001])
    b = h.decim(xr[1000:])                                    # the next even call continues the stream
    assert_bitwise(np.concatenate([a, b]), ref)


def test_directions_keep_separate_state_and_reset(ld, data, refs):
    xc, xr = data
    h = ld.HilbertTransform(5)
    n = 3000
    y = [h.interp(xc[:n]), h.decim(xr[:n]), h.r2c(xr[:n]), h.c2r(xc[:n])[1]]
    y2 = [h.interp(xc[n:]), h.decim(xr[n:]), h.r2c(xr[n:]), h.c2r(xc[n:])[1]]
    want = [refs[5]["interp"], refs[5]["decim"], refs[5]["r2c"], refs[5]["c2r"][1]]
    for a, b, r in zip(y, y2, want):
        assert_bitwise(np.concatenate([a, b]), r)
    h.reset()
    assert_bitwise(h.interp(xc[:n]), refs[5]["interp"][:2 * n])
    assert_bitwise(h.decim(xr[:n]), refs[5]["decim"][:n // 2])
    assert_bitwise(h.r2c(xr[:n]), refs[5]["r2c"][:n])
    assert_bitwise(h.c2r(xc[:n])[0], refs[5]["c2r"][0][:n])


def test_device_tensors(ld, data, refs):
    import torch
    xc, xr = data
    h = ld.HilbertTransform(25)
    dc = torch.from_numpy(np.array(xc)).cuda()
    dr = torch.from_numpy(np.array(xr)).cuda()
    k = 4097                                                  # the second call starts at an odd offset
    lo = [h.c2r(dc[:k]), h.c2r(dc[k:])]
    got = {"interp": torch.cat([h(dc[:k]), h(dc[k:])]),
           "decim": torch.cat([h(dr[:k - 1]), h(dr[k - 1:])]),
           "r2c": torch.cat([h.r2c(dr[:k]), h.r2c(dr[k:])])}
    torch.cuda.synchronize()
    for name, t in got.items():
        assert t.is_cuda
        assert_bitwise(t.cpu().numpy(), refs[25][name])
    for i in (0, 1):
        assert_bitwise(torch.cat([lo[0][i], lo[1][i]]).cpu().numpy(), refs[25]["c2r"][i])
    assert h(dc.to(torch.complex128)) is None                 # as Delay: a dtype it does not take
