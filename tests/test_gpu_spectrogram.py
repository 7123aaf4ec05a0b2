"""Spectrogram on the GPU: the streaming Welch periodogram (k_spgram.hip)
against its definition, evaluated here in float64 with the object's own window,

    X_s[k] = sum_{i<W} w[i] x[(s + 1) d - W + i] exp(-2 pi i k i / N)
    P_s[k] = |X_s[k]|^2,   row r = mean of P_s over s = rA .. rA + A - 1,
    psd    = mean of P_s over every transform since reset() / clear()

with zeros before the stream's first sample.  Sizes come from the kernel's tile
(F transforms per workgroup): one call of d (2 F A + A + 1) + 3 samples is two
full tiles of rows, a short one and a ragged tail with a pending partial row.
Averages of 16 or more transforms that are multiples of 8 take the blocked
path (block sums of 8, then k_spgram_rows) and are among every group's shapes.
The gate of 1e-6 of a row's largest bin is the project's gate for FIR-class
kernels; a plain float32 numpy FFT of the same windowed segments
stays at or below 1.8e-7 on these inputs.  Streams cut into calls must give the
single call's rows bit for bit."""
import ctypes as C
import functools
import os

import numpy as np
import pytest

from conftest import cgauss

pytestmark = pytest.mark.gpu

GATE = 1e-6
HERE = os.path.dirname(os.path.abspath(__file__))
LIBPATH = os.path.join(os.path.dirname(HERE), "python-liquiddsp_amd", "libldsp.so")
MEM_HOST, MEM_DEVICE = 0, 1

# (N, W, d, A, window): every instantiation; zero padding with a hop dividing
# nothing; no overlap; a window shorter than the hop's multiple; one
# blackmanharris and one user window ("user": seeded, not normalised)
SHAPES = [(256, 256, 128, 1, "hann"), (512, 512, 256, 2, "hann"), (1024, 1024, 256, 1, "hann"),
          (1024, 300, 7, 3, "hann"), (2048, 2048, 2048, 1, "hann"), (4096, 4096, 1024, 2, "hann"),
          (4096, 1000, 1000, 1, "hann"), (512, 400, 100, 2, "blackmanharris"), (2048, 1500, 700, 3, "user")]
# averages of 16 or more that are multiples of 8 are summed in blocks of 8 transforms (k_spgram_rows)
SHAPES += [(256, 256, 32, 16, "hann"), (4096, 4096, 1024, 16, "hann")]
STREAM_SHAPES = [(256, 256, 128, 1, "hann"), (1024, 300, 7, 3, "hann"), (4096, 4096, 1024, 2, "hann"),
                 (1024, 1024, 64, 24, "hamming")]


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def bits64(a):
    return np.ascontiguousarray(a).view(np.uint64)


def make(ld, N, W, d, A, window):
    if window == "user":
        w = (np.random.default_rng(77 + W).standard_normal(W) / np.sqrt(W)).astype(np.float32)
        return ld.Spectrogram(N, window=w, window_len=W, delay=d, average=A)
    return ld.Spectrogram(N, window=window, window_len=W, delay=d, average=A)


def signal(seed, n, N):
    """cgauss noise at 1e-2 plus two unit-scale tones off bin centres."""
    t = np.arange(n, dtype=np.float64)
    f1, f2 = (0.1 * N + 0.37) / N, -(0.3 * N + 0.21) / N
    x = np.exp(2j * np.pi * f1 * t) + 0.8 * np.exp(2j * np.pi * (f2 * t + 0.1))
    return (x + cgauss(np.random.default_rng(seed), n, 1e-2)).astype(np.complex64)


def definition(x, w, N, d, s0, s1):
    """P_s for s0 <= s < s1 in float64: [s1 - s0, N]."""
    w = np.asarray(w).astype(np.float64)
    W = w.size
    xp = np.concatenate([np.zeros(W - 1, np.complex128), np.asarray(x).astype(np.complex128)])   # xp[t + W - 1] = x[t]
    first = (np.arange(s0, s1) + 1) * d - 1                       # xp index of the window's first sample
    assert s1 == s0 or first[-1] + W <= xp.size
    seg = xp[first[:, None] + np.arange(W)[None, :]] * w[None, :]
    X = np.fft.fft(seg, n=N, axis=1)
    return X.real ** 2 + X.imag ** 2


def rows_of(P, A):
    K = P.shape[0] // A
    return P[:K * A].reshape(K, A, -1).mean(axis=1)


def row_err(y, ref):
    return np.max(np.abs(y.astype(np.float64) - ref), axis=1) / np.max(ref, axis=1)


def base_len(F, d, A):
    return d * (2 * F * A + A + 1) + 3


@functools.lru_cache(maxsize=None)
def case(N, W, d, A, window, n=None):
    """Input, the object's window and the float64 transforms of one stream (shared, never modified)."""
    import liquiddsp
    s = make(liquiddsp, N, W, d, A, window)
    n = base_len(s.tile, d, A) if n is None else n
    x = signal(3000 + N + W + d + A, n, N)
    P = definition(x, s.window, N, d, 0, n // d)
    for a in (x, P):
        a.setflags(write=False)
    return x, P


# ---------------------------------------------------------------- 1. parity with the definition
@pytest.mark.parametrize("N,W,d,A,window", SHAPES)
def test_parity_with_definition(ld, N, W, d, A, window):
    x, P = case(N, W, d, A, window)
    s = make(ld, N, W, d, A, window)
    F = s.tile
    y = s(x)
    S = x.size // d
    assert S == 2 * F * A + A + 1 and S % A == 1 % A
    assert y.dtype == np.float32 and y.shape == (S // A, N)
    assert (s.num_samples, s.num_transforms) == (x.size, S)
    err = row_err(y, rows_of(P, A))
    print(f"N={N} W={W} d={d} A={A} {window}: worst row {err.max():.3g}")
    assert err.max() <= GATE, (int(np.argmax(err)), float(err.max()))


@pytest.mark.parametrize("N,W,d,A", [(256, 256, 128, 1), (1024, 300, 7, 3), (4096, 4096, 1024, 2)])
def test_first_rows_see_zeros_before_the_stream(ld, N, W, d, A):
    """The rows whose windows reach before t = 0: the definition with zeros there."""
    x, P = case(N, W, d, A, "hann")
    s = make(ld, N, W, d, A, "hann")
    early = -(-(-(-W // d)) // A)                      # rows holding a transform with (s + 1) d < W
    n = early * A * d
    assert n <= x.size
    y = s(x[:n])
    assert y.shape == (early, N)
    err = row_err(y, rows_of(P[:early * A], A))
    print(f"N={N} W={W} d={d} A={A}: first {early} rows, worst {err.max():.3g}")
    assert err.max() <= GATE
    # the very first transform of a one-sample hop sees one sample: |w[W - 1] x[0]|^2 in every bin
    s1 = ld.Spectrogram(N, window="hamming", window_len=W, delay=1)
    y1 = s1(x[:1])
    ref = np.full(N, abs(np.float64(s1.window[-1]) * np.complex128(x[0])) ** 2)
    assert y1.shape == (1, N) and np.max(np.abs(y1[0] - ref)) <= GATE * ref[0]


# ---------------------------------------------------------------- 2. streaming invariance, bitwise
def cuts_for(F, W, d, A, seed, base):
    rng = np.random.default_rng(seed)
    forced = [0, 1, d - 1, d + 1, A * d - 1, A * d + 1, F * d, F * d + 1, W - 2]
    cuts = []
    for f in forced:
        cuts += [f, int(rng.integers(0, 3 * d * A + 1))]
    rest = base - sum(cuts)
    if rest > 0:
        cuts.append(rest)
    return cuts


@pytest.mark.parametrize("N,W,d,A,window", STREAM_SHAPES)
def test_streaming_is_bitwise_invariant(ld, N, W, d, A, window):
    F = make(ld, N, W, d, A, window).tile
    cuts = cuts_for(F, W, d, A, 4000 + N, base_len(F, d, A))
    n = sum(cuts)
    x, P = case(N, W, d, A, window, n)
    whole = make(ld, N, W, d, A, window)
    ref = whole(x)
    assert ref.shape == (n // d // A, N)
    assert row_err(ref, rows_of(P, A)).max() <= GATE
    s = make(ld, N, W, d, A, window)
    got, T = [], 0
    for c in cuts:
        want = ((T + c) // d - T // d, (T + c) // d // A - T // d // A)
        assert s.num_outputs(c) == want
        y = s(x[T:T + c])
        assert y.shape == (want[1], N)
        got.append(y)
        T += c
        assert (s.num_samples, s.num_transforms) == (T, T // d)
    got = np.concatenate(got)
    assert got.shape == ref.shape and (bits(got) == bits(ref)).all()
    # the accumulator of a differently cut stream: the same mean within the gate, bits not required
    mean = P.mean(axis=0)
    for obj in (whole, s):
        assert obj.num_transforms == P.shape[0]
        assert np.max(np.abs(obj.psd - mean)) / mean.max() <= GATE


def test_long_blocked_call_is_taken_in_pieces(ld):
    """A blocked average passes its block sums through memory, at most 16384 - 1
    blocks of 8 transforms per launch pair: one call longer than that gives the
    bits of the same stream in short calls, and the rows around the seam match
    the definition."""
    N, W, d, A = 256, 256, 1, 16
    seam = d * 8 * (16384 - 1)                        # samples of the first piece
    n = seam + 9000
    x = signal(4500, n, N)
    whole = make(ld, N, W, d, A, "hann")
    ref = whole(x)
    assert ref.shape == (n // A, N) and (whole.num_samples, whole.num_transforms) == (n, n)
    s = make(ld, N, W, d, A, "hann")
    got = np.concatenate([s(x[o:o + 30011]) for o in range(0, n, 30011)])
    assert (bits(got) == bits(ref)).all()
    r0 = seam // A - 2
    P = definition(x[:(r0 + 4) * A], s.window, N, d, r0 * A, (r0 + 4) * A)
    err = row_err(ref[r0:r0 + 4], rows_of(P, A))
    print(f"rows {r0}..{r0 + 3} around the seam: worst {err.max():.3g}")
    assert err.max() <= GATE


# ---------------------------------------------------------------- 3. accumulator
@pytest.mark.parametrize("N,W,d,A,window", STREAM_SHAPES + [(2048, 1500, 700, 3, "user")])
def test_accumulator(ld, N, W, d, A, window):
    x, P = case(N, W, d, A, window)
    mean = P.mean(axis=0)
    a = make(ld, N, W, d, A, window)
    a(x)
    assert a.num_transforms == P.shape[0]
    psd = a.psd
    assert psd.dtype == np.float64 and psd.shape == (N,)
    err = np.max(np.abs(psd - mean)) / mean.max()
    print(f"N={N} W={W} d={d} A={A} {window}: psd {err:.3g}")
    assert err <= GATE
    # the same calls through write(), and a twin fed the same sequence: the same bits
    h = x.size // 3 + 1
    seq = [x[:h], x[h:h + 5], x[h + 5:]]
    b, c, e = (make(ld, N, W, d, A, window) for _ in range(3))
    T = 0
    for part in seq:
        nt = (T + part.size) // d - T // d
        b(part)
        e(part)
        assert c.write(part) == nt
        T += part.size
    assert b.num_transforms == c.num_transforms == e.num_transforms == P.shape[0]
    assert (bits64(b.psd) == bits64(c.psd)).all()
    assert (bits64(b.psd) == bits64(e.psd)).all()
    assert np.max(np.abs(b.psd - mean)) / mean.max() <= GATE


# ---------------------------------------------------------------- 4. clear() and reset()
@pytest.mark.parametrize("N,W,d,A,window", [(1024, 300, 7, 3, "hann"), (4096, 4096, 1024, 2, "hann"),
                                            (1024, 1024, 64, 24, "hamming")])
def test_clear_keeps_the_stream(ld, N, W, d, A, window):
    x, P = case(N, W, d, A, window)
    ref = make(ld, N, W, d, A, window)(x)
    s = make(ld, N, W, d, A, window)
    n1 = d * (A + 1) + 2                              # one row and a partial one behind, T unaligned
    y1 = s(x[:n1])
    s.clear()
    assert (s.num_samples, s.num_transforms) == (n1, 0) and not s.psd.any()
    assert s.num_outputs(x.size - n1) == (x.size // d - n1 // d, x.size // d // A - n1 // d // A)
    y2 = s(x[n1:])
    got = np.concatenate([y1, y2])
    assert got.shape == ref.shape and (bits(got) == bits(ref)).all()
    S1 = n1 // d
    assert s.num_transforms == P.shape[0] - S1
    mean = P[S1:].mean(axis=0)
    assert np.max(np.abs(s.psd - mean)) / mean.max() <= GATE


@pytest.mark.parametrize("N,W,d,A,window", [(1024, 300, 7, 3, "hann"), (4096, 4096, 1024, 2, "hann"),
                                            (1024, 1024, 64, 24, "hamming")])
def test_reset_restarts(ld, N, W, d, A, window):
    x, _ = case(N, W, d, A, window)
    s = make(ld, N, W, d, A, window)
    first = s(x)
    psd = s.psd
    assert (x.size // d) % A != 0 and x.size % d != 0    # a partial row and an unaligned T are left behind
    s(x[:d * (A // 2 + 1) + 1])
    s.reset()
    assert (s.num_samples, s.num_transforms) == (0, 0) and not s.psd.any()
    again = s(x)
    assert (bits(again) == bits(first)).all() and (bits64(s.psd) == bits64(psd)).all()


# ---------------------------------------------------------------- 5. memory kinds and layouts
def test_host_device_strided_complex128_agree(ld):
    import torch
    N, W, d, A = 1024, 300, 7, 3
    x, _ = case(N, W, d, A, "hann")
    ref = make(ld, N, W, d, A, "hann")(x)
    dev = make(ld, N, W, d, A, "hann")(torch.from_numpy(np.array(x)).to("cuda:0"))
    assert dev.is_cuda and dev.dtype == torch.float32 and tuple(dev.shape) == ref.shape
    assert (bits(dev.cpu().numpy()) == bits(ref)).all()
    wide = np.zeros((x.size, 2), np.complex64)
    wide[:, 0] = x
    assert (bits(make(ld, N, W, d, A, "hann")(wide[:, 0])) == bits(ref)).all()
    wide_d = torch.from_numpy(wide).to("cuda:0")
    assert (bits(make(ld, N, W, d, A, "hann")(wide_d[:, 0]).cpu().numpy()) == bits(ref)).all()
    assert (bits(make(ld, N, W, d, A, "hann")(x.astype(np.complex128))) == bits(ref)).all()
    s = make(ld, N, W, d, A, "hann")
    assert s.write(torch.from_numpy(np.array(x)).to("cuda:0")) == x.size // d
    twin = make(ld, N, W, d, A, "hann")
    twin.write(x)
    assert (bits64(s.psd) == bits64(twin.psd)).all()


def test_c_abi_row_stride(ld):
    """ld > nfft in host and in device memory: the floats between rows stay untouched."""
    import torch
    N, W, d, A = 256, 256, 128, 1
    x, _ = case(N, W, d, A, "hann")
    ref = make(ld, N, W, d, A, "hann")(x)
    K, ldy = ref.shape[0], N + 5
    L = C.CDLL(LIBPATH)
    vp, u, sz = C.c_void_p, C.c_uint, C.c_size_t
    L.ldsp_spgram_create.argtypes = [u, C.c_int, u, u, u, C.POINTER(vp)]
    L.ldsp_spgram_destroy.argtypes = [vp]
    L.ldsp_spgram_execute.argtypes = [vp, vp, sz, vp, sz, C.POINTER(sz), C.c_int, vp]
    L.ldsp_spgram_get_psd.argtypes = [vp, vp, C.POINTER(C.c_uint64)]
    # host memory
    q = vp()
    assert L.ldsp_spgram_create(N, 1, W, d, A, C.byref(q)) == 0
    y = np.full((K, ldy), -7.0, np.float32)
    nr = sz()
    xs = np.array(x)
    assert L.ldsp_spgram_execute(q, xs.ctypes.data, xs.size, y.ctypes.data, ldy, C.byref(nr), MEM_HOST, None) == 0
    assert nr.value == K and (bits(y[:, :N]) == bits(ref)).all() and (y[:, N:] == -7.0).all()
    # accumulate only: y = NULL, ld ignored, the count still set
    nr = sz(99)
    assert L.ldsp_spgram_execute(q, xs.ctypes.data, d, None, 0, C.byref(nr), MEM_HOST, None) == 0 and nr.value == 1
    p = np.zeros(N)
    S = C.c_uint64()
    assert L.ldsp_spgram_get_psd(q, p.ctypes.data, C.byref(S)) == 0 and S.value == K + 1 and p.max() > 0
    assert L.ldsp_spgram_destroy(q) == 0
    # device memory on the current stream
    q = vp()
    assert L.ldsp_spgram_create(N, 1, W, d, A, C.byref(q)) == 0
    xd = torch.from_numpy(xs).to("cuda:0")
    yd = torch.full((K, ldy), -7.0, dtype=torch.float32, device="cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    nr = sz()
    assert L.ldsp_spgram_execute(q, xd.data_ptr(), xs.size, yd.data_ptr(), ldy, C.byref(nr), MEM_DEVICE, st) == 0
    torch.cuda.synchronize()
    yh = yd.cpu().numpy()
    assert nr.value == K and (bits(yh[:, :N]) == bits(ref)).all() and (yh[:, N:] == -7.0).all()
    assert L.ldsp_spgram_destroy(q) == 0


# ---------------------------------------------------------------- 6. with the Channelizer
@pytest.mark.parametrize("k", [3, 13])
def test_finds_the_channelizer_channel(ld, k):
    ch = ld.Channelizer(16)
    N, n = 1024, 8192
    t = np.arange(n, dtype=np.float64)
    x = (np.exp(2j * np.pi * ch.centers[k] * t) + cgauss(np.random.default_rng(6000 + k), n, 1e-3)).astype(np.complex64)
    s = ld.Spectrogram(N)
    assert s.write(x) == n // s.delay
    assert int(np.argmax(s.psd)) == k * N // 16
    assert s.freqs[k * N // 16] == ch.centers[k]
    y = ch(x)
    assert int(np.argmax(np.sum(np.abs(y.astype(np.complex128)) ** 2, axis=1))) == k
