"""Int16 IQ ingest for the wideband objects: Channelizer.from_bytes,
Downconverter.from_bytes, Spectrogram.from_bytes and Spectrogram.write_bytes
(C ABI ldsp_chan_execute_iq16, ldsp_ddc_execute_iq16, ldsp_spgram_execute_iq16)
convert the SDR wire format -- interleaved int16 (I, Q) pairs -- in the
kernel's own loads.

The contract is obj.from_bytes(b) == obj(bytes_to_iq(b)), bit for bit, and the
same object state afterwards.  Every check below is therefore bit equality
against a twin object fed bytes_to_iq(raw): no tolerance is involved, the
two-call path is unchanged code that the objects' own tests hold to the float64
definitions.  The shapes are the smallest that reach every load path of each
kernel: a tile that begins in the history, inner tiles, a one-frame tile and a
ragged tail (F is the object's `tile`), in a first call and in one that
continues from the history the first one left.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CHAN = [(4, 4, 2), (16, 6, 8), (64, 6, 64), (256, 6, 128)]            # (M, m, D)
DDC = [(1, 2, 6), (3, 5, 6), (16, 64, 6), (2, 256, 8)]                # (C, D, m)
SPGRAM = [(256, 256, 128, 1), (1024, 300, 7, 3), (4096, 4096, 1024, 2)]   # (N, W, d, A)


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    assert liquiddsp.device_count() > 0
    return liquiddsp


def raw_iq(rng, n):
    """n random (I, Q) pairs over the full int16 range, the extremes of the wire format first."""
    r = rng.integers(-32768, 32768, size=2 * n, dtype=np.int64).astype(np.int16)
    head = [32767, -32768, 0, -1, 1, -32767]
    r[:min(len(head), r.size)] = head[:r.size]
    return r


def host(y):
    return y.cpu().numpy() if hasattr(y, "is_cuda") else np.asarray(y)


def same_bits(a, b):
    a, b = host(a), host(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    w = {np.dtype(np.complex64): np.uint64, np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}[a.dtype]
    return np.array_equal(np.ascontiguousarray(a).view(w), np.ascontiguousarray(b).view(w))


def freqs(C):
    return [((7 * c + 3) % 19 - 9) / 20.0 for c in range(C)]          # distinct, both signs, in (-0.5, 0.5)


def chan(ld, M, m, D):
    return ld.Channelizer(M, D, m=m)


def ddc(ld, C, D, m):
    return ld.Downconverter(freqs(C), D, m=m)


def spgram(ld, N, W, d, A):
    return ld.Spectrogram(N, window="hann", window_len=W, delay=d, average=A)


def feed(kind, raw, dev):
    """raw (int16 numpy, whole pairs) as one of from_bytes' input kinds."""
    if dev:
        import torch
        return torch.from_numpy(raw).cuda()
    return raw.tobytes() if kind % 2 else raw


def two_call(ld, obj, raw, dev, method="__call__"):
    import torch
    b = torch.from_numpy(raw).cuda() if dev else raw.tobytes()
    return getattr(obj, method)(ld.bytes_to_iq(b))


# ------------------------------------------------------------------ every load path, per object
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("M,m,D", CHAN)
def test_channelizer_from_bytes(ld, rng, M, m, D, dev):
    a, b = chan(ld, M, m, D), chan(ld, M, m, D)
    n = D * (2 * a.tile + 1) + 3
    for call in range(2):
        raw = raw_iq(rng, n)
        ya, yb = a.from_bytes(feed(call, raw, dev)), two_call(ld, b, raw, dev)
        assert hasattr(ya, "is_cuda") == dev and ya.shape[0] == M and ya.shape[1] >= 2 * a.tile + 1
        assert same_bits(ya, yb), call
        assert a.skip == b.skip


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("C,D,m", DDC)
def test_downconverter_from_bytes(ld, rng, C, D, m, dev):
    a, b = ddc(ld, C, D, m), ddc(ld, C, D, m)
    n = D * (2 * a.tile + 1) + 3
    for call in range(2):
        raw = raw_iq(rng, n)
        ya, yb = a.from_bytes(feed(call, raw, dev)), two_call(ld, b, raw, dev)
        assert hasattr(ya, "is_cuda") == dev and ya.shape[0] == C
        assert same_bits(ya, yb), call
        assert a.skip == b.skip


@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("N,W,d,A", SPGRAM)
def test_spectrogram_from_bytes_and_write_bytes(ld, rng, N, W, d, A, dev):
    """Rows from from_bytes; the return value and the float64 psd from write_bytes.  Each call
    takes 2 tile + 3 transforms (three workgroups), the second continues the first one's
    history and unfinished row."""
    a, b = spgram(ld, N, W, d, A), spgram(ld, N, W, d, A)
    wa, wb = spgram(ld, N, W, d, A), spgram(ld, N, W, d, A)
    n = d * (2 * a.tile + 3) + W + 5
    for call in range(2):
        raw = raw_iq(rng, n)
        ya, yb = a.from_bytes(feed(call, raw, dev)), two_call(ld, b, raw, dev)
        assert hasattr(ya, "is_cuda") == dev and ya.shape[1] == N and ya.shape[0] >= (2 * a.tile) // A
        assert same_bits(ya, yb), call
        assert same_bits(a.psd, b.psd)
        ta, tb = wa.write_bytes(feed(call, raw, dev)), two_call(ld, wb, raw, dev, "write")
        assert ta == tb and ta >= 2 * a.tile + 3
        assert (wa.num_samples, wa.num_transforms) == (wb.num_samples, wb.num_transforms)
        assert same_bits(wa.psd, wb.psd) and same_bits(wa.psd, a.psd)


# ------------------------------------------------------------------ one stream, both kinds of call
def stream_cuts(D, F, H):
    """Call lengths with 0, 1, D - 1, D + 1, F D - 1, F D, F D + 1 and H - 1 among them (H the
    history length), ordered so that short calls follow long ones and the other way round."""
    return [F * D + 1, 0, 1, D - 1, H - 1, F * D, 0, D + 1, F * D - 1, 3 * F * D + D + 2, 1, H + 3]


def run_stream(ld, rng, a, b, cuts, dev, first, state):
    """a alternates from_bytes and the complex64 call from cut to cut (first: the kind of its
    first call, so that every length is taken by both kinds), b takes complex64 throughout."""
    for i, n in enumerate(cuts):
        raw = raw_iq(rng, n)
        if (i + first) % 2 == 0:
            ya = a.from_bytes(feed(i // 2, raw, dev))
        else:
            ya = two_call(ld, a, raw, dev)
        yb = two_call(ld, b, raw, dev)
        assert same_bits(ya, yb), (i, n)
        assert state(a) == state(b), (i, n)
    a.reset()
    b.reset()
    raw = raw_iq(rng, cuts[0])
    assert same_bits(a.from_bytes(feed(0, raw, dev)), two_call(ld, b, raw, dev))
    assert state(a) == state(b)


@pytest.mark.parametrize("first", [0, 1], ids=["int16-first", "complex64-first"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_channelizer_stream_mixes_int16_and_complex64(ld, rng, dev, first):
    M, m, D = CHAN[1]
    a, b = chan(ld, M, m, D), chan(ld, M, m, D)
    run_stream(ld, rng, a, b, stream_cuts(D, a.tile, len(a.taps) + (-len(a.taps)) % M - 1), dev, first,
               lambda o: o.skip)


@pytest.mark.parametrize("first", [0, 1], ids=["int16-first", "complex64-first"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_downconverter_stream_mixes_int16_and_complex64(ld, rng, dev, first):
    C, D, m = DDC[1]
    a, b = ddc(ld, C, D, m), ddc(ld, C, D, m)
    run_stream(ld, rng, a, b, stream_cuts(D, a.tile, len(a.taps) - 1), dev, first, lambda o: o.skip)


@pytest.mark.parametrize("first", [0, 1], ids=["int16-first", "complex64-first"])
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_spectrogram_stream_mixes_int16_and_complex64(ld, rng, dev, first):
    N, W, d, A = SPGRAM[1]
    a, b = spgram(ld, N, W, d, A), spgram(ld, N, W, d, A)
    run_stream(ld, rng, a, b, stream_cuts(d, a.tile, W - 1), dev, first,
               lambda o: (o.num_samples, o.num_transforms, o.psd.tobytes()))


# ------------------------------------------------------------------ alignment and input kinds
def test_channelizer_input_kinds_and_alignment(ld, rng):
    """The kernel may assume 4-byte alignment of x and no more: device int16 views that start
    0 .. 3 pairs into a buffer (every residue of a 16-byte line), a uint8 view at an odd byte
    offset (from_bytes clones it), host bytes with 1 .. 3 trailing bytes (dropped, as
    bytes_to_iq drops them) and an int16 numpy array."""
    import torch
    M, m, D = CHAN[1]
    n = D * (2 * chan(ld, M, m, D).tile + 1) + 3
    raw = raw_iq(rng, n)
    ref = host(two_call(ld, chan(ld, M, m, D), raw, False))

    buf = torch.zeros(2 * (n + 4), dtype=torch.int16, device="cuda")
    for off in range(4):
        buf.zero_()
        view = buf[2 * off:2 * (off + n)]
        view.copy_(torch.from_numpy(raw))
        assert view.data_ptr() % 16 == (buf.data_ptr() + 4 * off) % 16
        y = chan(ld, M, m, D).from_bytes(view)
        assert y.is_cuda and same_bits(y, ref), off

    b8 = torch.zeros(4 * n + 8, dtype=torch.uint8, device="cuda")
    odd = b8[1:1 + 4 * n]
    odd.copy_(torch.from_numpy(raw.view(np.uint8)))
    assert odd.data_ptr() % 4 != 0
    assert same_bits(chan(ld, M, m, D).from_bytes(odd), ref)

    for extra in (b"\x01", b"\x01\x02", b"\x01\x02\x03"):
        y = chan(ld, M, m, D).from_bytes(raw.tobytes() + extra)
        assert isinstance(y, np.ndarray) and same_bits(y, ref), len(extra)
        t = torch.frombuffer(bytearray(raw.tobytes() + extra), dtype=torch.uint8).cuda()
        assert same_bits(chan(ld, M, m, D).from_bytes(t), ref), len(extra)
    assert same_bits(chan(ld, M, m, D).from_bytes(raw), ref)
    assert same_bits(chan(ld, M, m, D).from_bytes(raw.view(np.uint8)), ref)
    assert same_bits(chan(ld, M, m, D).from_bytes(bytearray(raw.tobytes())), ref)


# ------------------------------------------------------------------ retune
@pytest.mark.parametrize("dev", [False, True], ids=["host", "device"])
def test_downconverter_retune_between_from_bytes_calls(ld, rng, dev):
    """The history holds converted samples, so dc.freqs = ... between two int16 calls gives what
    it gives between two complex64 calls (the tuner count changes too)."""
    C, D, m = DDC[2]
    a, b = ddc(ld, C, D, m), ddc(ld, C, D, m)
    n = D * a.tile + D // 2 + 1
    raw0, raw1 = raw_iq(rng, n), raw_iq(rng, n)
    assert same_bits(a.from_bytes(feed(0, raw0, dev)), two_call(ld, b, raw0, dev))
    new = [0.05, -0.3, 0.45]
    a.freqs = new
    b.freqs = new
    ya, yb = a.from_bytes(feed(1, raw1, dev)), two_call(ld, b, raw1, dev)
    assert ya.shape[0] == 3 and same_bits(ya, yb)
    assert a.skip == b.skip and np.array_equal(a.words, b.words)
