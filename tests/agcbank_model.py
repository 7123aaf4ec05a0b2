"""The AGCBank's definition (include/ldsp.h) in numpy, shared by tests/test_agcbank_host.py
and tests/test_gpu_agcbank.py: the dB -> unit conversion, the quantised block peaks in
float64, the integer tracker as the serial recurrence and as the closed form, and the
output from a given gain_q in float64 or float32."""
import numpy as np

Q = 1 << 24
FLOOR = -64 * Q
CEIL = 64 * Q
DB_PER_OCTAVE = 20 * np.log10(2.0)


def units(db):
    """llrint(v 2^24 / (20 log10 2)) in double (rint: ties to even, as llrint in the default mode)."""
    return int(np.rint(np.float64(db) * np.float64(Q) / DB_PER_OCTAVE))


def block_peaks(x, B):
    """a_b per row and block, float64 [C, nb], over the whole blocks of x [C, n]."""
    x = np.asarray(x)
    C, n = x.shape
    nb = n // B
    xb = x[:, :nb * B].reshape(C, nb, B)
    if np.iscomplexobj(xb):
        m = xb.real.astype(np.float64) ** 2 + xb.imag.astype(np.float64) ** 2
        m = np.where(np.isfinite(m), m, 0.0)
        return np.sqrt(m.max(axis=2))
    a = np.abs(xb.astype(np.float32))
    a = np.where(np.isfinite(a), a, np.float32(0))
    return a.max(axis=2).astype(np.float64)


def quantise(a):
    """peak_q = clamp(ceil(log2(a) Q), FLOOR, CEIL), FLOOR for a = 0; int64."""
    a = np.asarray(a, np.float64)
    with np.errstate(divide="ignore"):
        t = np.ceil(np.log2(a) * np.float64(Q))
    t = np.where(a > 0, np.clip(t, FLOOR, CEIL), FLOOR)
    return t.astype(np.int64)


def window_max(pq, H, tail=None):
    """w_b = max(peak_q[b - H .. b]); tail: the H peaks before the first, oldest first (FLOOR if None)."""
    pq = np.atleast_2d(np.asarray(pq, np.int64))
    C, n = pq.shape
    front = np.full((C, H), FLOOR, np.int64) if tail is None else np.atleast_2d(np.asarray(tail, np.int64))
    ext = np.concatenate([front, pq], axis=1)
    if n == 0:
        return ext[:, :0]
    return np.lib.stride_tricks.sliding_window_view(ext, H + 1, axis=1).max(axis=2)


def track_serial(pq, H, d, level=None, tail=None):
    """L_b = max(w_b, L_{b-1} - d, FLOOR), block after block; int64 [C, n].  Python integers
    would do no better: every intermediate fits int64."""
    pq = np.atleast_2d(np.asarray(pq, np.int64))
    w = window_max(pq, H, tail)
    C, n = pq.shape
    L = np.empty((C, n), np.int64)
    cur = np.full(C, FLOOR, np.int64) if level is None else np.asarray(level, np.int64).reshape(C).copy()
    for b in range(n):
        cur = np.maximum(np.maximum(w[:, b], cur - d), FLOOR)
        L[:, b] = cur
    return L


def track_closed(pq, H, d):
    """L_b = max(FLOOR, max_{j <= b} (peak_q[j] - d max(0, b - j - H))) from a fresh stream; O(n^2)."""
    pq = np.atleast_2d(np.asarray(pq, np.int64))
    C, n = pq.shape
    b = np.arange(n)[:, None]
    j = np.arange(n)[None, :]
    pen = np.maximum(0, b - j - H).astype(np.int64) * np.int64(d)
    cand = np.where(j <= b, pq[:, None, :] - pen[None], FLOOR)
    return np.maximum(cand.max(axis=2), FLOOR)


def gain_q(L, T, Gmax):
    """min(T - L, Gmax); T a scalar or one per row."""
    T = np.asarray(T, np.int64).reshape(-1, 1)
    return np.minimum(T - np.asarray(L, np.int64), Gmax)


def gains(gq):
    """g = (float) exp2(gain_q / Q)."""
    return np.exp2(np.asarray(gq, np.float64) / np.float64(Q)).astype(np.float32)


def apply(x, gq, B, dtype=np.float64):
    """The emitted blocks of a fresh stream x [C, n] under gain_q [C, nb]: y [C, (nb - 1) B], with
    gamma = h_{b-1} + (h_b - h_{b-1}) (i + 1) / B evaluated left to right in `dtype`."""
    x = np.asarray(x)
    C = x.shape[0]
    g = gains(gq)
    nb = g.shape[1]
    ne = max(nb - 1, 0)
    if ne == 0:
        return x[:, :0].copy()
    h = np.minimum(g[:, :-1], g[:, 1:]).astype(dtype)                   # h_0 .. h_{nb-2}
    hm = np.concatenate([g[:, :1].astype(dtype), h[:, :-1]], axis=1)     # h_{-1} .. h_{nb-3}
    i1 = (np.arange(B) + 1).astype(dtype)
    gam = hm[:, :, None] + (h - hm)[:, :, None] * i1[None, None, :] / dtype(B)
    xb = x[:, :ne * B].reshape(C, ne, B)
    if np.iscomplexobj(xb):
        ct = np.complex128 if dtype == np.float64 else np.complex64
        y = (xb.real.astype(dtype) * gam + 1j * (xb.imag.astype(dtype) * gam)).astype(ct)
    else:
        y = xb.astype(dtype) * gam
    return y.reshape(C, ne * B)


def counts(T, B):
    """Blocks tracked and emitted after T samples."""
    return T // B, max(0, T // B - 1)
