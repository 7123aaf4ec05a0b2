"""The ToneBank's definition (include/ldsp.h) restated in numpy, shared by
tests/test_tonebank_host.py and tests/test_gpu_tonebank.py: the tables in double, the
float64 evaluation of the powers from float32 tables, the decision as an exact function of
float32 powers, and the hold window with its carried counter."""
import numpy as np

SAT = 65                      # the counter's ceiling: one more than the largest hold


def window(B, name):
    i = np.arange(B, dtype=np.float64)
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * i / B) if name == "hann" else np.ones(B)


def tables64(tones, B, name):
    """(Tc, Ts) as float64 [F][B] before the one rounding, and sum w."""
    w = window(B, name)
    sumw = 0.0
    for v in w:               # the order of the host's loop
        sumw += v
    s = np.sqrt(2.0) / sumw
    i = np.arange(B, dtype=np.float64)
    ph = 2.0 * np.pi * np.asarray(tones, np.float64)[:, None] * i[None, :]
    return s * w * np.cos(ph), -s * w * np.sin(ph), sumw


def power64(tables, x):
    """float64 powers [C][N][F] of the whole blocks of x ([C][K], any float) from the object's
    float32 tables ([2][F][B])."""
    t = np.asarray(tables, np.float64)
    F, B = t.shape[1], t.shape[2]
    C, K = x.shape
    N = K // B
    blocks = np.asarray(x[:, :N * B], np.float64).reshape(C * N, B)
    with np.errstate(invalid="ignore", over="ignore"):
        re = blocks @ t[0].T
        im = blocks @ t[1].T
        return (re * re + im * im).reshape(C, N, F)


def detect(power, floor, dominance):
    """(kstar, hit) from powers [..., F]: float32 powers give the kernel's rule bit for bit."""
    p = np.asarray(power)
    F = p.shape[-1]
    kstar = np.zeros(p.shape[:-1], np.int64)
    best = p[..., 0].copy()
    for k in range(1, F):     # the lowest index of the largest: replace on > only
        up = p[..., k] > best
        kstar = np.where(up, k, kstar)
        best = np.where(up, p[..., k], best)
    p64 = p.astype(np.float64)
    others = np.zeros(p.shape[:-1], np.float64)
    for k in range(F):        # in index order; the best one adds +0
        others = others + np.where(kstar == k, 0.0, p64[..., k])
    with np.errstate(invalid="ignore", over="ignore"):
        fin = np.isfinite(p).all(axis=-1)
        above = best > (np.float32(floor) if p.dtype == np.float32 else floor)
        dom = best.astype(np.float64) * float(F - 1) > float(dominance) * others
    return kstar, fin & above & dom


def decide(power, floor, dominance, want, hold, since):
    """tone int8 [C][N], open uint8 [C][N] and the next counter from powers [C][N][F], the
    wanted tone per row and the counter per row before the call."""
    kstar, hit = detect(power, floor, dominance)
    C, N = hit.shape
    want = np.broadcast_to(np.asarray(want, np.int64), (C,))
    since = np.asarray(since, np.int64)
    acc = hit & ((want[:, None] < 0) | (want[:, None] == kstar))
    idx = np.where(acc, np.arange(N)[None, :], -(1 << 40))
    last = np.maximum.accumulate(np.concatenate([(-1 - since)[:, None], idx], axis=1), axis=1)[:, 1:]
    opn = (np.arange(N)[None, :] - last) <= hold
    nxt = np.minimum(N - 1 - last[:, -1], SAT) if N else since
    tone = np.where(hit, kstar, -1).astype(np.int8)
    return tone, opn.astype(np.uint8), nxt.astype(np.int64), acc


def gate(x, opn, B):
    """the gated rows: closed blocks +0, open ones the input's bits."""
    C, N = opn.shape
    y = np.array(x[:, :N * B], np.float32).reshape(C, N, B)
    y[opn == 0] = 0.0
    return y.reshape(C, N * B)
