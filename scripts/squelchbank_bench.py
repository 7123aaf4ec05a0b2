"""SquelchBank timing on the GPU, device tensors, two shapes of 64 Mi input samples
(16 rows of 4 Mi, 256 rows of 256 Ki) at block = 1024 and block = 64, the
configurations alternated in one process:
  m  sq.measure(x)                        k_sqbank_power, k_sqbank_fsm
  c  sq(x)                                the two and k_sqbank_gate
  p  the torch baseline of m's device work: p = (x.real**2 + x.imag**2)
     .view(C, nb, B).mean(2)
  g  the torch baseline of c's device work: p as above and
     x.view(C, nb, B) * open[:, :, None] with a mask already on the device
and, per shape and block, the baseline's state machine in numpy on the host
copy of p, timed once with the host clock and reported on its own line
(host_fsm_ms): p and g leave it out, so the baseline's call is p or g plus a
device-to-host copy, that loop and a host-to-device copy.  Then
  r  Channelizer(16, 8) -> FMBank(16, kf, 8) -> AudioBank(16, 0.192, deemphasis=250e3)
  s  the same with SquelchBank(16) after the Channelizer
on 64 Mi wideband samples, end to end.
Even rows are noise at 0 dB, odd rows noise at -40 dB, the threshold is -10 dB:
half of the blocks are open.  Before the timing the bank's status must equal
the numpy state machine over its own level, its level must agree with the
baseline's to 1e-5 of the row's maximum, and its gated rows must equal the
baseline's product.  Per configuration: SQBENCH_ROUNDS rounds (12), each of
enough calls to fill SQBENCH_WINDOW_MS between two device events on the
object's stream (per-call time of each round; their median and min-max), then
the per-kernel times of a separate pass under the library's profile hooks.
Floors over 8 TB/s: m reads 8 B per sample; c reads 8 B and writes 8 B per
sample and reads 8 B again per sample of an open block.  Fails without a GPU
and when a check fails; it sets no speed threshold.  Prints one JSON line (and
writes it to the file named by --out).  LDSP_PKG_DIR selects the package build."""
import json
import math
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("LDSP_PKG_DIR") or os.path.join(REPO, "python-liquiddsp_amd")
sys.path[:0] = [REPO, PKG]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import liquiddsp as L  # noqa: E402

HBM = 8.0e12                       # bytes / s
DB = -10.0
ALPHA, TIMEOUT = 0.25, 4
KF, RATE, SR = 0.25, 0.192, 250e3


def step(m, timer, hi, timeout):
    """agc_squelch_update_mode over rows: the next (mode, timer)."""
    mode = np.where(m == 1, np.where(hi, 2, 1), np.where(hi, 3, np.where(m >= 4, 5, 4)))
    timer = np.where(m == 4, timeout, np.where(m == 5, timer - 1, timer))
    mode = np.where((m == 5) & (timer == 0), 6, mode)
    return np.where(m == 6, 1, mode), timer


def host_fsm(p, alpha, thr, timeout):
    """The baseline's state machine: numpy over rows, a Python loop over blocks."""
    C, nb = p.shape
    s = np.zeros(C)
    mode = np.ones(C, np.int64)
    timer = np.zeros(C, np.int64)
    level = np.empty((C, nb), np.float32)
    st = np.empty((C, nb), np.uint8)
    for b in range(nb):
        s = s + alpha * (p[:, b] - s)
        level[:, b] = s
        mode, timer = step(mode, timer, level[:, b] > thr, timeout)
        st[:, b] = mode
    return level, st


def status_from(level, thr, timeout):
    """The state machine over the bank's own float32 level."""
    C, nb = level.shape
    mode = np.ones(C, np.int64)
    timer = np.zeros(C, np.int64)
    st = np.empty((C, nb), np.uint8)
    hi = level > thr
    for b in range(nb):
        mode, timer = step(mode, timer, hi[:, b], timeout)
        st[:, b] = mode
    return st


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("squelchbank_bench: needs a GPU")
    shapes = {"16": (16, int(os.environ.get("SQBENCH_N16", 4 << 20))),
              "256": (256, int(os.environ.get("SQBENCH_N256", 256 << 10)))}
    blocks = (1024, 64)
    wide_n = int(os.environ.get("SQBENCH_WIDE", 64 << 20))
    rounds = int(os.environ.get("SQBENCH_ROUNDS", 12))
    window = float(os.environ.get("SQBENCH_WINDOW_MS", 20.0))
    assert rounds >= 3
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    xs = {}
    for key, (C, n) in shapes.items():
        amp = torch.where(torch.arange(C, device="cuda") % 2 == 0, 1.0, 0.01)[:, None] / math.sqrt(2.0)
        xs[key] = torch.complex(torch.randn((C, n), generator=g, device="cuda") * amp,
                                torch.randn((C, n), generator=g, device="cuda") * amp)
    wide = torch.complex(torch.randn(wide_n, generator=g, device="cuda"), torch.randn(wide_n, generator=g, device="cuda"))
    thr = np.float32(10.0 ** (DB / 10))

    cfg, info, checks, host_ms = {}, {}, {}, {}
    for key, (C, n) in shapes.items():
        x = xs[key]
        for B in blocks:
            nb = n // B
            tag = f"{C}_b{B}"

            def base_p(x=x, C=C, nb=nb, B=B):
                return (x.real ** 2 + x.imag ** 2).view(C, nb, B).mean(2)

            # the checks, on fresh objects
            sq = L.SquelchBank(C, B, DB, ALPHA, TIMEOUT)
            y = sq(x)
            st, lv = sq.status.cpu().numpy(), sq.level.cpu().numpy()
            p = base_p().cpu().numpy().astype(np.float64)
            t0 = time.perf_counter()
            blv, bst = host_fsm(p, ALPHA, thr, TIMEOUT)
            host_ms[tag] = round((time.perf_counter() - t0) * 1e3, 2)
            opn = (st >= 2) & (st <= 5)
            mask = torch.from_numpy(opn).to("cuda")
            by = (x.view(C, nb, B) * mask[:, :, None]).view(C, nb * B)
            den = np.maximum(np.max(np.abs(blv), axis=1, keepdims=True), 1e-30)
            checks[tag] = {"status_is_a_function_of_level": bool((st == status_from(lv, thr, TIMEOUT)).all()),
                           "level_max_diff_over_row_max": float(np.max(np.abs(lv.astype(np.float64) - blv) / den)),
                           "gated_rows_equal_baseline": bool(torch.equal(y, by)),
                           "open_fraction": float(opn.mean())}
            del y, by
            bank_m, bank_c = L.SquelchBank(C, B, DB, ALPHA, TIMEOUT), L.SquelchBank(C, B, DB, ALPHA, TIMEOUT)
            info[f"m_measure_{tag}"] = info[f"c_call_{tag}"] = (C, n, B, float(opn.mean()), bank_m.tile)
            cfg[f"m_measure_{tag}"] = (lambda b=bank_m, x=x: b.measure(x))
            cfg[f"c_call_{tag}"] = (lambda b=bank_c, x=x: b(x))
            cfg[f"p_torch_power_{tag}"] = base_p
            cfg[f"g_torch_power_gate_{tag}"] = (lambda x=x, C=C, nb=nb, B=B, mask=mask, f=base_p:
                                               (f(), x.view(C, nb, B) * mask[:, :, None]))
    ch, fm, au = L.Channelizer(16, 8), L.FMBank(16, KF, 8), L.AudioBank(16, RATE, deemphasis=SR)
    ch2, sq2, fm2, au2 = L.Channelizer(16, 8), L.SquelchBank(16), L.FMBank(16, KF, 8), L.AudioBank(16, RATE, deemphasis=SR)
    cfg["r_channelizer_fmbank_audiobank_16"] = lambda: au(fm(ch(wide)))
    cfg["s_channelizer_squelchbank_fmbank_audiobank_16"] = lambda: au2(fm2(sq2(ch2(wide))))
    cfg = dict(sorted(cfg.items()))

    calls = {}
    for name, fn in cfg.items():   # warm-up (code objects, history buffers, torch's allocator), then the call count
        fn()
        fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(3):
            fn()
        e1.record()
        e1.synchronize()
        calls[name] = max(3, min(2000, math.ceil(window / (e0.elapsed_time(e1) / 3))))
    per_call = {k: [] for k in cfg}
    for _ in range(rounds):
        for name, fn in cfg.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls[name]):
                fn()
            e1.record()
            e1.synchronize()
            per_call[name].append(e0.elapsed_time(e1) / calls[name])
    kernels = {}
    for name, fn in cfg.items():
        L._profile_reset()
        L._profile_enable(True)
        for _ in range(4):
            fn()
        torch.cuda.synchronize()
        L._profile_enable(False)
        kernels[name] = {k: round(tot / 4, 4) for k, (c, tot) in L._profile_report().items()}
    sq2_open = float(((sq2.status >= 2) & (sq2.status <= 5)).float().mean())

    res = {"shapes": {k: {"C": v[0], "n_per_row": v[1]} for k, v in shapes.items()}, "blocks": list(blocks),
           "wideband_samples": wide_n, "threshold_dB": DB, "bandwidth": ALPHA, "timeout": TIMEOUT, "rounds": rounds,
           "window_ms": window, "calls_per_round": calls, "pkg": os.path.relpath(PKG, REPO), "checks": checks,
           "host_fsm_ms": host_ms, "receiver_open_fraction": sq2_open, "configs": {}}
    for name in cfg:
        t = per_call[name]
        med = statistics.median(t)
        c = {"call_ms_median": round(med, 4), "call_ms_min": round(min(t), 4), "call_ms_max": round(max(t), 4),
             "call_ms_rounds": [round(v, 4) for v in t], "kernels_ms_per_call": kernels[name]}
        if name in info:
            C, n, B, frac, tile = info[name]
            total = C * n
            per = 8.0 if name.startswith("m_") else 16.0 + 8.0 * frac
            floor = per * total / HBM * 1e3
            kms = sum(v for k, v in kernels[name].items() if k.startswith("k_sqbank"))
            c.update({"C": C, "block": B, "tile": tile, "gsamples_per_s": round(total / med / 1e6, 2),
                      "floor_ms_bytes": round(floor, 5), "share_of_floor_kernels": round(floor / kms, 4) if kms else None,
                      "share_of_floor_call": round(floor / med, 4)})
        if name[0] in "rs":
            c["gsamples_per_s"] = round(wide_n / med / 1e6, 2)
        res["configs"][name] = c
    cf = res["configs"]
    for key, (C, n) in shapes.items():
        for B in blocks:
            tag = f"{C}_b{B}"
            for new, old in ((f"m_measure_{tag}", f"p_torch_power_{tag}"), (f"c_call_{tag}", f"g_torch_power_gate_{tag}")):
                res[f"speedup_{new[0]}_over_{old[0]}_{tag}"] = round(cf[old]["call_ms_median"] / cf[new]["call_ms_median"], 2)
    ok = all(c["status_is_a_function_of_level"] and c["gated_rows_equal_baseline"] and
             c["level_max_diff_over_row_max"] <= 1e-5 for c in checks.values())
    res["checks_pass"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("squelchbank_bench: the bank and the baseline disagree")


if __name__ == "__main__":
    main()
