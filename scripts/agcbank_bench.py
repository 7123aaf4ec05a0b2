"""AGCBank timing on the GPU, device tensors, two shapes of 64 Mi real input samples
(16 rows of 4 Mi, 256 rows of 256 Ki) at block = 256 and block = 64, the
configurations alternated in one process:
  a  ag(x) with hang = 0                  k_agcbank_peak, k_agcbank_track, k_agcbank_apply
  d  ag(x) with the default hang = 8      the same three
  t  the torch baseline of a's device work, the same definition at hang = 0:
     x.abs().view(C, nb, B).amax(2), log2 in double, ceil and clamp,
     torch.cummax(l + j d) - j d, the gain, exp2, the boundary minima, the
     ramp and the product
Then
  r  Channelizer(256, 128) -> SSBBank(256, 2) -> AudioBank(256, 0.96, deemphasis=None)
  s  the same with AGCBank(256) in front of the AudioBank
on 64 Mi wideband samples, end to end.
Even rows are noise at -20 dB, odd rows noise at -60 dB, under an envelope that
drops by 20 dB for every other 4096 samples.  Before the timing the bank's
peak_q must lie within 2 units of the baseline's, its gain_q must equal the
baseline's recurrence over its own peak_q, and its output must lie within 1e-6
of the target of the baseline's product from its own gain_q.  Per
configuration: AGCBENCH_ROUNDS rounds (12), each of enough calls to fill
AGCBENCH_WINDOW_MS between two device events on the object's stream (per-call
time of each round; their median and min-max), then the per-kernel times of a
separate pass under the library's profile hooks.  Floors over 8 TB/s: the peak
kernel reads 4 B per sample, the apply kernel reads 4 B and writes 4 B; the
track kernel has no byte floor worth the name (12 B per block).  k_agcbank_track
at 16 rows of 65 536 blocks (block 64) stands beside 16 rows of 16 384 (block
256): how it grows with a row's blocks.  Fails without a GPU and when a check
fails; it sets no speed threshold.  Prints one JSON line (and writes it to the
file named by --out).  LDSP_PKG_DIR selects the package build."""
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("LDSP_PKG_DIR") or os.path.join(REPO, "python-liquiddsp_amd")
sys.path[:0] = [REPO, PKG]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import liquiddsp as L  # noqa: E402

HBM = 8.0e12                       # bytes / s
Q = float(1 << 24)
FLOOR, CEIL = -64.0 * Q, 64.0 * Q
TARGET, MAX_GAIN, DECAY = -12.0, 60.0, 0.5


def units(db):
    return float(np.rint(np.float64(db) * Q / (20 * np.log10(2.0))))


def torch_agc(x, C, nb, B, pq=None):
    """The definition at hang = 0 in torch; levels as float64 (integers below 2^53: exact).
    pq: take these peaks instead of the input's.  Returns (peak_q, gain_q, y)."""
    T, G, d = units(TARGET), units(MAX_GAIN), units(DECAY)
    if pq is None:
        a = x.abs().view(C, nb, B).amax(2)
        pq = torch.clamp(torch.ceil(torch.log2(a.double()) * Q), FLOOR, CEIL)
    j = torch.arange(nb, device=x.device, dtype=torch.float64) * d
    lev = torch.clamp(torch.cummax(pq + j, 1).values - j, min=FLOOR)
    gq = torch.clamp(T - lev, max=G)
    g = torch.exp2(gq / Q).float()
    h = torch.minimum(g[:, :-1], g[:, 1:])
    hm = torch.cat([g[:, :1], h[:, :-1]], 1)
    ramp = torch.arange(1, B + 1, device=x.device, dtype=torch.float32)
    gam = hm[:, :, None] + (h - hm)[:, :, None] * ramp[None, None, :] / float(B)
    y = x[:, :(nb - 1) * B].view(C, nb - 1, B) * gam
    return pq, gq, y.view(C, (nb - 1) * B)


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("agcbank_bench: needs a GPU")
    shapes = {"16": (16, int(os.environ.get("AGCBENCH_N16", 4 << 20))),
              "256": (256, int(os.environ.get("AGCBENCH_N256", 256 << 10)))}
    blocks = (256, 64)
    wide_n = int(os.environ.get("AGCBENCH_WIDE", 64 << 20))
    rounds = int(os.environ.get("AGCBENCH_ROUNDS", 12))
    window = float(os.environ.get("AGCBENCH_WINDOW_MS", 20.0))
    assert rounds >= 3
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    xs = {}
    for key, (C, n) in shapes.items():
        amp = torch.where(torch.arange(C, device="cuda") % 2 == 0, 0.1, 0.001)[:, None]
        env = torch.where((torch.arange(n, device="cuda") // 4096) % 2 == 0, 1.0, 0.1)[None, :]
        xs[key] = torch.randn((C, n), generator=g, device="cuda") * amp * env
    wide = torch.complex(torch.randn(wide_n, generator=g, device="cuda"), torch.randn(wide_n, generator=g, device="cuda"))
    tl = 10.0 ** (TARGET / 20.0)

    cfg, info, checks = {}, {}, {}
    for key, (C, n) in shapes.items():
        x = xs[key]
        for B in blocks:
            nb = n // B
            tag = f"{C}_b{B}"
            ag = L.AGCBank(C, B, TARGET, MAX_GAIN, 0, DECAY)
            y = ag(x)
            pq, gq = ag.peak_q, ag.gain_q
            tpq, _, _ = torch_agc(x, C, nb, B)
            _, tgq, ty = torch_agc(x, C, nb, B, pq.double())
            checks[tag] = {"peak_q_max_diff_units": float((pq.double() - tpq).abs().max()),
                           "gain_q_equals_recurrence_over_peak_q": bool(torch.equal(gq.double(), tgq)),
                           "y_max_diff_over_target": float((y - ty).abs().max()) / tl,
                           "y_max_over_target": float(y.abs().max()) / tl,
                           "gain_db_min": float(ag.gain_db.min()), "gain_db_max": float(ag.gain_db.max())}
            del y, ty, tpq, tgq
            bank_a, bank_d = L.AGCBank(C, B, TARGET, MAX_GAIN, 0, DECAY), L.AGCBank(C, B, TARGET, MAX_GAIN, 8, DECAY)
            info[f"a_call_hang0_{tag}"] = info[f"d_call_hang8_{tag}"] = (C, n, B)
            cfg[f"a_call_hang0_{tag}"] = (lambda b=bank_a, x=x: b(x))
            cfg[f"d_call_hang8_{tag}"] = (lambda b=bank_d, x=x: b(x))
            cfg[f"t_torch_hang0_{tag}"] = (lambda x=x, C=C, nb=nb, B=B: torch_agc(x, C, nb, B))
    ch, sb, au = L.Channelizer(256, 128), L.SSBBank(256, 2), L.AudioBank(256, 0.96, deemphasis=None)
    ch2, sb2, ag2, au2 = L.Channelizer(256, 128), L.SSBBank(256, 2), L.AGCBank(256), L.AudioBank(256, 0.96, deemphasis=None)
    cfg["r_channelizer_ssbbank_audiobank_256"] = lambda: au(sb(ch(wide)))
    cfg["s_channelizer_ssbbank_agcbank_audiobank_256"] = lambda: au2(ag2(sb2(ch2(wide))))
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

    res = {"shapes": {k: {"C": v[0], "n_per_row": v[1]} for k, v in shapes.items()}, "blocks": list(blocks),
           "wideband_samples": wide_n, "target_dB": TARGET, "max_gain_dB": MAX_GAIN, "decay_dB": DECAY, "rounds": rounds,
           "window_ms": window, "calls_per_round": calls, "pkg": os.path.relpath(PKG, REPO), "checks": checks,
           "configs": {}}
    for name in cfg:
        t = per_call[name]
        med = statistics.median(t)
        c = {"call_ms_median": round(med, 4), "call_ms_min": round(min(t), 4), "call_ms_max": round(max(t), 4),
             "call_ms_rounds": [round(v, 4) for v in t], "kernels_ms_per_call": kernels[name]}
        if name in info:
            C, n, B = info[name]
            total = C * n
            fp, fa = 4.0 * total / HBM * 1e3, 8.0 * total / HBM * 1e3
            k = kernels[name]
            c.update({"C": C, "block": B, "blocks_per_row": n // B, "gsamples_per_s": round(total / med / 1e6, 2),
                      "floor_ms_peak": round(fp, 5), "floor_ms_apply": round(fa, 5),
                      "share_of_floor_peak": round(fp / k["k_agcbank_peak"], 4) if k.get("k_agcbank_peak") else None,
                      "share_of_floor_apply": round(fa / k["k_agcbank_apply"], 4) if k.get("k_agcbank_apply") else None,
                      "share_of_floor_call": round((fp + fa) / med, 4)})
        if name[0] in "rs":
            c["gsamples_per_s"] = round(wide_n / med / 1e6, 2)
        res["configs"][name] = c
    cf = res["configs"]
    for key, (C, n) in shapes.items():
        for B in blocks:
            tag = f"{C}_b{B}"
            res[f"speedup_a_over_t_{tag}"] = round(cf[f"t_torch_hang0_{tag}"]["call_ms_median"] /
                                                   cf[f"a_call_hang0_{tag}"]["call_ms_median"], 2)
    for h in ("a_call_hang0", "d_call_hang8"):
        res[f"track_ms_{h}_16_rows"] = {str(cf[f"{h}_16_b{B}"]["blocks_per_row"]):
                                        cf[f"{h}_16_b{B}"]["kernels_ms_per_call"].get("k_agcbank_track") for B in blocks}
    res["receiver_agc_cost_ms"] = round(cf["s_channelizer_ssbbank_agcbank_audiobank_256"]["call_ms_median"] -
                                        cf["r_channelizer_ssbbank_audiobank_256"]["call_ms_median"], 4)
    ok = all(c["peak_q_max_diff_units"] <= 2 and c["gain_q_equals_recurrence_over_peak_q"] and
             c["y_max_diff_over_target"] <= 1e-6 and c["y_max_over_target"] <= 1 + 1e-6 for c in checks.values())
    res["checks_pass"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("agcbank_bench: the bank and the baseline disagree")


if __name__ == "__main__":
    main()
