"""ToneBank timing on the GPU, device tensors, two shapes of 64 Mi real input samples
(16 rows of 4 Mi, 256 rows of 256 Ki) at (F, B) = (50, 4096) and (8, 256), the
configurations alternated in one process:
  m  tb.measure(x)                        k_tonebank_power, k_tonebank_detect
  c  tb(x)                                the two and k_tonebank_gate
  p  the torch baseline of m's device work: X = x.view(C nb, B) @ tables.view(2F, B).T
     (a vendor GEMM), p = Xre^2 + Xim^2, max / argmax over the tones, the floor and the
     dominance test in float32
  g  the torch baseline of c's device work: p as above and
     x.view(C, nb, B) * hit[:, :, None]
Then
  r  Channelizer(256, 128) -> SquelchBank(256) -> FMBank(256, kf, 4) -> AudioBank(256, ..)
  s  the same with ToneBank(256, ctcss, 4096) between the FMBank and the AudioBank
on 64 Mi wideband samples, end to end.
Even rows carry a listed tone of amplitude 0.2 in noise of sigma 0.05, odd rows the noise
alone, hold = 0: about half of the blocks are open.  Before the timing the bank's tone
and open must equal the numpy rule (tests/tonebank_model.py) over its own power, its power
must agree with the baseline's to 1e-5 of the row's maximum, and its gated rows must equal
the product of the input with its own open flags.  Per configuration: TBBENCH_ROUNDS rounds
(12), each of enough calls to fill TBBENCH_WINDOW_MS between two device events on the
object's stream (per-call time of each round; their median and min-max), then the
per-kernel times of a separate pass under the library's profile hooks.
Floors: 4 F_padded flops per sample (F_padded = 16 ceil(F / 16), the zero rows included)
over the f32 matrix peak of 157.3 TFLOPS, and 4 B per sample (8 with the gate: closed
blocks are written and not read, open ones read again) over 8 TB/s.  Fails without a
GPU and when a check fails; it sets no speed threshold.  Prints one JSON line (and writes
it to the file named by --out).  LDSP_PKG_DIR selects the package build."""
import json
import math
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("LDSP_PKG_DIR") or os.path.join(REPO, "python-liquiddsp_amd")
sys.path[:0] = [REPO, PKG, os.path.join(REPO, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import liquiddsp as L  # noqa: E402
import tonebank_model as M  # noqa: E402

HBM = 8.0e12                       # bytes / s
PEAK = 157.3e12                    # f32 matrix flops / s
DOM, FLOOR = 8.0, 1e-3
KF, RATE, SR = 0.25, 0.192, 250e3
CTCSS = [67.0, 69.3, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8,
         118.8, 123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3,
         179.9, 183.5, 186.2, 189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3,
         254.1]


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("tonebank_bench: needs a GPU")
    shapes = {"16": (16, int(os.environ.get("TBBENCH_N16", 4 << 20))),
              "256": (256, int(os.environ.get("TBBENCH_N256", 256 << 10)))}
    banks = {"f50_b4096": (np.array(CTCSS) / 8000.0, 4096), "f8_b256": ((np.arange(8) + 1.5) * 0.05, 256)}
    wide_n = int(os.environ.get("TBBENCH_WIDE", 64 << 20))
    rounds = int(os.environ.get("TBBENCH_ROUNDS", 12))
    window = float(os.environ.get("TBBENCH_WINDOW_MS", 20.0))
    assert rounds >= 3
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    wide = torch.complex(torch.randn(wide_n, generator=g, device="cuda"), torch.randn(wide_n, generator=g, device="cuda"))

    cfg, info, checks = {}, {}, {}
    for key, (C, n) in shapes.items():
        for bname, (f, B) in banks.items():
            F, nb = len(f), n // B
            tag = f"{C}_{bname}"
            t = torch.arange(n, device="cuda", dtype=torch.float64)
            fr = torch.from_numpy(f[np.arange(C) % F]).to("cuda")[:, None]
            amp = torch.where(torch.arange(C, device="cuda") % 2 == 0, 0.2, 0.0)[:, None]
            x = (amp * torch.cos(2 * math.pi * fr * t)).float() + 0.05 * torch.randn((C, n), generator=g, device="cuda")
            del t

            def mk(C=C, f=f, B=B):
                return L.ToneBank(C, f, block=B, dominance=DOM, floor=FLOOR, hold=0)

            tb = mk()
            tabT = torch.from_numpy(tb.tables.reshape(2 * F, B)).to("cuda").T.contiguous()

            def base_p(x=x, C=C, nb=nb, B=B, F=F, tabT=tabT):
                X = x.view(C * nb, B) @ tabT
                p = X[:, :F] ** 2 + X[:, F:] ** 2
                best, k = p.max(dim=1)
                hit = (best > FLOOR) & (best * (F - 1) > DOM * (p.sum(dim=1) - best))
                return p, k, hit

            # the checks, on a fresh object
            y = tb(x)
            pw, tn, op = tb.power.cpu().numpy(), tb.tone.cpu().numpy(), tb.open.cpu().numpy()
            tone, opn, _, _ = M.decide(pw, FLOOR, DOM, -1, 0, np.full(C, M.SAT))
            bp = base_p()[0].view(C, nb, F).cpu().numpy().astype(np.float64)
            den = np.maximum(bp.max(axis=(1, 2), keepdims=True), 1e-30)
            mask = torch.from_numpy(op.astype(bool)).to("cuda")
            by = (x.view(C, nb, B) * mask[:, :, None]).view(C, nb * B)
            checks[tag] = {"tone_and_open_follow_the_rule": bool((tn == tone).all() and (op == opn).all()),
                           "power_max_diff_over_row_max": float(np.max(np.abs(pw.astype(np.float64) - bp) / den)),
                           "gated_rows_equal_product": bool(torch.equal(y, by)),
                           "open_fraction": float(op.mean())}
            del y, by
            bank_m, bank_c = mk(), mk()
            info[f"m_measure_{tag}"] = info[f"c_call_{tag}"] = (C, n, B, F, float(op.mean()), tb.tile)
            cfg[f"m_measure_{tag}"] = (lambda b=bank_m, x=x: b.measure(x))
            cfg[f"c_call_{tag}"] = (lambda b=bank_c, x=x: b(x))
            cfg[f"p_torch_measure_{tag}"] = base_p
            cfg[f"g_torch_measure_gate_{tag}"] = (lambda x=x, C=C, nb=nb, B=B, f=base_p:
                                                 x.view(C, nb, B) * f()[2].view(C, nb)[:, :, None])
    ctcss = np.array(CTCSS) / 8000.0
    ch, sq, fm, au = L.Channelizer(256, 128), L.SquelchBank(256), L.FMBank(256, KF, 4), L.AudioBank(256, RATE, deemphasis=SR)
    ch2, sq2, fm2 = L.Channelizer(256, 128), L.SquelchBank(256), L.FMBank(256, KF, 4)
    tb2, au2 = L.ToneBank(256, ctcss, 4096), L.AudioBank(256, RATE, deemphasis=SR)
    cfg["r_channelizer_squelchbank_fmbank_audiobank_256"] = lambda: au(fm(sq(ch(wide))))
    cfg["s_channelizer_squelchbank_fmbank_tonebank_audiobank_256"] = lambda: au2(tb2(fm2(sq2(ch2(wide)))))
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

    res = {"shapes": {k: {"C": v[0], "n_per_row": v[1]} for k, v in shapes.items()},
           "banks": {k: {"F": len(v[0]), "block": v[1]} for k, v in banks.items()}, "wideband_samples": wide_n,
           "dominance": DOM, "floor": FLOOR, "hold": 0, "rounds": rounds, "window_ms": window, "calls_per_round": calls,
           "pkg": os.path.relpath(PKG, REPO), "checks": checks, "configs": {}}
    for name in cfg:
        t = per_call[name]
        med = statistics.median(t)
        c = {"call_ms_median": round(med, 4), "call_ms_min": round(min(t), 4), "call_ms_max": round(max(t), 4),
             "call_ms_rounds": [round(v, 4) for v in t], "kernels_ms_per_call": kernels[name]}
        if name in info:
            C, n, B, F, frac, tile = info[name]
            total = C * n
            fpad = 16 * ((F + 15) // 16)
            floor_flops = 4.0 * fpad * total / PEAK * 1e3
            floor_bytes = (4.0 if name.startswith("m_") else 8.0) * total / HBM * 1e3
            floor = max(floor_flops, floor_bytes)
            kms = sum(v for k, v in kernels[name].items() if k.startswith("k_tonebank"))
            c.update({"C": C, "block": B, "F": F, "tile": tile, "gsamples_per_s": round(total / med / 1e6, 2),
                      "floor_ms_flops": round(floor_flops, 5), "floor_ms_bytes": round(floor_bytes, 5),
                      "share_of_floor_kernels": round(floor / kms, 4) if kms else None,
                      "share_of_floor_call": round(floor / med, 4)})
        if name[0] in "rs":
            c["gsamples_per_s"] = round(wide_n / med / 1e6, 2)
        res["configs"][name] = c
    cf = res["configs"]
    for key, (C, n) in shapes.items():
        for bname in banks:
            tag = f"{C}_{bname}"
            for new, old in ((f"m_measure_{tag}", f"p_torch_measure_{tag}"), (f"c_call_{tag}", f"g_torch_measure_gate_{tag}")):
                res[f"speedup_{new[0]}_over_{old[0]}_{tag}"] = round(cf[old]["call_ms_median"] / cf[new]["call_ms_median"], 2)
    ok = all(c["tone_and_open_follow_the_rule"] and c["gated_rows_equal_product"] and
             c["power_max_diff_over_row_max"] <= 1e-5 for c in checks.values())
    res["checks_pass"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("tonebank_bench: the bank and the baseline disagree")


if __name__ == "__main__":
    main()
