"""AudioBank timing on the GPU, device tensors, two shapes (8 Mi and 16 Mi input
samples) and nine configurations alternated in one process (rate 0.192: 250 kS/s
rows to 48 kS/s):
  a  AudioBank(16, 0.192, deemphasis=250e3)  on float32[16, 512 Ki]        k_audiobank
  b  the 16 rows of a without the AudioBank: per row DeemphasisFilter(250e3) and
     RealResampler(0.192), copied into a preallocated [16, nout] tensor
  c  AudioBank(256, 0.192, deemphasis=250e3) on float32[256, 64 Ki]
  d  the 256 rows of c the same way
  e  AudioBank(16, 0.192)  on a's input, the resampler alone
  f  16 per-row RealResampler calls on a's input
  g  AudioBank(256, 0.192) on c's input
  h  256 per-row RealResampler calls on c's input
  i  Channelizer(16, 8) -> FMBank(16, kf, 8) -> AudioBank(16, 0.192, deemphasis=...)
     on 64 Mi wideband samples, end to end (three launches)
b, d, f and h run code the AudioBank does not touch: they are the yardstick.
Before the timing, fresh objects of e / f and of g / h run their inputs once and
every row must be bit-equal; the difference of row 5 of a and of b over the
row's maximum is reported (b's de-emphasis keeps liquid's float32 state).  Per
configuration: ABBENCH_ROUNDS rounds, each of enough calls to fill
ABBENCH_WINDOW_MS between two device events (per-call time of each round; their
median and spread), then the per-kernel times of a separate pass under the
library's profile hooks.  The floor of an AudioBank configuration is its
algorithmic bytes (4 B in + 4 rate B out per input sample) over 8 TB/s.  Fails
without a GPU and when the resampler-alone rows differ; it sets no speed
threshold.  Prints one JSON line (and writes it to the file named by --out).
LDSP_PKG_DIR selects the package build."""
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
RATE = 0.192
SR = 250e3
KF = 0.25


class Baseline:
    """Rows of a bank from the API without the AudioBank: per row DeemphasisFilter (optional)
    and RealResampler with the bank's design."""

    def __init__(self, bank, n, deemph):
        C = bank.nchan
        fc = float(np.float32(0.45 * min(float(np.float32(RATE)), 1.0)))
        self.des = [L.DeemphasisFilter(SR) for _ in range(C)] if deemph else None
        self.rss = [L.RealResampler(RATE, bank.len, fc, 60.0, bank.nfilter) for _ in range(C)]
        # the streams go on from call to call, so a call's count moves by one: room for the longest
        self.out = torch.empty((C, bank.num_outputs(n) + 2), dtype=torch.float32, device="cuda")

    def __call__(self, x):
        for k, rs in enumerate(self.rss):
            y = rs(self.des[k](x[k]) if self.des else x[k])
            self.out[k, :y.numel()].copy_(y)
        return self.out[:, :y.numel()]


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("audiobank_bench: needs a GPU")
    shapes = {"16": (16, int(os.environ.get("ABBENCH_N16", 512 << 10))),
              "256": (256, int(os.environ.get("ABBENCH_N256", 64 << 10)))}
    wide_n = int(os.environ.get("ABBENCH_WIDE", 64 << 20))
    rounds = int(os.environ.get("ABBENCH_ROUNDS", 6))
    window = float(os.environ.get("ABBENCH_WINDOW_MS", 20.0))
    assert rounds >= 3
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    xs = {k: torch.randn((C, n), generator=g, device="cuda") for k, (C, n) in shapes.items()}
    wide = torch.complex(torch.randn(wide_n, generator=g, device="cuda"), torch.randn(wide_n, generator=g, device="cuda"))

    banks, cfg, checks = {}, {}, {}
    for (key, (C, n)), (ab, base, rs, baser) in zip(shapes.items(), (("a", "b", "e", "f"), ("c", "d", "g", "h"))):
        x = xs[key]
        bank, alone = L.AudioBank(C, RATE, deemphasis=SR), L.AudioBank(C, RATE)
        base_d, base_r = Baseline(bank, n, True), Baseline(alone, n, False)
        # the resampler alone: bit-equal rows before any timing
        ya, yb = L.AudioBank(C, RATE)(x).cpu().numpy(), Baseline(alone, n, False)(x).cpu().numpy()
        checks[f"{rs}_{baser}_bit_equal"] = bool(ya.shape == yb.shape and (ya.view(np.uint32) == yb.view(np.uint32)).all())
        if key == "16":
            ya = L.AudioBank(C, RATE, deemphasis=SR)(x)[5].cpu().numpy().astype(np.float64)
            yb = Baseline(bank, n, True)(x)[5].cpu().numpy().astype(np.float64)
            checks["row5_max_diff_over_max"] = float(np.max(np.abs(ya - yb)) / np.max(np.abs(yb)))
        names = (f"{ab}_audiobank_{C}_deemph", f"{base}_{C}x_deemph_resamp", f"{rs}_audiobank_{C}_resamp",
                 f"{baser}_{C}x_resamp")
        banks[names[0]], banks[names[2]] = bank, alone
        for name, fn in zip(names, (bank, base_d, alone, base_r)):
            cfg[name] = (lambda fn=fn, x=x: fn(x))
    ch, fm, au = L.Channelizer(16, 8), L.FMBank(16, KF, 8), L.AudioBank(16, RATE, deemphasis=SR)

    def receiver():
        return au(fm(ch(wide)))
    cfg["i_channelizer_fmbank_audiobank_16"] = receiver
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

    res = {"shapes": {k: {"C": v[0], "n_per_row": v[1]} for k, v in shapes.items()}, "wideband_samples": wide_n,
           "rate": RATE, "sample_rate": SR, "rounds": rounds, "window_ms": window, "calls_per_round": calls,
           "pkg": os.path.relpath(PKG, REPO), "checks": checks, "configs": {}}
    for name in cfg:
        t = per_call[name]
        med = statistics.median(t)
        c = {"call_ms_median": round(med, 4), "call_ms_min": round(min(t), 4), "call_ms_max": round(max(t), 4),
             "call_ms_rounds": [round(v, 4) for v in t], "kernels_ms_per_call": kernels[name]}
        bank = banks.get(name)
        if bank is not None:
            total = bank.nchan * shapes[str(bank.nchan)][1]
            floor = (4 + 4 * RATE) * total / HBM * 1e3
            kms = kernels[name].get("k_audiobank", 0.0)
            c.update({"C": bank.nchan, "tile": bank.tile, "gsamples_per_s": round(total / med / 1e6, 2),
                      "floor_ms_bytes": round(floor, 5), "share_of_floor_kernel": round(floor / kms, 4) if kms else None,
                      "share_of_floor_call": round(floor / med, 4)})
        if name.startswith("i_"):
            c["gsamples_per_s"] = round(wide_n / med / 1e6, 2)
        res["configs"][name] = c
    cf = res["configs"]
    names = list(cf)
    for new, old in ((names[0], names[1]), (names[2], names[3]), (names[4], names[5]), (names[6], names[7])):
        key = new[0] + "_over_" + old[0]
        res["speedup_" + key] = round(cf[old]["call_ms_median"] / cf[new]["call_ms_median"], 2)
    ok = all(v for k, v in checks.items() if k.endswith("bit_equal"))
    res["rows_agree"] = bool(ok)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("audiobank_bench: rows differ from the per-row RealResampler path")


if __name__ == "__main__":
    main()
