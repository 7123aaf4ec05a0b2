"""FMBank timing on the GPU, device tensors, two shapes of 64 Mi input samples and
eight configurations alternated in one process:
  a  FMBank(16, kf, 8)  on complex64[16, 4 Mi]                k_fmbank, 97 taps
  b  the 16 rows of a without the FMBank: per row FreqDem, RealFIRFilter(a.taps)
     and [::8] copied into a preallocated [16, n / 8] tensor (a's scale left out):
     48 launches, the full-rate float32 discriminator output written and read back
  c  FMBank(256, kf, 4) on complex64[256, 256 Ki]             k_fmbank, 49 taps
  d  the 256 rows of c the same way: 768 launches
  e  FMBank(16, kf)     on a's input, the discriminator alone  k_fmbank_disc
  f  16 per-row FreqDem calls on a's input
  g  FMBank(256, kf)    on c's input
  h  256 per-row FreqDem calls on c's input
b, d, f and h run code the FMBank does not touch: they are the yardstick.
Per configuration: FMBENCH_ROUNDS rounds of FMBENCH_CALLS calls between two
device events (per-call time of each round; their median and spread), then the
per-kernel times of a separate pass under the library's profile hooks.  The
floor of an FMBank configuration is the larger of its algorithmic bytes
(8 B in + 4 / D B out per input sample) over 8 TB/s and its VALU work over the
float32 VALU rate (256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz): the
discriminator's instructions per sample plus L / D multiply-adds.  The
discriminator's count is read from the built kernel's ISA (hipcc --save-temps
on csrc/k_fmbank.hip, k_fmbank_disc's one-sample loop): 144 VALU instructions,
4 of them packed float32 (two passes each), loads' address arithmetic and
lm_atan2f's selects and two IEEE divisions included.  Before the timing, row 5
of a and of b over the first 256 Ki samples are compared (fresh objects).
Fails without a GPU and when the rows differ by more than 2e-6 of the row's
maximum; it sets no speed threshold.  Prints one JSON line (and writes it to
the file named by --out).  LDSP_PKG_DIR selects the package build."""
import json
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
VALU = 256 * 4 * 32 * 2.4e9        # float32 lane operations / s (v_fma_f32, not packed)
DISC_VALU = 144 + 4                # VALU issue slots per sample of the discriminator (see above)
KF = 0.25


class Baseline:
    """Rows of a bank from the API without the FMBank: per row FreqDem, then (decim > 1) a
    full-rate RealFIRFilter and a strided copy."""

    def __init__(self, C, n, D, taps):
        self.D = D
        self.dems = [L.FreqDem(KF) for _ in range(C)]
        self.firs = [L.RealFIRFilter(taps) for _ in range(C)] if D > 1 else None
        self.out = torch.empty((C, n // D), dtype=torch.float32, device="cuda")

    def __call__(self, x):
        for k, dem in enumerate(self.dems):
            d = dem(x[k])
            self.out[k].copy_(self.firs[k](d)[::self.D] if self.firs else d)
        return self.out


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("fmbank_bench: needs a GPU")
    shapes = {"16": (16, int(os.environ.get("FMBENCH_N16", 4 << 20)), 8),
              "256": (256, int(os.environ.get("FMBENCH_N256", 256 << 10)), 4)}
    rounds = int(os.environ.get("FMBENCH_ROUNDS", 6))
    calls = int(os.environ.get("FMBENCH_CALLS", 4))
    assert rounds >= 3 and all(n % 256 == 0 for _, n, _ in shapes.values())
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    xs = {k: torch.complex(torch.randn((C, n), generator=g, device="cuda"), torch.randn((C, n), generator=g, device="cuda"))
          for k, (C, n, _) in shapes.items()}

    # row 5 both ways, fresh objects
    C, n, D = shapes["16"]
    nchk = min(n, 256 << 10)
    chk = L.FMBank(C, KF, D)
    xc = xs["16"][:, :nchk]
    ya = chk(xc)[5].cpu().numpy().astype(np.float64)
    yb = Baseline(6, nchk, D, chk.taps)(xc[:6])[5].cpu().numpy().astype(np.float64) * np.float64(chk.scale)
    row5 = float(np.max(np.abs(ya - yb)) / np.max(np.abs(yb)))
    del ya, yb, chk, xc

    banks, cfg = {}, {}
    for (key, (C, n, D)), (fb, base, fd, based) in zip(shapes.items(), (("a", "b", "e", "f"), ("c", "d", "g", "h"))):
        x = xs[key]
        bank, disc = L.FMBank(C, KF, D), L.FMBank(C, KF)
        base_f, base_d = Baseline(C, n, D, bank.taps), Baseline(C, n, 1, None)
        names = (f"{fb}_fmbank_{C}_d{D}", f"{base}_{C}x_freqdem_fir_slice", f"{fd}_fmbank_{C}_disc", f"{based}_{C}x_freqdem")
        banks[names[0]], banks[names[2]] = bank, disc
        for name, fn in zip(names, (bank, base_f, disc, base_d)):
            cfg[name] = (lambda fn=fn, x=x: fn(x))
    cfg = dict(sorted(cfg.items()))
    for fn in cfg.values():        # warm-up: code objects, history buffers, torch's allocator
        fn()
        fn()
    torch.cuda.synchronize()
    per_call = {k: [] for k in cfg}
    for _ in range(rounds):
        for name, fn in cfg.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            per_call[name].append(e0.elapsed_time(e1) / calls)
    kernels = {}
    for name, fn in cfg.items():
        L._profile_reset()
        L._profile_enable(True)
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        L._profile_enable(False)
        kernels[name] = {k: round(tot / c, 4) for k, (c, tot) in L._profile_report().items()}

    res = {"shapes": {k: {"C": v[0], "n_per_row": v[1], "D": v[2]} for k, v in shapes.items()}, "rounds": rounds,
           "calls_per_round": calls, "pkg": os.path.relpath(PKG, REPO), "disc_valu_per_sample": DISC_VALU,
           "row5_max_diff_over_max_256Ki": row5, "configs": {}}
    for name in cfg:
        t = per_call[name]
        med = statistics.median(t)
        key = "16" if "_16" in name else "256"
        total = shapes[key][0] * shapes[key][1]
        c = {"call_ms_median": round(med, 4), "call_ms_min": round(min(t), 4), "call_ms_max": round(max(t), 4),
             "call_ms_rounds": [round(v, 4) for v in t], "kernels_ms": kernels[name],
             "gsamples_per_s": round(total / med / 1e6, 2)}
        fb = banks.get(name)
        if fb is not None:
            D, Lh = fb.decim, len(fb.taps)
            nbytes = 8 + 4 / D
            valu = DISC_VALU + Lh / D
            t_bytes, t_valu = nbytes * total / HBM * 1e3, valu * total / VALU * 1e3
            floor = max(t_bytes, t_valu)
            kms = sum(kernels[name].values())
            c.update({"C": fb.nchan, "D": D, "L": Lh, "tile": fb.tile, "bytes_per_sample": nbytes,
                      "valu_per_sample": round(valu, 2), "floor_ms_bytes": round(t_bytes, 4),
                      "floor_ms_valu": round(t_valu, 4), "binds": "bytes" if t_bytes >= t_valu else "valu",
                      "share_of_floor_kernel": round(floor / kms, 4) if kms else None,
                      "share_of_floor_call": round(floor / med, 4)})
        res["configs"][name] = c

    cf = res["configs"]
    names = list(cf)
    for new, old in ((names[0], names[1]), (names[2], names[3]), (names[4], names[5]), (names[6], names[7])):
        key = new[0] + "_over_" + old[0]
        res["spread_ms_" + key] = round(max(cf[new]["call_ms_max"] - cf[new]["call_ms_min"],
                                            cf[old]["call_ms_max"] - cf[old]["call_ms_min"]), 4)
        res["speedup_" + key] = round(cf[old]["call_ms_median"] / cf[new]["call_ms_median"], 2)
    res["row5_agrees"] = bool(row5 <= 2e-6)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not res["row5_agrees"]:
        sys.exit("fmbank_bench: row 5 differs from the per-row FreqDem / RealFIRFilter path")


if __name__ == "__main__":
    main()
