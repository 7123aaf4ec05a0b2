"""Downconverter timing on the GPU at 64 Mi wideband samples, device tensors, five
configurations alternated in one process:
  a  Downconverter(16 seeded off-grid frequencies, 64, m=6)    k_ddc, four tuners per wave
  b  Downconverter(the first of them, 64, m=6)                 k_ddc, one tuner per wave
  c  Downconverter(64 seeded frequencies, 128, m=6)            k_ddc, four tuners per wave
  d  the 16 rows of a without the Downconverter: per tuner,
     mix_down_filter(table NCO, ComplexFIRFilter(a.taps), x)[::64] copied into a
     preallocated [16, n / 64] tensor (a's scale left out)
  e  one such pass, against b
d and e run code the Downconverter does not touch: they are the yardstick.
Per configuration: DDCBENCH_ROUNDS rounds of DDCBENCH_CALLS calls between two
device events (per-call time of each round; their median and spread), then the
per-kernel times of a separate pass under the library's profile hooks.  The
floor of a Downconverter configuration is the larger of its algorithmic bytes
(8 B in + 8 C / D B out per wideband sample) over 8 TB/s and its multiply-adds
(4 C L / D per wideband sample) over the float32 VALU rate (256 CUs x 4 SIMDs x
32 lanes per clock at 2.4 GHz).  Before the timing, row 5 of an on-grid check
bank (16 tuners at k / 16, where the table NCO is exact) and of the
mix_down_filter path over the first 4 Mi samples are compared (fresh objects).
Fails without a GPU, when a is slower than d or b slower than e by more than
the spread between rounds, and when the rows differ by more than 2e-6 of the
row's maximum.  Prints one JSON line (and writes it to the file named by
--out).  LDSP_PKG_DIR selects the package build."""
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


class Baseline:
    """Rows of a bank from the API without the Downconverter: one full-rate pass per tuner."""

    def __init__(self, freqs, taps, n, D, exact=False):
        self.D = D
        self.ncos, self.firs = [], []
        for f in freqs:
            nco = L.NCO("nco")
            nco.freq = np.float32(2 * np.pi * f)
            if exact:                                            # the phase step is the tuner's word: no drift
                assert nco.state()[1] == int(np.rint(f * 2.0 ** 32)) % 2 ** 32
            self.ncos.append(nco)
            self.firs.append(L.ComplexFIRFilter(taps))
        self.out = torch.empty((len(freqs), n // D), dtype=torch.complex64, device="cuda")

    def __call__(self, x):
        for k in range(len(self.ncos)):
            self.out[k].copy_(L.mix_down_filter(self.ncos[k], self.firs[k], x)[::self.D])
        return self.out


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("downconverter_bench: needs a GPU")
    n = int(os.environ.get("DDCBENCH_N", 64 << 20))
    rounds = int(os.environ.get("DDCBENCH_ROUNDS", 6))
    calls = int(os.environ.get("DDCBENCH_CALLS", 4))
    assert rounds >= 3 and n % 256 == 0
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.complex(torch.randn(n, generator=g, device="cuda"), torch.randn(n, generator=g, device="cuda"))

    # row 5 both ways on the grid the table NCO is exact on, fresh objects
    nchk = min(n, 4 << 20)
    grid = [k / 16 for k in range(16)]
    chk = L.Downconverter(grid, 64, m=6)
    ya = chk(x[:nchk])[5].cpu().numpy().astype(np.complex128)
    yb = Baseline(grid[5:6], chk.taps, nchk, 64, exact=True)(x[:nchk])[0].cpu().numpy().astype(np.complex128)
    yb *= np.float64(chk.scale)
    row5 = float(np.max(np.abs(ya - yb)) / np.max(np.abs(yb)))
    del ya, yb, chk

    rng = np.random.default_rng(1)
    f16, f64 = rng.uniform(-0.5, 0.5, 16), rng.uniform(-0.5, 0.5, 64)
    banks = {"a_ddc_16_d64": L.Downconverter(f16, 64, m=6), "b_ddc_1_d64": L.Downconverter(f16[:1], 64, m=6),
             "c_ddc_64_d128": L.Downconverter(f64, 128, m=6)}
    taps = banks["a_ddc_16_d64"].taps
    base16, base1 = Baseline(f16, taps, n, 64), Baseline(f16[:1], taps, n, 64)
    cfg = {name: (lambda c=c: c(x)) for name, c in banks.items()}
    cfg["d_16x_mix_down_filter"] = lambda: base16(x)
    cfg["e_1x_mix_down_filter"] = lambda: base1(x)
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

    res = {"n": n, "rounds": rounds, "calls_per_round": calls, "pkg": os.path.relpath(PKG, REPO),
           "row5_max_diff_over_max_4Mi": row5, "configs": {}}
    for name, fn in cfg.items():
        t = per_call[name]
        med = statistics.median(t)
        c = {"call_ms_median": round(med, 4), "call_ms_min": round(min(t), 4), "call_ms_max": round(max(t), 4),
             "call_ms_rounds": [round(v, 4) for v in t], "kernels_ms": kernels[name],
             "gsamples_per_s": round(n / med / 1e6, 2)}
        dc = banks.get(name)
        if dc is not None:
            C, D, Lh = dc.ntuners, dc.decim, len(dc.taps)
            nbytes = 8 + 8 * C / D
            macs = 4 * C * Lh / D
            t_bytes, t_valu = nbytes * n / HBM * 1e3, macs * n / VALU * 1e3
            floor = max(t_bytes, t_valu)
            kms = sum(kernels[name].values())
            c.update({"C": C, "D": D, "L": Lh, "tile": dc.tile, "bytes_per_sample": nbytes,
                      "macs_per_sample": round(macs, 2), "floor_ms_bytes": round(t_bytes, 4),
                      "floor_ms_valu": round(t_valu, 4), "binds": "bytes" if t_bytes >= t_valu else "valu",
                      "share_of_floor_kernel": round(floor / kms, 4) if kms else None,
                      "share_of_floor_call": round(floor / med, 4)})
        res["configs"][name] = c

    def spread(p, q):
        return max(p["call_ms_max"] - p["call_ms_min"], q["call_ms_max"] - q["call_ms_min"])

    cf = res["configs"]
    for new, old, key in (("a_ddc_16_d64", "d_16x_mix_down_filter", "a_over_d"),
                          ("b_ddc_1_d64", "e_1x_mix_down_filter", "b_over_e")):
        s = spread(cf[new], cf[old])
        res["spread_ms_" + key] = round(s, 4)
        res["not_slower_" + key] = bool(cf[new]["call_ms_median"] <= cf[old]["call_ms_median"] + s)
        res["speedup_" + key] = round(cf[old]["call_ms_median"] / cf[new]["call_ms_median"], 2)
    res["row5_agrees"] = bool(row5 <= 2e-6)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not res["not_slower_a_over_d"]:
        sys.exit("downconverter_bench: 16 tuners are slower than 16 mix_down_filter passes")
    if not res["not_slower_b_over_e"]:
        sys.exit("downconverter_bench: one tuner is slower than one mix_down_filter pass")
    if not res["row5_agrees"]:
        sys.exit("downconverter_bench: row 5 differs from the mix_down_filter path")


if __name__ == "__main__":
    main()
