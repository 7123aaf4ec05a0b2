"""Channelizer timing on the GPU at 64 Mi wideband samples, device tensors, four
configurations alternated in one process:
  a  Channelizer(16, 8, m=6)       2x oversampled    k_chan<16, 8>
  b  Channelizer(256, 128, m=6)    2x oversampled    k_chan<256, 128>
  c  Channelizer(16, 16, m=6)      critically sampled k_chan<16, 16>
  d  the 16 rows of a without the Channelizer: per channel k,
     mix_down_filter(NCO at 2 pi k / 16, ComplexFIRFilter(a.taps), x)[::8] copied
     into a preallocated [16, n / 8] tensor (a's scale left out)
Per configuration: CHANBENCH_ROUNDS rounds of CHANBENCH_CALLS calls between two
device events (per-call time of each round; their median and spread), then the
per-kernel times of a separate pass under the library's profile hooks.  The
floor of a Channelizer configuration is the larger of its algorithmic bytes
(8 B in + 8 M / D B out per wideband sample) over 8 TB/s and its flops
(4 L / D for the branch sums + 5 M log2(M) / D for the DFT per wideband sample)
over the float32 VALU rate (256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz).
Before the timing, row 5 of a and of d over the first 4 Mi samples are compared
(fresh objects).  Fails without a GPU, when a is slower than d by more than the
spread between rounds, and when the rows differ by more than 2e-6 of the
row's maximum.  Prints one JSON line (and writes it to the file named by
--out).  LDSP_PKG_DIR selects the package build."""
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
VALU = 256 * 4 * 32 * 2.4e9        # float32 lane operations / s (v_mul_f32 / v_add_f32, not packed)


class Baseline:
    """The M = 16, D = 8 rows from the API without the Channelizer."""

    def __init__(self, taps, n, M=16, D=8):
        self.M, self.D = M, D
        self.ncos, self.firs = [], []
        for k in range(M):
            nco = L.NCO("nco")
            nco.freq = np.float32(2 * np.pi * k / M)
            assert nco.state()[1] == (k << 32) // M          # the phase step is exact: no drift over the run
            self.ncos.append(nco)
            self.firs.append(L.ComplexFIRFilter(taps))
        self.out = torch.empty((M, n // D), dtype=torch.complex64, device="cuda")

    def __call__(self, x):
        for k in range(self.M):
            self.out[k].copy_(L.mix_down_filter(self.ncos[k], self.firs[k], x)[::self.D])
        return self.out


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("channelizer_bench: needs a GPU")
    n = int(os.environ.get("CHANBENCH_N", 64 << 20))
    rounds = int(os.environ.get("CHANBENCH_ROUNDS", 6))
    calls = int(os.environ.get("CHANBENCH_CALLS", 4))
    assert rounds >= 3 and n % 256 == 0
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.complex(torch.randn(n, generator=g, device="cuda"), torch.randn(n, generator=g, device="cuda"))

    # row 5 both ways, fresh objects
    nchk = min(n, 4 << 20)
    ca = L.Channelizer(16, 8, m=6)
    ya = ca(x[:nchk])[5].cpu().numpy().astype(np.complex128)
    yb = Baseline(ca.taps, nchk)(x[:nchk])[5].cpu().numpy().astype(np.complex128) * np.float64(ca.scale)
    row5 = float(np.max(np.abs(ya - yb)) / np.max(np.abs(yb)))
    del ya, yb

    chans = {"a_chan_16_8": L.Channelizer(16, 8, m=6), "b_chan_256_128": L.Channelizer(256, 128, m=6),
             "c_chan_16_16": L.Channelizer(16, 16, m=6)}
    base = Baseline(chans["a_chan_16_8"].taps, n)
    cfg = {name: (lambda c=c: c(x)) for name, c in chans.items()}
    cfg["d_16x_mix_down_filter"] = lambda: base(x)
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
        ch = chans.get(name)
        if ch is not None:
            M, D, Lh = ch.nchan, ch.decim, len(ch.taps)
            nbytes = 8 + 8 * M / D
            flops = 4 * Lh / D + 5 * M * math.log2(M) / D
            t_bytes, t_valu = nbytes * n / HBM * 1e3, flops * n / VALU * 1e3
            floor = max(t_bytes, t_valu)
            kms = sum(kernels[name].values())
            c.update({"M": M, "D": D, "L": Lh, "bytes_per_sample": nbytes, "flops_per_sample": round(flops, 2),
                      "floor_ms_bytes": round(t_bytes, 4), "floor_ms_valu": round(t_valu, 4),
                      "binds": "bytes" if t_bytes >= t_valu else "valu",
                      "share_of_floor_kernel": round(floor / kms, 4) if kms else None,
                      "share_of_floor_call": round(floor / med, 4)})
        res["configs"][name] = c
    a, d = res["configs"]["a_chan_16_8"], res["configs"]["d_16x_mix_down_filter"]
    spread = max(a["call_ms_max"] - a["call_ms_min"], d["call_ms_max"] - d["call_ms_min"])
    res["spread_ms"] = round(spread, 4)
    res["a_not_slower_than_d"] = bool(a["call_ms_median"] <= d["call_ms_median"] + spread)
    res["speedup_a_over_d"] = round(d["call_ms_median"] / a["call_ms_median"], 2)
    res["row5_agrees"] = bool(row5 <= 2e-6)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not res["a_not_slower_than_d"]:
        sys.exit("channelizer_bench: the Channelizer is slower than 16 mix_down_filter passes")
    if not res["row5_agrees"]:
        sys.exit("channelizer_bench: row 5 differs from the mix_down_filter path")


if __name__ == "__main__":
    main()
