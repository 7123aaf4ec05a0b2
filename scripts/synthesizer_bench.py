"""Synthesizer timing on the GPU at 64 Mi output samples, device tensors, four
configurations alternated in one process:
  a  Synthesizer(16, 8, m=6)       2x oversampled     k_synth<16, 8>
  b  Synthesizer(256, 128, m=6)    2x oversampled     k_synth<256, 128>
  c  Synthesizer(16, 16, m=6)      critically sampled k_synth<16, 16>
  d  the output of a without the Synthesizer: per row k, the row zero-stuffed by
     8 into a preallocated buffer, ComplexFIRFilter(a.taps), NCO.mix_up at
     2 pi k / 16, added into a preallocated sum (a's scale left out)
Per configuration: SYNBENCH_ROUNDS rounds of SYNBENCH_CALLS calls between two
device events (per-call time of each round; their median and spread), then the
per-kernel times of a separate pass under the library's profile hooks.  The
floor of a Synthesizer configuration is the larger of its algorithmic bytes
(8 M / D B in + 8 B out per output sample) over 8 TB/s and its lane operations
(4 L / D for the output sums + 5 M log2(M) / D for the DFT per output sample)
over the float32 VALU rate (256 CUs x 4 SIMDs x 32 lanes per clock at 2.4 GHz).
Before the timing, a and d over the first 4 Mi output samples are compared
(fresh objects); the figure is reported, and a difference above 1e-4 of the
maximum -- a wiring mistake, not rounding: the tests hold parity -- fails the
run.  Fails without a GPU and when a is slower than d by more than the spread
between rounds.  Prints one JSON line (and writes it to the file named by
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
    """The M = 16, D = 8 output from the API without the Synthesizer."""

    def __init__(self, taps, K, M=16, D=8):
        self.M, self.D = M, D
        self.ncos, self.firs = [], []
        for k in range(M):
            nco = L.NCO("nco")
            nco.freq = np.float32(2 * np.pi * k / M)
            assert nco.state()[1] == (k << 32) // M          # the phase step is exact: no drift over the run
            self.ncos.append(nco)
            self.firs.append(L.ComplexFIRFilter(taps))
        self.up = torch.zeros(K * D, dtype=torch.complex64, device="cuda")
        self.out = torch.empty(K * D, dtype=torch.complex64, device="cuda")

    def __call__(self, y):
        self.out.zero_()
        for k in range(self.M):
            self.up[::self.D] = y[k]
            self.out += self.ncos[k].mix_up(self.firs[k](self.up))
        return self.out


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("synthesizer_bench: needs a GPU")
    n = int(os.environ.get("SYNBENCH_N", 64 << 20))
    rounds = int(os.environ.get("SYNBENCH_ROUNDS", 6))
    calls = int(os.environ.get("SYNBENCH_CALLS", 4))
    assert rounds >= 3 and n % 256 == 0
    g = torch.Generator(device="cuda")
    g.manual_seed(1)

    def rows(M, K):
        return torch.complex(torch.randn((M, K), generator=g, device="cuda"),
                             torch.randn((M, K), generator=g, device="cuda"))

    syns = {"a_synth_16_8": L.Synthesizer(16, 8, m=6), "b_synth_256_128": L.Synthesizer(256, 128, m=6),
            "c_synth_16_16": L.Synthesizer(16, 16, m=6)}
    ins = {name: rows(s.nchan, n // s.interp) for name, s in syns.items()}

    # a and d, fresh objects, the first 4 Mi output samples
    nchk = min(n, 4 << 20)
    sa = L.Synthesizer(16, 8, m=6)
    ychk = ins["a_synth_16_8"][:, :nchk // 8]
    za = sa(ychk).cpu().numpy().astype(np.complex128)
    zb = Baseline(sa.taps, nchk // 8)(ychk).cpu().numpy().astype(np.complex128) * np.float64(sa.scale)
    diff = float(np.max(np.abs(za - zb)) / np.max(np.abs(zb)))
    del za, zb, ychk

    base = Baseline(syns["a_synth_16_8"].taps, n // 8)
    cfg = {name: (lambda s=s, y=ins[name]: s(y)) for name, s in syns.items()}
    cfg["d_16x_stuff_fir_mix_up_sum"] = lambda: base(ins["a_synth_16_8"])
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

    res = {"n_out": n, "rounds": rounds, "calls_per_round": calls, "pkg": os.path.relpath(PKG, REPO),
           "a_vs_d_max_diff_over_max_4Mi": diff, "configs": {}}
    for name, fn in cfg.items():
        t = per_call[name]
        med = statistics.median(t)
        c = {"call_ms_median": round(med, 4), "call_ms_min": round(min(t), 4), "call_ms_max": round(max(t), 4),
             "call_ms_rounds": [round(v, 4) for v in t], "kernels_ms": kernels[name],
             "gsamples_out_per_s": round(n / med / 1e6, 2)}
        sy = syns.get(name)
        if sy is not None:
            M, D, Lg = sy.nchan, sy.interp, len(sy.taps)
            nbytes = 8 + 8 * M / D
            ops = 4 * Lg / D + 5 * M * math.log2(M) / D
            t_bytes, t_valu = nbytes * n / HBM * 1e3, ops * n / VALU * 1e3
            floor = max(t_bytes, t_valu)
            kms = sum(kernels[name].values())
            c.update({"M": M, "D": D, "L": Lg, "tile_cols": sy.tile, "bytes_per_sample": nbytes,
                      "lane_ops_per_sample": round(ops, 2), "floor_ms_bytes": round(t_bytes, 4),
                      "floor_ms_valu": round(t_valu, 4), "binds": "bytes" if t_bytes >= t_valu else "valu",
                      "share_of_floor_kernel": round(floor / kms, 4) if kms else None,
                      "share_of_floor_call": round(floor / med, 4)})
        res["configs"][name] = c
    a, d = res["configs"]["a_synth_16_8"], res["configs"]["d_16x_stuff_fir_mix_up_sum"]
    spread = max(a["call_ms_max"] - a["call_ms_min"], d["call_ms_max"] - d["call_ms_min"])
    res["spread_ms"] = round(spread, 4)
    res["a_not_slower_than_d"] = bool(a["call_ms_median"] <= d["call_ms_median"] + spread)
    res["speedup_a_over_d"] = round(d["call_ms_median"] / a["call_ms_median"], 2)
    res["a_agrees_with_d"] = bool(diff <= 1e-4)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not res["a_not_slower_than_d"]:
        sys.exit("synthesizer_bench: the Synthesizer is slower than 16 zero-stuff / FIR / mix_up passes")
    if not res["a_agrees_with_d"]:
        sys.exit("synthesizer_bench: the Synthesizer's output differs from the FIR / mix_up path")


if __name__ == "__main__":
    main()
