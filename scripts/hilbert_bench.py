"""Hilbert kernel timing on the GPU at 64 Mi input samples, device tensors, four
configurations alternated in one process:
  a  SSBDemod("usb")                                   k_hilbert_c2r, M = 25
  b  AmpModem(0.5, "usb", carrier=False), same input   k_ssb_c2r (the baseline a must not lose to)
  c  HilbertTransform(5).r2c                           k_hilbert_r2c
  d  HilbertTransform(5).decim                         k_hilbert_decim
Per configuration: HILBENCH_ROUNDS rounds of HILBENCH_CALLS calls between two
device events (per-call time of each round; their median and spread), then the
per-kernel times of a separate pass under the library's profile hooks.  The
floor of a configuration is the larger of its algorithmic bytes over 8 TB/s and
4M unfused float32 lane operations per sum over the float32 VALU rate (256 CUs
x 4 SIMDs x 32 lanes per clock at 2.4 GHz).  Fails without a GPU.  Prints one
JSON line (and writes it to the file named by --out).  LDSP_PKG_DIR selects the
package build."""
import json
import os
import statistics
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("LDSP_PKG_DIR") or os.path.join(REPO, "python-liquiddsp_amd")
sys.path[:0] = [REPO, PKG]
import torch  # noqa: E402
import liquiddsp as L  # noqa: E402

HBM = 8.0e12                       # bytes / s
VALU = 256 * 4 * 32 * 2.4e9        # float32 lane operations / s (v_mul_f32 / v_add_f32, not packed)


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("hilbert_bench: needs a GPU")
    n = int(os.environ.get("HILBENCH_N", 64 << 20))
    rounds = int(os.environ.get("HILBENCH_ROUNDS", 6))
    calls = int(os.environ.get("HILBENCH_CALLS", 4))
    assert rounds * calls >= 20 and n % 2 == 0
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    xc = torch.complex(torch.randn(n, generator=g, device="cuda"), torch.randn(n, generator=g, device="cuda"))
    xr = torch.randn(n, generator=g, device="cuda")
    ssb, amp = L.SSBDemod("usb"), L.AmpModem(modulation=0.5, type="usb", carrier=False)
    h = L.HilbertTransform(5)
    # name: (call, bytes per input sample, sums per input sample, M)
    cfg = {"a_ssbdemod_usb": (lambda: ssb(xc), 12, 1.0, 25),
           "b_ampmodem_usb": (lambda: amp(xc), 12, 1.0, 25),
           "c_r2c_m5": (lambda: h.r2c(xr), 12, 1.0, 5),
           "d_decim_m5": (lambda: h.decim(xr), 8, 0.5, 5)}
    for fn, *_ in cfg.values():    # warm-up: code objects, history buffers, torch's allocator
        fn()
        fn()
    torch.cuda.synchronize()
    same = bool(torch.equal(ssb(xc[:1 << 20]).view(torch.int32), amp(xc[:1 << 20]).view(torch.int32)))
    per_call = {k: [] for k in cfg}
    for _ in range(rounds):
        for name, (fn, *_) in cfg.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                fn()
            e1.record()
            e1.synchronize()
            per_call[name].append(e0.elapsed_time(e1) / calls)
    kernels = {}
    for name, (fn, *_) in cfg.items():
        L._profile_reset()
        L._profile_enable(True)
        for _ in range(calls):
            fn()
        torch.cuda.synchronize()
        L._profile_enable(False)
        kernels[name] = {k: round(tot / c, 4) for k, (c, tot) in L._profile_report().items()}
    res = {"n": n, "rounds": rounds, "calls_per_round": calls, "pkg": os.path.relpath(PKG, REPO),
           "a_equals_b_bitwise_1Mi": same, "configs": {}}
    for name, (_, nbytes, sums, M) in cfg.items():
        t = per_call[name]
        med = statistics.median(t)
        t_bytes, t_valu = nbytes * n / HBM * 1e3, 4 * M * sums * n / VALU * 1e3
        floor = max(t_bytes, t_valu)
        kms = sum(kernels[name].values())
        res["configs"][name] = {"call_ms_median": round(med, 4), "call_ms_min": round(min(t), 4),
                                "call_ms_max": round(max(t), 4), "call_ms_rounds": [round(v, 4) for v in t],
                                "kernels_ms": kernels[name], "floor_ms_bytes": round(t_bytes, 4),
                                "floor_ms_valu": round(t_valu, 4), "binds": "bytes" if t_bytes >= t_valu else "valu",
                                "share_of_floor_kernel": round(floor / kms, 4),
                                "share_of_floor_call": round(floor / med, 4)}
    a, b = res["configs"]["a_ssbdemod_usb"], res["configs"]["b_ampmodem_usb"]
    spread = max(a["call_ms_max"] - a["call_ms_min"], b["call_ms_max"] - b["call_ms_min"])
    res["spread_ms"] = round(spread, 4)
    res["a_not_slower_than_b"] = bool(a["call_ms_median"] <= b["call_ms_median"] + spread)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not res["a_not_slower_than_b"]:
        sys.exit("hilbert_bench: SSBDemod is slower than the AmpModem baseline")


if __name__ == "__main__":
    main()
