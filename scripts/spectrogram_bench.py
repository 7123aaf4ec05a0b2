"""Spectrogram timing on the GPU at 64 Mi samples, device tensors, four
configurations alternated in one process with the torch formulation of each:
  a  Spectrogram(1024).write(x)                                  accumulate only
  b  Spectrogram(1024, delay=256, window="blackmanharris")(x)    rows, 75 % overlap
  c  Spectrogram(4096, average=64)(x)                            rows of 64 transforms
  d  Spectrogram(256)(x)                                         rows, the smallest size
The torch formulation of a configuration is
  xz.unfold(0, W, d) * w -> torch.fft.fft(n=N) -> abs() ** 2 -> mean
over xz = W - d zeros ++ x (the windows of the definition, the ones reaching
before the stream included): the mean over `average` windows for rows, over all
windows for a.  It runs in one go unless SPGBENCH_SLICES cuts it into that many
slices of whole rows (then the JSON says so).
Per configuration: SPGBENCH_ROUNDS rounds of SPGBENCH_CALLS calls between two
device events (per-call time of each round; their median and spread), then the
per-kernel times of a separate pass under the library's profile hooks.  The
floor is the larger of the algorithmic bytes (8 B in + 4 N / (d A) B out per
sample, no output for write) over 8 TB/s and the flops ((5 N log2 N + 8 N) / d
per sample) over the float32 VALU rate of scripts/hilbert_bench.py (256 CUs x
4 SIMDs x 32 lanes per clock at 2.4 GHz).  Before the timing the first 4 Mi
samples go through both ways (fresh objects) and the rows / the mean are
compared.  Fails without a GPU and when they differ by more than 2e-6 of the
largest bin.  Prints one JSON line (and writes it to the file named by --out).
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
VALU = 256 * 4 * 32 * 2.4e9        # float32 lane operations / s (v_mul_f32 / v_add_f32, not packed)

CONFIGS = {
    "a_1024_write": (dict(nfft=1024), False),
    "b_1024_d256_bh": (dict(nfft=1024, delay=256, window="blackmanharris"), True),
    "c_4096_avg64": (dict(nfft=4096, average=64), True),
    "d_256": (dict(nfft=256), True),
}


class TorchForm:
    """The same rows (or, for write, the same mean) from torch operators."""

    def __init__(self, sp, rows, slices):
        self.N, self.W, self.d, self.A, self.rows, self.slices = sp.nfft, sp.window_len, sp.delay, sp.average, rows, slices
        self.w = torch.from_numpy(sp.window).to("cuda")

    def prepare(self, x):
        return torch.cat([torch.zeros(self.W - self.d, dtype=x.dtype, device=x.device), x])

    def __call__(self, xz):
        fr = xz.unfold(0, self.W, self.d)
        S = fr.shape[0]
        A = self.A if self.rows else S
        K = S // A
        step = -(-K // self.slices)
        out = []
        for k0 in range(0, K, step):
            k1 = min(K, k0 + step)
            p = torch.fft.fft(fr[k0 * A:k1 * A] * self.w, n=self.N).abs() ** 2
            out.append(p.reshape(k1 - k0, A, self.N).mean(dim=1))
        return torch.cat(out) if len(out) > 1 else out[0]


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("spectrogram_bench: needs a GPU")
    n = int(os.environ.get("SPGBENCH_N", 64 << 20))
    rounds = int(os.environ.get("SPGBENCH_ROUNDS", 6))
    calls = int(os.environ.get("SPGBENCH_CALLS", 4))
    slices = int(os.environ.get("SPGBENCH_SLICES", 1))
    assert rounds >= 3 and n % (4096 * 64) == 0
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    x = torch.complex(torch.randn(n, generator=g, device="cuda"), torch.randn(n, generator=g, device="cuda"))

    # both ways over the first 4 Mi samples, fresh objects
    nchk = min(n, 4 << 20)
    agree = {}
    for name, (kw, rows) in CONFIGS.items():
        sp = L.Spectrogram(**kw)
        tf = TorchForm(sp, rows, 1)
        ref = tf(tf.prepare(x[:nchk])).double()
        if rows:
            got = sp(x[:nchk]).double()
        else:
            sp.write(x[:nchk])
            got = torch.from_numpy(sp.psd).to("cuda")[None, :]
        assert got.shape == ref.shape, (name, got.shape, ref.shape)
        agree[name] = float(((got - ref).abs().amax(dim=1) / ref.amax(dim=1)).max())
        del ref, got

    objs, cfg = {}, {}
    for name, (kw, rows) in CONFIGS.items():
        sp = L.Spectrogram(**kw)
        tf = TorchForm(sp, rows, slices)
        xz = tf.prepare(x)
        objs[name] = (sp, rows)
        cfg[name] = (lambda sp=sp: sp(x)) if rows else (lambda sp=sp: sp.write(x))
        cfg[name + "_torch"] = lambda tf=tf, xz=xz: tf(xz)
    for fn in cfg.values():        # warm-up: code objects, state buffers, torch's allocator and FFT plans
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
    for name in objs:
        L._profile_reset()
        L._profile_enable(True)
        for _ in range(calls):
            cfg[name]()
        torch.cuda.synchronize()
        L._profile_enable(False)
        kernels[name] = {k: round(tot / c, 4) for k, (c, tot) in L._profile_report().items()}

    res = {"n": n, "rounds": rounds, "calls_per_round": calls, "pkg": os.path.relpath(PKG, REPO),
           "torch_slices": slices, "max_diff_over_max_4Mi": agree, "configs": {}}
    for name in cfg:
        t = per_call[name]
        med = statistics.median(t)
        res["configs"][name] = {"call_ms_median": round(med, 4), "call_ms_min": round(min(t), 4),
                                "call_ms_max": round(max(t), 4), "call_ms_rounds": [round(v, 4) for v in t],
                                "gsamples_per_s": round(n / med / 1e6, 2)}
    for name, (sp, rows) in objs.items():
        c = res["configs"][name]
        N, W, d, A = sp.nfft, sp.window_len, sp.delay, sp.average
        nbytes = 8 + (4 * N / (d * A) if rows else 0)
        flops = (5 * N * math.log2(N) + 8 * N) / d
        t_bytes, t_valu = nbytes * n / HBM * 1e3, flops * n / VALU * 1e3
        floor = max(t_bytes, t_valu)
        kms = sum(kernels[name].values())
        tmed = res["configs"][name + "_torch"]["call_ms_median"]
        c.update({"nfft": N, "window_len": W, "delay": d, "average": A, "rows": rows, "kernels_ms": kernels[name],
                  "bytes_per_sample": round(nbytes, 3), "flops_per_sample": round(flops, 2),
                  "floor_ms_bytes": round(t_bytes, 4), "floor_ms_valu": round(t_valu, 4),
                  "binds": "bytes" if t_bytes >= t_valu else "valu",
                  "share_of_floor_kernel": round(floor / kms, 4) if kms else None,
                  "share_of_floor_call": round(floor / c["call_ms_median"], 4),
                  "torch_over_spectrogram": round(tmed / c["call_ms_median"], 2)})
    res["agrees"] = bool(max(agree.values()) <= 2e-6)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not res["agrees"]:
        sys.exit("spectrogram_bench: the rows differ from the torch formulation")


if __name__ == "__main__":
    main()
