"""StereoBank timing on the GPU, device tensors, 64 Mi input samples in two shapes
and the receivers end to end, alternated in one process:
  a  StereoBank(16, 0.076, 5)  on float32[16, 4 Mi]             k_stbank, 225 taps
  b  torch's device work for the same definition on a's input: the five
     pre-mixed real signals (u and u times cos / -sin of the two phases, the
     phase tables computed once outside the timing) stacked as [16, 5, 4 Mi],
     one strided grouped conv1d with the taps (h, h, h, g, g), the elementwise
     combine
  c  StereoBank(128, 0.076, 5) on float32[128, 512 Ki]
  d  the same torch work on c's input
  s  the stereo receiver on 64 Mi wideband samples, four calls:
     Channelizer(16, 8) -> FMBank(16, kf, 1) -> StereoBank(16, 0.076, 5)
     -> AudioBank(32, 0.96, deemphasis=50e3) on the [32, ncols] view
  m  the mono receiver of the README on the same capture, three calls:
     Channelizer(16, 8) -> FMBank(16, kf, 8) -> AudioBank(16, 0.192, deemphasis=250e3)
  n  a mono receiver at s's rates: Channelizer(16, 8) -> FMBank(16, kf, 5)
     -> AudioBank(16, 0.96, deemphasis=50e3)
b and d run code the StereoBank does not touch: they are the yardstick.  Per
configuration: STBENCH_ROUNDS rounds of STBENCH_CALLS calls between two device
events (per-call time of each round; their median and spread), then the
per-kernel times of a separate pass under the library's profile hooks.  The
floors of a StereoBank configuration are its algorithmic bytes (4 B in + 8 / D B
out per input sample) over 8 TB/s and its multiply-adds (5 L / D per input
sample) over the float32 VALU rate (256 CUs x 4 SIMDs x 32 lanes per clock at
2.4 GHz).  Before the timing, a and b over the first 256 Ki samples of row 5 are
compared (fresh objects).  Fails without a GPU and when the rows differ by more
than 1e-4 of the row's maximum (b mixes in float32); it sets no speed
threshold.  Prints one JSON line (and writes it to the file named by --out).
LDSP_PKG_DIR selects the package build."""
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
PILOT, D, KF = 0.076, 5, 0.15


class Baseline:
    """The definition with torch: pre-mix, one strided grouped conv1d, combine."""

    def __init__(self, sb, n):
        h, g, w = sb.taps.astype(np.float64), sb.pilot_taps.astype(np.float64), sb.word
        self.D, self.L, self.ncols = sb.decim, h.size, -(-n // sb.decim)
        self.thr2 = float(np.float32(sb.threshold) ** 2)
        t = np.arange(n, dtype=np.int64)
        a1 = 2 * np.pi * (np.mod(t * w, 2 ** 32) / 2.0 ** 32)
        a2 = 2 * np.pi * (np.mod(t * 2 * w, 2 ** 32) / 2.0 ** 32)
        tab = np.stack([np.ones(n), np.cos(a2), -np.sin(a2), np.cos(a1), -np.sin(a1)])
        self.mix = torch.from_numpy(tab.astype(np.float32)).cuda()                        # [5][n]
        k = np.stack([h, h, h, g, g])[:, None, ::-1].copy()                               # conv1d correlates
        self.k = torch.from_numpy(k.astype(np.float32)).cuda()                            # [5][1][L]

    def __call__(self, x):
        v = x[:, None, :] * self.mix[None, :, :]
        f = torch.nn.functional.conv1d(v, self.k, stride=self.D, padding=self.L - 1, groups=5)[:, :, :self.ncols]
        s, zr, zi, pr, pi = f.unbind(1)
        m = pr * pr + pi * pi
        im = zi * (pr * pr - pi * pi) - zr * (2 * pr * pi)
        S = torch.where(m > self.thr2, 2 * im / m, torch.zeros_like(m))
        return torch.stack([s + S, s - S], dim=1)


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("stereobank_bench: needs a GPU")
    shapes = {"16": (16, int(os.environ.get("STBENCH_N16", 4 << 20))),
              "128": (128, int(os.environ.get("STBENCH_N128", 512 << 10)))}
    nwide = int(os.environ.get("STBENCH_NWIDE", 64 << 20))
    rounds = int(os.environ.get("STBENCH_ROUNDS", 12))
    calls = int(os.environ.get("STBENCH_CALLS", 3))
    assert rounds >= 3 and nwide % 4096 == 0
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    # multiplex-like rows: noise of deviation 0.2 and a pilot of amplitude 0.1, so the stereo branch is taken
    xs = {}
    for k, (C, n) in shapes.items():
        t = torch.arange(n, device="cuda", dtype=torch.float64)
        pil = (0.1 * torch.sin(2 * np.pi * PILOT * t)).float()
        xs[k] = 0.2 * torch.randn((C, n), generator=g, device="cuda") + pil[None, :]
        del t, pil

    # row 5 both ways, fresh objects
    C, n = shapes["16"]
    nchk = min(n, 256 << 10)
    chk = L.StereoBank(C, PILOT, D)
    xc = xs["16"][:6, :nchk].contiguous()
    ya = L.StereoBank(6, PILOT, D)(xc)[5].cpu().numpy().astype(np.float64)
    yb = Baseline(chk, nchk)(xc)[5].cpu().numpy().astype(np.float64)
    row5 = float(np.max(np.abs(ya - yb)) / np.max(np.abs(yb)))
    stereo_share = float(np.mean(ya[0] != ya[1]))
    del ya, yb, xc, chk

    banks, cfg = {}, {}
    for (key, (C, n)), (nb, nt) in zip(shapes.items(), (("a", "b"), ("c", "d"))):
        x = xs[key]
        bank = L.StereoBank(C, PILOT, D)
        base = Baseline(bank, n)
        banks[f"{nb}_stbank_{C}"] = bank
        cfg[f"{nb}_stbank_{C}"] = (lambda fn=bank, x=x: fn(x))
        cfg[f"{nt}_torch_{C}"] = (lambda fn=base, x=x: fn(x))
    wide = torch.complex(torch.randn(nwide, generator=g, device="cuda"), torch.randn(nwide, generator=g, device="cuda"))
    ch_s, fm_s, st_s = L.Channelizer(16, 8), L.FMBank(16, KF, 1), L.StereoBank(16, PILOT, D)
    au_s = L.AudioBank(32, 0.96, deemphasis=50e3)
    ch_m, fm_m, au_m = L.Channelizer(16, 8), L.FMBank(16, KF, 8), L.AudioBank(16, 0.192, deemphasis=250e3)
    ch_n, fm_n, au_n = L.Channelizer(16, 8), L.FMBank(16, KF, D), L.AudioBank(16, 0.96, deemphasis=50e3)

    def stereo_rx():
        y = st_s(fm_s(ch_s(wide)))
        return au_s(y.reshape(32, y.shape[2]))

    cfg["s_stereo_receiver_4_calls"] = stereo_rx
    cfg["m_mono_receiver_readme"] = lambda: au_m(fm_m(ch_m(wide)))
    cfg["n_mono_receiver_same_rates"] = lambda: au_n(fm_n(ch_n(wide)))
    for fn in cfg.values():        # warm-up: code objects, history buffers, torch's allocator and conv1d's search
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

    res = {"shapes": {k: {"C": v[0], "n_per_row": v[1], "D": D} for k, v in shapes.items()}, "wideband_samples": nwide,
           "rounds": rounds, "calls_per_round": calls, "pkg": os.path.relpath(PKG, REPO),
           "row5_max_diff_over_max_256Ki": row5, "row5_stereo_columns_share": round(stereo_share, 4), "configs": {}}
    for name in cfg:
        t = per_call[name]
        med = statistics.median(t)
        c = {"call_ms_median": round(med, 4), "call_ms_min": round(min(t), 4), "call_ms_max": round(max(t), 4),
             "call_ms_rounds": [round(v, 4) for v in t], "kernels_ms": kernels[name]}
        sb = banks.get(name)
        if sb is not None:
            total = sb.nchan * shapes[str(sb.nchan)][1]
            Lh = len(sb.taps)
            nbytes, fma = 4 + 8 / D, 5 * Lh / D
            t_bytes, t_valu = nbytes * total / HBM * 1e3, fma * total / VALU * 1e3
            kms = sum(kernels[name].values())
            c.update({"C": sb.nchan, "D": D, "L": Lh, "tile": sb.tile, "gsamples_per_s": round(total / med / 1e6, 2),
                      "bytes_per_sample": nbytes, "fma_per_sample": fma, "floor_ms_bytes": round(t_bytes, 4),
                      "floor_ms_valu": round(t_valu, 4), "binds": "bytes" if t_bytes >= t_valu else "valu",
                      "kernel_share_of_bytes_floor": round(t_bytes / kms, 4) if kms else None,
                      "kernel_share_of_valu_floor": round(t_valu / kms, 4) if kms else None})
        res["configs"][name] = c
    cf = res["configs"]
    for new, old in (("a_stbank_16", "b_torch_16"), ("c_stbank_128", "d_torch_128")):
        res[f"speedup_{new[0]}_over_{old[0]}"] = round(cf[old]["call_ms_median"] / cf[new]["call_ms_median"], 2)
    res["row5_agrees"] = bool(row5 <= 1e-4)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not res["row5_agrees"]:
        sys.exit("stereobank_bench: row 5 differs from the torch evaluation of the definition")


if __name__ == "__main__":
    main()
