"""SSBBank timing on the GPU, device tensors, 64 Mi input samples in two shapes
(16 rows of 4 Mi, 256 rows of 256 Ki) and two designs, random per-row BFOs and
sidebands, and the HF receiver end to end, alternated in one process:
  s81_C    SSBBank(C, 2, lo=0.025, hi=0.225)            k_ssbbank, 81 taps: the byte floor and the
                                                        multiply-add floor are close
  t81_C    torch's device work for the same definition on the same input: the
           per-row mix (a complex multiply by a rotator table made once, outside
           the timing), one strided grouped conv1d with the real and the
           imaginary band-pass taps over (re, im), the combine re - s im
  s1001_C  SSBBank(C, 4, lo=0.004, hi=0.121, ntaps=1001)  k_ambank's bench length
  t1001_C  the same torch work
  am_C     AMBank(C, 4, ntaps=1001) on s1001_C's input: the same multiply-adds per offset
  r        the HF receiver on 64 Mi wideband samples, three calls:
           Channelizer(256, 128) -> SSBBank(256, 2) -> AudioBank(256, 0.96, deemphasis=None)
The torch configurations run code the SSBBank does not touch: they are the
yardstick.  Per configuration: SSBBENCH_ROUNDS rounds of SSBBENCH_CALLS calls
between two device events (per-call time of each round; their median and
spread), then the per-kernel times of a separate pass under the library's
profile hooks.  The floors of an SSBBank configuration are its algorithmic bytes
(8 B in + 4 / D B out per input sample) over 8 TB/s and its multiply-adds
(4 L / D per input sample) over the float32 VALU rate (256 CUs x 4 SIMDs x 32
lanes per clock at 2.4 GHz).  Before the timing, the kernel and the torch work
over the first 256 Ki samples of six rows are compared (fresh objects, both
designs).  Fails without a GPU and when the rows differ by more than 1e-5 of
the largest output; it sets no speed threshold.  Prints one JSON line (and
writes it to the file named by --out).  LDSP_PKG_DIR selects the package build;
SSBBENCH_ONLY=kernel leaves out the torch work, the AMBank and the receiver."""
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
DESIGNS = {"81": dict(decim=2, lo=0.025, hi=0.225, ntaps=81), "1001": dict(decim=4, lo=0.004, hi=0.121, ntaps=1001)}


class Baseline:
    """The definition with torch: mix every row to its carrier, one strided grouped conv1d of (re, im) with the
    real and the imaginary taps of the upper-sideband band-pass, y = re - s im."""

    def __init__(self, sb, n):
        p, w = sb.taps.astype(np.float64), sb.words
        self.D, self.L, self.ncols = sb.decim, p.size, -(-n // sb.decim)
        fm = np.rint((sb.lo + sb.hi) / 2 * 4294967296.0) / 4294967296.0
        q = p * np.exp(2j * np.pi * fm * (np.arange(p.size) - (p.size - 1) / 2))          # the usb band-pass
        k = np.stack([q.real, q.imag])[:, None, ::-1].copy()                              # conv1d correlates
        self.k = torch.from_numpy(k.astype(np.float32)).cuda()                            # [2][1][L]
        self.s = torch.tensor([1.0 if s == "usb" else -1.0 for s in sb.sideband], device="cuda")[:, None]
        t = torch.arange(n, device="cuda", dtype=torch.int64)[None, :]
        ph = (t * torch.from_numpy(w.astype(np.int64)).cuda()[:, None]) & 0xFFFFFFFF      # exact: t w < 2^63
        a = ph.to(torch.float64) * (-2 * np.pi / 4294967296.0)
        self.rot = torch.polar(torch.ones_like(a), a).to(torch.complex64)                 # [C][n], made once
        del t, ph, a

    def __call__(self, x):
        v = torch.view_as_real(x * self.rot).permute(0, 2, 1)                             # [C][2][n]
        f = torch.nn.functional.conv1d(v, self.k, stride=self.D, padding=self.L - 1, groups=2)[:, :, :self.ncols]
        return f[:, 0] - self.s * f[:, 1]


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("ssbbank_bench: needs a GPU")
    shapes = {"16": (16, int(os.environ.get("SSBBENCH_N16", 4 << 20))),
              "256": (256, int(os.environ.get("SSBBENCH_N256", 256 << 10)))}
    nwide = int(os.environ.get("SSBBENCH_NWIDE", 64 << 20))
    rounds = int(os.environ.get("SSBBENCH_ROUNDS", 12))
    calls = int(os.environ.get("SSBBENCH_CALLS", 3))
    kernel_only = os.environ.get("SSBBENCH_ONLY") == "kernel"
    assert rounds >= 3 and nwide % 4096 == 0
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)
    rng = np.random.default_rng(2)

    def cnoise(shape, dev):
        return dev * torch.complex(torch.randn(shape, generator=gen, device="cuda"), torch.randn(shape, generator=gen, device="cuda"))

    xs = {k: cnoise((C, n), 0.2) for k, (C, n) in shapes.items()}
    tune = {k: (rng.uniform(-0.5, 0.5, C), [("usb", "lsb")[int(v)] for v in rng.integers(0, 2, C)])
            for k, (C, n) in shapes.items()}

    def bank(key, name, C=None):
        bfo, side = tune[key]
        C = C or shapes[key][0]
        return L.SSBBank(C, bfo=bfo[:C], sideband=side[:C], **DESIGNS[name])

    # six rows both ways, fresh objects, both designs
    agree = {}
    nchk = min(shapes["16"][1], 256 << 10)
    xc = xs["16"][:6, :nchk].contiguous()
    for name in DESIGNS:
        sb = bank("16", name, 6)
        ya = sb(xc).cpu().numpy().astype(np.float64)
        yb = Baseline(bank("16", name, 6), nchk)(xc).cpu().numpy().astype(np.float64)
        agree[name] = float(np.max(np.abs(ya - yb)) / np.max(np.abs(yb)))
    del xc, ya, yb

    banks, cfg = {}, {}
    for key, (C, n) in shapes.items():
        for name in DESIGNS:
            sb = bank(key, name)
            banks[f"s{name}_{C}"] = sb
            cfg[f"s{name}_{C}"] = (lambda fn=sb, x=xs[key]: fn(x))
            if not kernel_only:
                cfg[f"t{name}_{C}"] = (lambda fn=Baseline(sb, n), x=xs[key]: fn(x))
        if not kernel_only:
            cfg[f"am_{C}"] = (lambda fn=L.AMBank(C, 4, ntaps=1001), x=xs[key]: fn(x))
    if not kernel_only:
        wide = cnoise(nwide, 0.05)
        bfo, side = tune["256"]
        ch_r, sb_r = L.Channelizer(256, 128), L.SSBBank(256, bfo=bfo, sideband=side, **DESIGNS["81"])
        au_r = L.AudioBank(256, 0.96, deemphasis=None)
        cfg["r_hf_receiver_3_calls"] = lambda: au_r(sb_r(ch_r(wide)))
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

    res = {"shapes": {k: {"C": v[0], "n_per_row": v[1]} for k, v in shapes.items()}, "designs": DESIGNS,
           "wideband_samples": nwide, "rounds": rounds, "calls_per_round": calls, "pkg": os.path.relpath(PKG, REPO),
           "six_rows_max_diff_of_max_256Ki": agree, "configs": {}}
    for name in cfg:
        t = per_call[name]
        med = statistics.median(t)
        c = {"call_ms_median": round(med, 4), "call_ms_min": round(min(t), 4), "call_ms_max": round(max(t), 4),
             "call_ms_rounds": [round(v, 4) for v in t], "kernels_ms": kernels[name]}
        sb = banks.get(name)
        if sb is not None:
            total = sb.nchan * shapes[str(sb.nchan)][1]
            D, Lh = sb.decim, sb.ntaps
            nbytes, fma = 8 + 4 / D, 4 * Lh / D
            t_bytes, t_valu = nbytes * total / HBM * 1e3, fma * total / VALU * 1e3
            kms = sum(kernels[name].values())
            c.update({"C": sb.nchan, "D": D, "L": Lh, "tile": sb.tile, "gsamples_per_s": round(total / med / 1e6, 2),
                      "bytes_per_sample": nbytes, "fma_per_sample": fma, "floor_ms_bytes": round(t_bytes, 4),
                      "floor_ms_valu": round(t_valu, 4), "binds": "bytes" if t_bytes >= t_valu else "valu",
                      "kernel_share_of_bytes_floor": round(t_bytes / kms, 4) if kms else None,
                      "kernel_share_of_valu_floor": round(t_valu / kms, 4) if kms else None})
        res["configs"][name] = c
    cf = res["configs"]
    if not kernel_only:
        for C in (16, 256):
            for name in DESIGNS:
                res[f"speedup_s{name}_{C}_over_torch"] = round(cf[f"t{name}_{C}"]["call_ms_median"] / cf[f"s{name}_{C}"]["call_ms_median"], 2)
            res[f"s1001_{C}_over_am_{C}"] = round(cf[f"s1001_{C}"]["call_ms_median"] / cf[f"am_{C}"]["call_ms_median"], 4)
    res["rows_agree"] = bool(max(agree.values()) <= 1e-5)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not res["rows_agree"]:
        sys.exit("ssbbank_bench: the rows differ from the torch evaluation of the definition")


if __name__ == "__main__":
    main()
