"""AMBank timing on the GPU, device tensors, 64 Mi input samples in two shapes and
the AM receiver end to end, alternated in one process:
  a  AMBank(16, 4, audio=0.125, carrier=0.004)  on complex64[16, 4 Mi]     k_ambank, 1001 taps
  b  torch's device work for the same definition on a's input: the real and
     imaginary parts as [16, 2, 4 Mi], one strided grouped conv1d with the taps
     (d, g) per part, the elementwise combine
  c  AMBank(256, 4, audio=0.125, carrier=0.004) on complex64[256, 256 Ki]
  d  the same torch work on c's input
  r  the AM receiver on 64 Mi wideband samples, three calls:
     Channelizer(16, 8) -> AMBank(16, 4) -> AudioBank(16, 0.768, deemphasis=None)
  q  the squelched receiver, four calls:
     Channelizer(16, 8) -> SquelchBank(16, 1024) -> AMBank(16, 4) -> AudioBank(16, 0.768, deemphasis=None)
b and d run code the AMBank does not touch: they are the yardstick.  Per
configuration: AMBENCH_ROUNDS rounds of AMBENCH_CALLS calls between two device
events (per-call time of each round; their median and spread), then the
per-kernel times of a separate pass under the library's profile hooks.  The
floors of an AMBank configuration are its algorithmic bytes (8 B in + 4 / D B
out per input sample) over 8 TB/s and its multiply-adds (4 L / D per input
sample) over the float32 VALU rate (256 CUs x 4 SIMDs x 32 lanes per clock at
2.4 GHz).  Before the timing, a and b over the first 256 Ki samples of row 5 are
compared (fresh objects).  Fails without a GPU and when the rows differ by more
than 1e-5 (absolute, 1 being 100 % modulation); it sets no speed threshold.
Prints one JSON line (and writes it to the file named by --out).  LDSP_PKG_DIR
selects the package build."""
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
D, AUDIO, CARRIER = 4, 0.125, 0.004


class Baseline:
    """The definition with torch: one strided grouped conv1d over (re, im), combine."""

    def __init__(self, am, n):
        d, g = am.band_taps, am.carrier_taps
        self.D, self.L, self.ncols = am.decim, d.size, -(-n // am.decim)
        self.thr2 = float(np.float32(am.threshold) ** 2)
        k = np.stack([d, g, d, g])[:, None, ::-1].copy()                                  # conv1d correlates
        self.k = torch.from_numpy(k.astype(np.float32)).cuda()                            # [4][1][L]

    def __call__(self, x):
        v = torch.view_as_real(x).permute(0, 2, 1)                                        # [C][2][n]
        f = torch.nn.functional.conv1d(v, self.k, stride=self.D, padding=self.L - 1, groups=2)[:, :, :self.ncols]
        br, cr, bi, ci = f.unbind(1)
        m = cr * cr + ci * ci
        return torch.where(m > self.thr2, (br * cr + bi * ci) / m, torch.zeros_like(m))


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("ambank_bench: needs a GPU")
    shapes = {"16": (16, int(os.environ.get("AMBENCH_N16", 4 << 20))),
              "256": (256, int(os.environ.get("AMBENCH_N256", 256 << 10)))}
    nwide = int(os.environ.get("AMBENCH_NWIDE", 64 << 20))
    rounds = int(os.environ.get("AMBENCH_ROUNDS", 12))
    calls = int(os.environ.get("AMBENCH_CALLS", 3))
    assert rounds >= 3 and nwide % 4096 == 0
    gen = torch.Generator(device="cuda")
    gen.manual_seed(1)

    def cnoise(shape, dev):
        return dev * torch.complex(torch.randn(shape, generator=gen, device="cuda"), torch.randn(shape, generator=gen, device="cuda"))

    # AM-like rows: a carrier of amplitude 0.5, 0.001 cycles per sample off, under noise of deviation 0.14
    xs = {}
    for k, (C, n) in shapes.items():
        t = torch.arange(n, device="cuda", dtype=torch.float64)
        car = torch.polar(torch.full((n,), 0.5, device="cuda", dtype=torch.float64), 2 * np.pi * 0.001 * t).to(torch.complex64)
        xs[k] = cnoise((C, n), 0.1) + car[None, :]
        del t, car

    # row 5 both ways, fresh objects
    C, n = shapes["16"]
    nchk = min(n, 256 << 10)
    kw = dict(audio=AUDIO, carrier=CARRIER)
    chk = L.AMBank(C, D, **kw)
    xc = xs["16"][:6, :nchk].contiguous()
    ya = L.AMBank(6, D, **kw)(xc)[5].cpu().numpy().astype(np.float64)
    yb = Baseline(chk, nchk)(xc)[5].cpu().numpy().astype(np.float64)
    n0 = -(-chk.ntaps // D) + 1                       # past the first columns, whose window holds the zeros before the stream
    row5 = float(np.max(np.abs(ya[n0:] - yb[n0:])))
    row5_max = float(np.max(np.abs(yb[n0:])))
    del ya, yb, xc, chk

    banks, cfg = {}, {}
    for (key, (C, n)), (nb, nt) in zip(shapes.items(), (("a", "b"), ("c", "d"))):
        x = xs[key]
        bank = L.AMBank(C, D, **kw)
        base = Baseline(bank, n)
        banks[f"{nb}_ambank_{C}"] = bank
        cfg[f"{nb}_ambank_{C}"] = (lambda fn=bank, x=x: fn(x))
        cfg[f"{nt}_torch_{C}"] = (lambda fn=base, x=x: fn(x))
    # 16 carriers at the channel centres under wideband noise
    tw = torch.arange(nwide, device="cuda", dtype=torch.int64)
    wide = cnoise(nwide, 0.05)
    for c in range(16):
        wide += torch.polar(torch.full((16,), 0.05, device="cuda"), 2 * np.pi * c * torch.arange(16, device="cuda") / 16.0)[tw % 16]
    del tw
    ch_r, am_r, au_r = L.Channelizer(16, 8), L.AMBank(16, D, **kw), L.AudioBank(16, 0.768, deemphasis=None)
    ch_q, sq_q, am_q = L.Channelizer(16, 8), L.SquelchBank(16, 1024, -40.0), L.AMBank(16, D, **kw)
    au_q = L.AudioBank(16, 0.768, deemphasis=None)
    cfg["r_am_receiver_3_calls"] = lambda: au_r(am_r(ch_r(wide)))
    cfg["q_squelched_am_receiver_4_calls"] = lambda: au_q(am_q(sq_q(ch_q(wide))))
    for fn in cfg.values():        # warm-up: code objects, history buffers, torch's allocator and conv1d's search
        fn()
        fn()
    torch.cuda.synchronize()
    st = sq_q.status
    st = st.cpu().numpy() if hasattr(st, "cpu") else np.asarray(st)
    open_share = float(np.isin(st, (2, 3, 4, 5)).mean())   # RISE, SIGNALHI, FALL, SIGNALLO: the blocks the gate passes
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
           "row5_max_abs_diff_256Ki": row5, "row5_max_abs": row5_max, "squelch_open_blocks_share": round(open_share, 4),
           "configs": {}}
    for name in cfg:
        t = per_call[name]
        med = statistics.median(t)
        c = {"call_ms_median": round(med, 4), "call_ms_min": round(min(t), 4), "call_ms_max": round(max(t), 4),
             "call_ms_rounds": [round(v, 4) for v in t], "kernels_ms": kernels[name]}
        am = banks.get(name)
        if am is not None:
            total = am.nchan * shapes[str(am.nchan)][1]
            Lh = am.ntaps
            nbytes, fma = 8 + 4 / D, 4 * Lh / D
            t_bytes, t_valu = nbytes * total / HBM * 1e3, fma * total / VALU * 1e3
            kms = sum(kernels[name].values())
            c.update({"C": am.nchan, "D": D, "L": Lh, "tile": am.tile, "gsamples_per_s": round(total / med / 1e6, 2),
                      "bytes_per_sample": nbytes, "fma_per_sample": fma, "floor_ms_bytes": round(t_bytes, 4),
                      "floor_ms_valu": round(t_valu, 4), "binds": "bytes" if t_bytes >= t_valu else "valu",
                      "kernel_share_of_bytes_floor": round(t_bytes / kms, 4) if kms else None,
                      "kernel_share_of_valu_floor": round(t_valu / kms, 4) if kms else None})
        res["configs"][name] = c
    cf = res["configs"]
    for new, old in (("a_ambank_16", "b_torch_16"), ("c_ambank_256", "d_torch_256")):
        res[f"speedup_{new[0]}_over_{old[0]}"] = round(cf[old]["call_ms_median"] / cf[new]["call_ms_median"], 2)
    res["row5_agrees"] = bool(row5 <= 1e-5)
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not res["row5_agrees"]:
        sys.exit("ambank_bench: row 5 differs from the torch evaluation of the definition")


if __name__ == "__main__":
    main()
