"""AudioBank call time over the window length, the de-emphasis warm-up and the
rate, to see what the kernel's time is made of ("AudioBank
kernel").  Device tensors float32[16, 512 Ki] and [256, 64 Ki]; per
configuration the median of 5 rounds of 200 calls between two device events, in
microseconds per call.  The rates of the last block come in pairs, 1 / s with s
a multiple of 4 words and a rate 2 % off it: at 8, 16 and 32 words the first of
a pair runs the kernel's skewed span layout and the second the linear one on
nearly the same bank pattern.  Prints one line per configuration
(profiles/audiobank_sweep.txt keeps a run).  Needs a GPU; sets no threshold.
LDSP_PKG_DIR selects the package build."""
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("LDSP_PKG_DIR") or os.path.join(REPO, "python-liquiddsp_amd")
sys.path[:0] = [REPO, PKG]
import torch  # noqa: E402
import liquiddsp as L  # noqa: E402

RATE = 0.192
WINDOWS = (dict(len=1, nfilter=16), dict(len=4), dict(len=10), dict(len=20), dict(len=32), dict(len=20, nfilter=64))
DEEMPH = tuple(dict(len=20, deemphasis=sr) for sr in (48e3, 125e3, 250e3, 426e3)) + (
    dict(len=1, nfilter=16, deemphasis=250e3), dict(len=20, deemphasis=250e3, pcm16=True))
STRIDES = (32, 31.4, 16, 15.7, 8, 7.85, 4, 3.9)


def per_call_us(fn, x, calls=200, rounds=5):
    for _ in range(5):
        fn(x)
    t = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            fn(x)
        e1.record()
        e1.synchronize()
        t.append(e0.elapsed_time(e1) / calls * 1e3)
    return sorted(t)[rounds // 2]


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("audiobank_sweep: needs a GPU")
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    xs = {C: torch.randn((C, n), generator=g, device="cuda") for C, n in ((16, 512 << 10), (256, 64 << 10))}
    for C, x in xs.items():
        for kw in WINDOWS + DEEMPH:
            ab = L.AudioBank(C, RATE, **kw)
            print(f"C={C} rate={RATE} {kw} tile={ab.tile} us={per_call_us(ab, x):.1f}", flush=True)
    for s in STRIDES:
        for kw in (dict(len=20), dict(len=20, deemphasis=250e3)):
            ab = L.AudioBank(16, 1 / s, nfilter=16, **kw)
            print(f"C=16 rate=1/{s:g} {kw} tile={ab.tile} us={per_call_us(ab, xs[16]):.1f}", flush=True)


if __name__ == "__main__":
    main()
