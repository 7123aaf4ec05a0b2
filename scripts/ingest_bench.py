"""Int16 IQ ingest timing on the GPU at 64 Mi wideband samples: for each object
three ways to process one capture, alternated call by call in one process:
  c64       obj(x)                    the complex64 capture already in memory
  two_call  obj(bytes_to_iq(raw))     the int16 capture converted by k_bytes_to_iq first
  fused     obj.from_bytes(raw)       the int16 capture converted in the kernel's loads
(Spectrogram: write / write_bytes, nothing stored.)  The objects:
  chan_16_8, chan_16_16, chan_256_128   Channelizer(M, D, m=6)
  ddc_16x64, ddc_1x64                   Downconverter(16 / 1 tuners, decim 64, m=6)
  spgram_1024, spgram_256               Spectrogram(N).write (hann, hop N / 2)
with raw a device int16 tensor, and chan_16_8_host: the same three with numpy
arrays in host memory (the upload is 4 n bytes instead of 8 n; timed on the
host's clock, the calls synchronise).
Per variant: INGESTBENCH_WARMUP untimed calls, then INGESTBENCH_REPEATS (>= 10)
timed ones, each between two device events of its own; min, median and max.
Before the timing fresh twins take the whole capture both ways and the outputs
(Spectrogram: the transform count and the float64 psd) must be bit-equal;
`bit_equal` in the result.  `fused_below_two_call` of a row: the fused median
lies below the two-call median by more than the two-call variant's own
max - min in this run.  Fails without a GPU and when an output differs.
Prints one JSON line (and writes it to the file named by --out).  LDSP_PKG_DIR
selects the package build."""
import json
import os
import statistics
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.environ.get("LDSP_PKG_DIR") or os.path.join(REPO, "python-liquiddsp_amd")
sys.path[:0] = [REPO, PKG]
import numpy as np  # noqa: E402
import torch  # noqa: E402
import liquiddsp as L  # noqa: E402

FREQS16 = [(2 * k - 15) / 34.0 for k in range(16)]

OBJECTS = {
    "chan_16_8": lambda: L.Channelizer(16, 8, m=6),
    "chan_16_16": lambda: L.Channelizer(16, 16, m=6),
    "chan_256_128": lambda: L.Channelizer(256, 128, m=6),
    "ddc_16x64": lambda: L.Downconverter(FREQS16, 64, m=6),
    "ddc_1x64": lambda: L.Downconverter([0.1], 64, m=6),
    "spgram_1024": lambda: L.Spectrogram(1024),
    "spgram_256": lambda: L.Spectrogram(256),
}


def variants(obj, x, raw):
    """The three calls of one object on one capture (x complex64, raw int16; both device or both host)."""
    if isinstance(obj, L.Spectrogram):
        return {"c64": lambda: obj.write(x), "two_call": lambda: obj.write(L.bytes_to_iq(raw)),
                "fused": lambda: obj.write_bytes(raw)}
    return {"c64": lambda: obj(x), "two_call": lambda: obj(L.bytes_to_iq(raw)), "fused": lambda: obj.from_bytes(raw)}


def equal_bits(make, raw):
    """Fresh twins, the whole capture both ways."""
    a, b = make(), make()
    if isinstance(a, L.Spectrogram):
        ta, tb = a.write_bytes(raw), b.write(L.bytes_to_iq(raw))
        return bool(ta == tb and np.array_equal(a.psd.view(np.uint64), b.psd.view(np.uint64)))
    ya, yb = a.from_bytes(raw), b(L.bytes_to_iq(raw))
    if isinstance(ya, np.ndarray):
        return bool(ya.shape == yb.shape and np.array_equal(ya.view(np.uint64), yb.view(np.uint64)))
    return bool(ya.shape == yb.shape and torch.equal(ya.view(torch.float32), yb.view(torch.float32)))


def time_device(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def time_host(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    return (time.perf_counter() - t0) * 1e3


def measure(calls, timer, warmup, repeats):
    for _ in range(warmup):
        for fn in calls.values():
            fn()
    torch.cuda.synchronize()
    t = {k: [] for k in calls}
    for _ in range(repeats):
        for k, fn in calls.items():      # alternated, not in blocks
            t[k].append(timer(fn))
    return t


def row(t):
    r = {}
    for k, v in t.items():
        r[k + "_ms"] = round(statistics.median(v), 4)
        r[k + "_ms_min"] = round(min(v), 4)
        r[k + "_ms_max"] = round(max(v), 4)
    spread = r["two_call_ms_max"] - r["two_call_ms_min"]
    r["two_call_spread_ms"] = round(spread, 4)
    r["fused_below_two_call"] = bool(r["two_call_ms"] - r["fused_ms"] > spread)
    r["fused_over_c64"] = round(r["fused_ms"] / r["c64_ms"], 4)
    return r


def main():
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("ingest_bench: needs a GPU")
    n = int(os.environ.get("INGESTBENCH_N", 64 << 20))
    repeats = int(os.environ.get("INGESTBENCH_REPEATS", 12))
    warmup = int(os.environ.get("INGESTBENCH_WARMUP", 3))
    host_repeats = int(os.environ.get("INGESTBENCH_HOST_REPEATS", 10))
    assert repeats >= 10 and host_repeats >= 10 and warmup >= 1 and n % 4096 == 0
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    raw = torch.randint(-32768, 32768, (2 * n,), generator=g, device="cuda", dtype=torch.int32).to(torch.int16)
    raw[:6] = torch.tensor([32767, -32768, 0, -1, 1, -32767], dtype=torch.int16)
    x = L.bytes_to_iq(raw)

    res = {"n": n, "repeats": repeats, "warmup": warmup, "pkg": os.path.relpath(PKG, REPO), "rows": {}}
    ok = True
    for name, make in OBJECTS.items():
        eq = equal_bits(make, raw)
        ok = ok and eq
        r = row(measure(variants(make(), x, raw), time_device, warmup, repeats))
        r["bit_equal"] = eq
        res["rows"][name] = r
        torch.cuda.empty_cache()

    # host memory: the upload is part of the call
    raw_h = raw.cpu().numpy()
    x_h = x.cpu().numpy()
    del raw, x
    torch.cuda.empty_cache()
    make = OBJECTS["chan_16_8"]
    eq = equal_bits(make, raw_h)
    ok = ok and eq
    r = row(measure(variants(make(), x_h, raw_h), time_host, 1, host_repeats))
    r["bit_equal"] = eq
    r["repeats"] = host_repeats
    res["rows"]["chan_16_8_host"] = r

    res["bit_equal"] = ok
    line = json.dumps(res)
    print(line)
    if "--out" in sys.argv:
        with open(sys.argv[sys.argv.index("--out") + 1], "w") as f:
            f.write(line + "\n")
    if not ok:
        sys.exit("ingest_bench: a fused output differs from the two-call output")


if __name__ == "__main__":
    main()
