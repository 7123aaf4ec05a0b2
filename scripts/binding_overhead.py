"""Per-call cost of the Python binding: a loop of small device-tensor calls, in
microseconds per call, for one object of each call shape the binding has --
same-length (ComplexFIRFilter), 1-D to num_outputs (ComplexResampler), 1-D to
rows (Channelizer), rows to rows (FMBank), rows to 1-D (Synthesizer) and
Spectrogram.write.  The inputs are small (4 096 samples, [4, 1 024] rows), so
the launch and the binding's own work dominate, not the kernel.  Each row is
warmed up, then timed `--repeats` times over `--calls` calls with one
synchronize at the end of each loop (host clock); the row's figure is the
median of the repeats.  The time until the last call returned (before the
synchronize) is kept beside it: where the two agree the host is the limit, where
they do not the GPU's dispatch rate is.  Prints one JSON line (and writes it to the file named by
--out).  LDSP_PKG_DIR selects the package build."""
import argparse
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

N, ROWS, K = 4096, 4, 1024


def rows_of(L, x, xr):
    h = np.hanning(31).astype(np.float32)
    return [
        ("same_length.ComplexFIRFilter", L.ComplexFIRFilter(h), x),
        ("num_outputs.ComplexResampler", L.ComplexResampler(0.5, Fc=0.2), x),
        ("to_rows.Channelizer", L.Channelizer(ROWS), x),
        ("rows_to_rows.FMBank", L.FMBank(ROWS, 0.25, 2), xr),
        ("rows_to_1d.Synthesizer", L.Synthesizer(ROWS), xr),
        ("write.Spectrogram", L.Spectrogram(256).write, x),
    ]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--calls", type=int, default=3000)
    ap.add_argument("--warmup", type=int, default=300)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out")
    a = ap.parse_args()
    if not torch.cuda.is_available() or L.device_count() == 0:
        sys.exit("binding_overhead: no GPU")
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(9)
    x = torch.from_numpy((rng.standard_normal(N) + 1j * rng.standard_normal(N)).astype(np.complex64)).to(dev)
    xr = torch.from_numpy((rng.standard_normal((ROWS, K)) + 1j * rng.standard_normal((ROWS, K))).astype(np.complex64)).to(dev)
    res = {"package": PKG, "calls": a.calls, "warmup": a.warmup, "input_samples": N, "input_rows": [ROWS, K], "us_per_call": {}}
    for name, call, arg in rows_of(L, x, xr):
        for _ in range(a.warmup):
            call(arg)
        torch.cuda.synchronize()
        runs, host = [], []
        for _ in range(a.repeats):
            t0 = time.perf_counter()
            for _ in range(a.calls):
                call(arg)
            t1 = time.perf_counter()                   # every call enqueued: the host's share
            torch.cuda.synchronize()
            runs.append(round((time.perf_counter() - t0) / a.calls * 1e6, 3))
            host.append(round((t1 - t0) / a.calls * 1e6, 3))
        res["us_per_call"][name] = {"median": statistics.median(runs), "runs": runs,
                                    "host_median": statistics.median(host), "host_runs": host}
    line = json.dumps(res)
    print(line, flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
