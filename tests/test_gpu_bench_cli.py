"""bench.py's command line on the GPU: a plain run carries the headline figures
only, --full adds the figures that take runs of their own, --steps sets the
number of timed steps, and --dump-outputs writes the last timed step's PCM --
the same array in both modes (the timed steps do not depend on --full) and the
same as --dump-pcm.  Small blocks (4 Mi IQ samples), two child processes."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N, STEPS = 1 << 22, 2
FULL_ONLY = ("roofline", "kernels", "stage_ms", "single_stream_ms_per_step", "components", "cpu_baseline", "parity")


def _run(outdir, extra):
    cmd = [sys.executable, "bench.py", "--gpus", "1", "--steps", str(STEPS), "--warmup", "1", "--iq-samples", str(N),
           "--dump-outputs", str(outdir)] + extra
    r = subprocess.run(cmd, cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout[-2000:]
    return json.loads(lines[0])


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    d = tmp_path_factory.mktemp("bench_cli")
    plain = _run(d / "plain", ["--dump-pcm", str(d / "pcm")])
    full = _run(d / "full", ["--full", "--no-components", "--no-cpu-baseline"])
    return d, plain, full


def test_plain_line(runs):
    _, res, _ = runs
    assert res["steps"] == STEPS and res["warmup"] == 1 and res["n_gpus"] == 1 and res["full"] is False
    assert res["unit"] == "Msamples/s" and res["higher_is_better"] is True and res["dtype"] == "f32"
    assert res["metric"].startswith("Msamples/s on AM chain")
    # value = IQ samples of all timed steps over their wall time; ms_per_step = that time / steps
    assert res["ms_per_step"] > 0
    assert abs(res["value"] - N / (res["ms_per_step"] * 1e-3) / 1e6) <= 1e-3 * res["value"] + 0.01
    assert not [k for k in FULL_ONLY if k in res]


def test_full_line(runs):
    _, plain, res = runs
    assert res["full"] is True and res["steps"] == STEPS
    for k in ("roofline", "kernels", "stage_ms", "single_stream_ms_per_step"):
        assert k in res, k
    assert "components" not in res and "cpu_baseline" not in res        # --no-components, --no-cpu-baseline
    assert res["kernels"]["k_pll_walk"]["calls_per_step"] >= 1
    assert {k: v for k, v in res.items() if k in plain and k not in ("value", "ms_per_step", "host_ms_per_step",
                                                                     "host_ms_max_step", "full")} == \
           {k: v for k, v in plain.items() if k not in ("value", "ms_per_step", "host_ms_per_step", "host_ms_max_step",
                                                        "full")}


def test_dump_outputs(runs):
    d, plain, _ = runs
    assert sorted(os.listdir(d / "plain")) == ["pcm.npy"]
    a = np.load(d / "plain" / "pcm.npy")
    assert a.dtype == np.float32 and a.shape == (plain["config"]["pcm_samples_per_step"],)
    assert np.all(np.isfinite(a)) and np.any(a != 0)
    b = np.load(d / "full" / "pcm.npy")
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))          # the same timed steps with --full
    c = np.load(str(d / "pcm") + ".rank0.npy")
    assert np.array_equal(a.view(np.uint32), c.view(np.uint32))
