"""The many-call recorder (csrc/batch.hpp, csrc/batch.cpp: BatchRecorder, the
mechanism under every execute_many / filter_resample_many / ldsp_*_many) on the
host alone: tests/sanitize/batch_driver.cpp links batch.cpp and nothing else of
the library, records op lists from tables -- equal lists, one longer, a shifted
one, a different grid / block / LDS size / kernel in the middle, xcd launches of
147, 160 and 1024 workgroups, empty lists, 1 to 17 channels, nested recorders,
and 4 000 seeded random tables -- with lambdas that log instead of launching,
and checks what flush() issues: every op once, each channel in order, groups
only of equal mergeable launches of one index, complete groups, the merged
count, an idle second flush, and batch_active() at every stage.  Built with
ASan + UBSan on the host side (`make batch_asan`); no GPU, no HIP call.
"""
import os
import subprocess

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "python-liquiddsp_amd")
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:")


def test_recorder_driver_asan_ubsan():
    r = subprocess.run(["make", "-s", "-C", PKG, "batch_asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(PKG, "build", "batch_driver_asan")
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the driver is not instrumented"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert not any(k in out for k in REPORTS), out[-4000:]
    assert "all checks passed" in r.stdout
