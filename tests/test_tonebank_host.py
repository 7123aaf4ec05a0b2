"""Host side of the ToneBank without a GPU (CPU suite): the exported ldsp_tonebank_* symbols,
defaults and getters, every argument error of the constructor and the setters with its text
(decided before any device work), the tables against the double formula, num_outputs and
fill over cut streams (through the C ABI's closed form; execute needs a device), the
detection rule and the hold window restated in numpy (tests/tonebank_model.py, the rule the
GPU test holds the kernel to) on hand-made powers, and the stand-alone C driver of the same
host code under ASan + UBSan (tests/sanitize/tonebank_driver.c).  The GPU side is
tests/test_gpu_tonebank.py."""
import os
import re
import subprocess

import numpy as np
import pytest

import tonebank_model as M

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PKG = os.path.join(REPO, "python-liquiddsp_amd")
LIBPATH = os.path.join(PKG, "libldsp.so")
HEADER = os.path.join(REPO, "include", "ldsp.h")

CTCSS = [67.0, 71.9, 74.4, 77.0, 79.7, 82.5, 85.4, 88.5, 91.5, 94.8, 97.4, 100.0, 103.5, 107.2, 110.9, 114.8, 118.8,
         123.0, 127.3, 131.8, 136.5, 141.3, 146.2, 151.4, 156.7, 159.8, 162.2, 165.5, 167.9, 171.3, 173.8, 177.3, 179.9,
         183.5, 186.2, 189.9, 192.8, 196.6, 199.5, 203.5, 206.5, 210.7, 218.1, 225.7, 229.1, 233.6, 241.8, 250.3, 254.1]


@pytest.fixture(scope="module")
def ld():
    import liquiddsp
    return liquiddsp


# ---------------------------------------------------------------- symbols
def test_library_exports_what_the_header_declares():
    with open(HEADER) as f:
        names = set(re.findall(r"\b(ldsp_(?:debug_)?tonebank_\w+)\s*\(", f.read()))
    want = {"ldsp_tonebank_" + n for n in (
        "create", "destroy", "reset", "get_info", "get_tables", "set_want", "get_want", "set_dominance", "get_dominance",
        "set_floor", "get_floor", "num_outputs", "execute", "get_state")} | {"ldsp_debug_tonebank_tile"}
    assert want == names, sorted(want ^ names)
    out = subprocess.run(["nm", "-D", "--defined-only", LIBPATH], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\b(ldsp_(?:debug_)?tonebank_\w+)\b", out))
    assert exported == want, sorted(exported ^ want)


# ---------------------------------------------------------------- construction
def test_defaults_and_getters(ld):
    f = np.array(CTCSS) / 8000.0
    tb = ld.ToneBank(16, f)
    assert (tb.nchan, tb.ntones, tb.block, tb.window, tb.dominance, tb.floor, tb.hold, tb.fill) == \
        (16, 49, 4096, "hann", 8.0, 0.0, 1, 0)
    assert tb.tones.dtype == np.float64 and np.array_equal(tb.tones, f)
    assert tb.want.tolist() == [-1] * 16
    assert tb.tone is None and tb.power is None and tb.open is None
    assert tb.state.tolist() == [M.SAT] * 16          # before the first call: nothing accepted within reach
    assert tb.tile % 32 == 0 and tb.tile >= 32
    tb.want = 3
    assert tb.want.tolist() == [3] * 16
    tb.want = np.arange(16) - 1
    assert tb.want.tolist() == list(range(-1, 15))
    tb.dominance = 1.0
    tb.floor = 0.125
    assert (tb.dominance, tb.floor) == (1.0, 0.125)
    tb.reset()                                        # keeps the settings
    assert (tb.dominance, tb.floor, tb.want.tolist()) == (1.0, 0.125, list(range(-1, 15)))
    tb2 = ld.ToneBank(3, [0.1, 0.2], block=64, window="rect", dominance=2.0, floor=0.5, hold=64, want=[0, 1, -1])
    assert (tb2.block, tb2.window, tb2.dominance, tb2.floor, tb2.hold) == (64, "rect", 2.0, 0.5, 64)
    assert tb2.want.tolist() == [0, 1, -1]


F3 = [0.1, 0.2, 0.3]


@pytest.mark.parametrize("kw, text", [
    (dict(tones=[0.1]), "the number of tones must lie in 2 .. 64"),                                    # F = 1
    (dict(tones=list(np.linspace(0.01, 0.49, 65))), "the number of tones must lie in 2 .. 64"),        # F = 65
    (dict(tones=[0.1, 0.0, 0.3]), "tones must lie in (0, 0.5) cycles per sample"),
    (dict(tones=[0.1, 0.5, 0.3]), "tones must lie in (0, 0.5) cycles per sample"),
    (dict(tones=[0.1, float("nan"), 0.3]), "tones must lie in (0, 0.5) cycles per sample"),
    (dict(tones=[0.1, float("inf"), 0.3]), "tones must lie in (0, 0.5) cycles per sample"),
    (dict(block=63), "the block length must be a multiple of 64 in 64 .. 16384"),
    (dict(block=100), "the block length must be a multiple of 64 in 64 .. 16384"),
    (dict(block=16448), "the block length must be a multiple of 64 in 64 .. 16384"),
    (dict(block=-64), "block must be a multiple of 64 in 64 .. 16384"),
    (dict(hold=65), "the hold must lie in 0 .. 64 blocks"),
    (dict(hold=-1), "hold must lie in 0 .. 64"),
    (dict(want=3), "want must lie in -1 .. F - 1"),                                                    # want = F
    (dict(want=-2), "want must be integers in -1 .. F - 1"),
    (dict(want=0.5), "want must be integers in -1 .. F - 1"),
    (dict(want=[0, 1]), "one wanted tone or one per row"),                                             # wrong length
    (dict(want=[0, 1, 2, 0]), "one wanted tone or one per row"),
    (dict(nchan=0), "the row count must lie in 1 .. 256"),
    (dict(nchan=257), "the row count must lie in 1 .. 256"),
    (dict(window="hamming"), "window must be 'hann' or 'rect'"),
    (dict(dominance=0.5), "the dominance must be finite and >= 1"),
    (dict(dominance=float("nan")), "the dominance must be finite and >= 1"),
    (dict(floor=-1.0), "the floor must be finite and >= 0"),
    (dict(floor=float("nan")), "the floor must be finite and >= 0"),
])
def test_argument_errors_and_their_texts(ld, kw, text):
    args = dict(nchan=3, tones=F3, block=256)
    args.update(kw)
    with pytest.raises(ValueError) as e:
        ld.ToneBank(**args)
    assert text in str(e.value), str(e.value)


def test_setter_errors_leave_the_settings(ld):
    tb = ld.ToneBank(3, F3, block=256, want=[0, 1, 2])
    for name, bad in (("want", 3), ("want", [0, 1]), ("want", float("nan")), ("dominance", 0.99),
                      ("dominance", float("nan")), ("floor", -0.1), ("floor", float("nan")), ("floor", float("inf"))):
        with pytest.raises(ValueError):
            setattr(tb, name, bad)
    assert (tb.want.tolist(), tb.dominance, tb.floor) == ([0, 1, 2], 8.0, 0.0)


# ---------------------------------------------------------------- tables
@pytest.mark.parametrize("B, name", [(64, "hann"), (192, "rect"), (4096, "hann"), (16384, "hann")])
def test_tables_follow_the_double_formula(ld, B, name):
    f = np.array([0.3 / B * 7, 0.0137, 0.1, 0.25, 0.4999])
    tb = ld.ToneBank(2, f, block=B, window=name)
    t = tb.tables
    assert t.dtype == np.float32 and t.shape == (2, 5, B)
    tc, ts, sumw = M.tables64(f, B, name)
    # sum w and the scale: B / 2 for the periodic Hann window, B for the rectangle
    assert abs(tb.window_sum - sumw) <= 1e-13 * sumw
    assert abs(sumw - (B / 2 if name == "hann" else B)) <= 1e-9 * B
    for got, ref in ((t[0], tc), (t[1], ts)):
        # one float32 rounding of the entry: half a unit in the last place of the double value
        # (0.501: the two libraries' cos may differ in the double's last bit)
        half_ulp = np.spacing(np.abs(ref).astype(np.float32)).astype(np.float64) * 0.501
        assert (np.abs(got.astype(np.float64) - ref) <= half_ulp + 1e-300).all()
    # a full-scale tone at f_k reads 1 / 2: |sum (Tc + i Ts) cos|^2, up to the image's leakage
    i = np.arange(B)
    x = np.cos(2 * np.pi * f[2] * i)
    p = M.power64(t, x[None, :])[0, 0]
    # (the image at -f, 2 f B bins away: the rectangle's side lobes fall as 1 / (pi bins), 1.7e-2
    # of the amplitude at 19 bins; Hann's as bins^-3)
    assert abs(p[2] - 0.5) < (4e-2 if name == "rect" else (2e-2 if B == 64 else 2e-3))


# ---------------------------------------------------------------- stream bookkeeping
def test_num_outputs_over_cut_streams(ld):
    rng = np.random.default_rng(5)
    for B in (64, 192, 4096):
        tb = ld.ToneBank(2, F3, block=B)
        assert [tb.num_outputs(k) for k in (0, 1, B - 1, B, B + 1, 3 * B - 1, 3 * B)] == [0, 0, 0, 1, 1, 2, 3]
        # fill moves only with a call that ran; without a device the call fails and consumes nothing
        seen = 0
        for K in rng.integers(0, 3 * B, 12):
            x = np.zeros((2, int(K)), np.float32)
            want = (seen + int(K)) // B - seen // B
            assert tb.num_outputs(int(K)) == want
            try:
                y = tb(x)
            except RuntimeError:
                assert tb.fill == seen % B
                continue
            seen += int(K)
            assert y.shape == (2, want * B) and tb.fill == seen % B
            assert tb.tone.shape == (2, want) and tb.power.shape == (2, want, 3) and tb.open.shape == (2, want)


# ---------------------------------------------------------------- the rule
def test_rule_tie_goes_to_the_lowest_index():
    p = np.array([[[0.0, 2.0, 2.0, 0.0]]], np.float32)
    k, hit = M.detect(p, 0.0, 1.0)
    assert k[0, 0] == 1 and hit[0, 0]                 # 2 * 3 > 1 * 2
    tone, opn, nxt, _ = M.decide(p, 0.0, 1.0, [2], 0, [M.SAT])
    assert tone[0, 0] == 1 and opn[0, 0] == 0         # the tie's other index is not the block's tone


def test_rule_zeros_nan_floor_and_dominance_are_strict():
    z = np.zeros((1, 1, 4), np.float32)
    assert not M.detect(z, 0.0, 1.0)[1][0, 0]         # 0 > 0 fails twice
    n = np.array([[[1.0, np.nan, 0.0, 0.0]]], np.float32)
    assert not M.detect(n, 0.0, 1.0)[1][0, 0]
    n = np.array([[[np.inf, 0.0, 0.0, 0.0]]], np.float32)
    assert not M.detect(n, 0.0, 1.0)[1][0, 0]
    fl = np.float32(0.1)
    p = np.array([[[fl, 0.0, 0.0, 0.0]]], np.float32)
    assert not M.detect(p, fl, 1.0)[1][0, 0]          # power exactly equal to the floor
    assert M.detect(p, np.nextafter(fl, np.float32(0)), 1.0)[1][0, 0]
    # a ratio exactly equal to dominance: best 8, others 1 + 1 + 1, F - 1 = 3: 24 > 8 * 3 fails
    p = np.array([[[1.0, 8.0, 1.0, 1.0]]], np.float32)
    assert not M.detect(p, 0.0, 8.0)[1][0, 0]
    assert M.detect(p, 0.0, np.nextafter(8.0, 0.0))[1][0, 0]
    # the compare is in float64 on the float32 powers: a last-bit excess decides
    p[0, 0, 1] = np.nextafter(np.float32(8.0), np.float32(9.0))
    assert M.detect(p, 0.0, 8.0)[1][0, 0]


def test_rule_hold_window_across_a_call_boundary():
    F, hold = 3, 2
    hitp, miss = [4.0, 0.0, 0.0], [1.0, 1.0, 1.0]
    seq = [1, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0]           # accepted blocks
    p = np.array([[hitp if s else miss for s in seq]], np.float32)
    want_open = [1, 1, 1, 0, 1, 1, 1, 0, 0, 1, 1]
    tone, opn, nxt, acc = M.decide(p, 0.0, 2.0, -1, hold, [M.SAT])
    assert acc[0].tolist() == [bool(s) for s in seq] and opn[0].tolist() == want_open and nxt[0] == 1
    assert tone[0].tolist() == [0 if s else -1 for s in seq]
    for cut in range(len(seq) + 1):                   # every cut into two calls, the counter carried
        t1, o1, n1, _ = M.decide(p[:, :cut], 0.0, 2.0, -1, hold, [M.SAT])
        t2, o2, n2, _ = M.decide(p[:, cut:], 0.0, 2.0, -1, hold, n1)
        assert np.concatenate([o1, o2], axis=1)[0].tolist() == want_open, cut
        assert n2[0] == 1
    # the counter saturates and a wanted tone other than the block's does not open
    assert M.decide(np.array([[miss] * 200], np.float32), 0.0, 2.0, -1, hold, [0])[2][0] == M.SAT
    assert M.decide(p, 0.0, 2.0, 1, hold, [M.SAT])[1].sum() == 0
    g = M.gate(np.arange(8, dtype=np.float32)[None, :] + 1, np.array([[0, 1]], np.uint8), 4)
    assert g.tolist() == [[0, 0, 0, 0, 5, 6, 7, 8]] and not np.signbit(g[0, 0])


# ---------------------------------------------------------------- sanitizers
REPORTS = ("ERROR: AddressSanitizer", "ERROR: LeakSanitizer", "runtime error:")


def test_tonebank_driver_asan_ubsan():
    """The host code of the C ABI (creation, the table design, getters and setters, argument
    checks, num_outputs, the no-device execute path) in a stand-alone instrumented program; no
    GPU and nothing loaded into Python."""
    r = subprocess.run(["make", "-s", "-j8", "-C", PKG, "tonebank_asan"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr[-3000:]
    exe = os.path.join(PKG, "build", "tonebank_driver_asan")
    syms = subprocess.run(["nm", exe], capture_output=True, text=True).stdout
    assert "__asan_init" in syms and "__ubsan_handle" in syms, "the driver is not instrumented"
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1")
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, out[-4000:]
    assert not any(k in out for k in REPORTS), out[-4000:]
    assert "all checks passed" in r.stdout
