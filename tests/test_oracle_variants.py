"""CPU: the build variants of the restatement (oracle/Makefile,
oracle.variant()) reproduce their committed outputs (tests/golden/variants.npz)
and the divergences recorded in variants.json; the default variant is the
golden fixture itself.  See tests/golden/make_variants.py for why the variants
exist (liquid-dsp's output depends on its libm and its SIMD dotprod order)."""
import json
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))

V = np.load(os.path.join(HERE, "golden", "variants.npz"))
G = dict(np.load(os.path.join(HERE, "golden", "golden.npz")),
         chain_x=np.load(os.path.join(HERE, "golden", "golden_chain_x.npy")))   # (a file of its own, for size)
META = json.load(open(os.path.join(HERE, "golden", "variants.json")))


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64 if a.dtype == np.complex64 else np.uint32)


@pytest.mark.parametrize("v", ["default", "libm", "simd", "libm_simd"])
def test_variant_reproduces_fixture(ora, v):
    from make_variants import stage_outputs
    outs = stage_outputs(ora.variant(v), dict(G))
    for k, y in outs.items():
        assert np.array_equal(_bits(y), _bits(V[f"{v}__{k}"])), (v, k)


def test_default_variant_is_the_golden_fixture():
    for k in ("fir127_y", "resamp_y", "agc_y", "ampmodem_y", "ampmodem_costas_y", "chain_y"):
        assert np.array_equal(_bits(V[f"default__{k}"]), _bits(G[k])), k


def test_variants_really_differ_and_stay_close_per_stage():
    gi = META["golden_inputs"]
    # the switches do something: libm moves the loops, SIMD order moves the dot products
    assert gi["agc_y"]["libm"]["maxrel"] > 0 and gi["agc_y"]["simd"]["maxrel"] == 0
    assert gi["fir127_y"]["simd"]["maxrel"] > 0 and gi["fir127_y"]["libm"]["maxrel"] == 0
    # one stage at a time, every variant agrees within SURVEY 8(d)'s 1e-6
    for stage in ("fir127_y", "resamp_y", "agc_y", "ampmodem_y", "ampmodem_costas_y"):
        for v, d in gi[stage].items():
            assert d["maxrel"] <= 1e-6, (stage, v, d)
    # end to end the PLL's table index amplifies any difference: the chain spread
    assert 1e-4 < META["chain_variant_spread_maxrel"] < 1e-2
