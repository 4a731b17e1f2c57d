"""Speculative sampling with a draft model that samples, without a GPU: the three entry points are declared, exported and bound at every layer,
and the rule the device is held to (tests/ratio_cases.py) is lossless -- the emitted id is distributed exactly as the target's p."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import ratio_cases as rc
from support import INCLUDE, rwkv_mod, syntax_only  # noqa: F401

NEW = ("rwkv_spec_ratio_rows", "rwkv_spec_verify_ratio", "rwkv_decode_speculative_sampled")


def test_declared_exported_and_bound(built, rwkv_mod, tmp_path):
    from rwkv_cpp_accelerated_amd import engine
    hdr = open(os.path.join(INCLUDE, "rwkv_mi355x.h")).read()
    lib = C.CDLL(built["engine"])
    for name in NEW:
        assert re.search(r"\bint " + name + r"\(", hdr) and hasattr(lib, name) and name in engine.ABI_SYMBOLS, name
        assert getattr(engine.lib(), name).argtypes, name
    assert C.sizeof(engine.RatioParams) == 16 and [n for n, _ in engine.RatioParams._fields_] == ["temp_target", "temp_draft", "flags", "reserved"]
    for method in ("spec_ratio_rows", "spec_verify_ratio", "decode_speculative_sampled"):
        assert callable(getattr(engine.RWKV, method, None)), method
    assert callable(getattr(rwkv_mod, "decodeSpeculativeSampled", None))
    src = tmp_path / "use_ratio.cpp"
    src.write_text('#include "rwkv.h"\n#include "rwkv_sampler.h"\nint twin(const float *l, const float *m) { return ratio_u(l, m, 5, 0.8f, 1.f, 0.5, 0.5); }\n'
                   "RWKV::SpecResult use(RWKV &m, RWKV &d) { return m.decodeSpeculativeSampled(d, 5, 16, 4, 0.8f, 1.0f, 1, 2); }\n")
    syntax_only(src)
    assert "a draft model that samples (" not in hdr                 # the two out-of-scope notes point at the new calls now


@pytest.mark.parametrize("name", ["cold_draft", "q_peaked_on_x", "x_is_0"])
def test_the_rule_is_lossless(name):
    """sum over the draft's draws x ~ q of [accept x] + [reject x] r / R is p: q(i) min(1, p(i) / q(i)) + (1 - beta) r(i) / R == p(i)"""
    l, m, _, Tt, Td = rc.cases()[name][:5]
    ru = rc.Rule(l, m, 0, Tt, Td)                                    # (x = 0: the residual without an id taken out)
    p, q, beta = ru.p, ru.q, np.minimum(ru.p, ru.q).sum()
    assert ru.R > 0 and abs((1.0 - beta) - ru.R) < 1e-12
    assert np.abs(np.minimum(p, q) + (1.0 - beta) * ru.r / ru.R - p).max() < 1e-12
