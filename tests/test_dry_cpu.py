"""DRY penalties WITHOUT a GPU: the entry points are declared, exported and bound, and the host twin include/rwkv_sampler.h dry_scan / dry_table
(tests/cpp/dry_app.cpp, a stand-alone program) gives what the Python restatement of tests/dry_cases.py gives on every planted history."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import dry_cases as dc

from support import E_ARG, ROOT, build_app, rwkv_mod  # noqa: F401

NEW = (("rwkv_dry_history_set", 4), ("rwkv_dry_history_get", 5), ("rwkv_debug_dry_scan", 6), ("rwkv_decode_batch_dry", 14))


def test_entry_points_are_declared_exported_and_bound(built, rwkv_mod):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    hdr = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    syms = subprocess.run(["nm", "-D", "--defined-only", built["engine"]], capture_output=True, text=True).stdout
    for name, n_args in NEW:
        assert name + "(" in hdr and name in engine.ABI_SYMBOLS and len(getattr(lib, name).argtypes) == n_args and f" T {name}\n" in syms, name
    assert C.sizeof(engine.DryParams) == 40 and engine.DryParams.breakers.offset == 24
    for name, val in (("WINDOW", 4096), ("MATCH", 64), ("BREAKERS", 32)):
        assert f"#define RWKV_DRY_MAX_{name} {val}u" in hdr and getattr(engine, "DRY_MAX_" + name) == val
    assert (dc.MAX_WINDOW, dc.MAX_MATCH) == (engine.DRY_MAX_WINDOW, engine.DRY_MAX_MATCH)
    assert lib.rwkv_decode_batch_dry(None, None, 1, 1, None, None, None, None, None, None, None, None, None, None) == E_ARG
    assert lib.rwkv_debug_dry_scan(None, 0, None, None, None, None) == E_ARG and lib.rwkv_dry_history_set(None, 0, None, 0) == E_ARG
    for f in ("dry_history_set", "dry_history_get", "debug_dry_scan", "decode_batch_dry"):
        assert callable(getattr(engine.RWKV, f, None)), f
    assert callable(rwkv_mod.decodeBatchDry) and "decodeBatchDry(" in open(os.path.join(ROOT, "include", "rwkv.h")).read()


@pytest.fixture(scope="module")
def twin(tmp_path_factory):
    """{case: [(id, L)]} and the table's bit patterns, from ONE run of the C++ twin over every planted history"""
    d = tmp_path_factory.mktemp("dry")
    exe = build_app("dry_app", d, link=False, extra=("-Wall",))
    with open(d / "cases.txt", "w") as f:
        for hist, kw in dc.CASES.values():
            br = list(kw.get("breakers", ()))
            f.write(" ".join(str(v) for v in [kw.get("allowed_length", 2), kw.get("window", dc.MAX_WINDOW), len(br), *br, len(hist), *hist]) + "\n")
    out = subprocess.run([exe, str(d / "cases.txt")], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    lines = [[int(v) for v in l.split()[1 if l.startswith("table") else 0:]] for l in out.stdout.split("\n")[: len(dc.CASES) + 1]]
    return dict(zip(dc.CASES, ([tuple(l[i: i + 2]) for i in range(0, len(l), 2)] for l in lines))), lines[-1]


@pytest.mark.parametrize("name", list(dc.CASES))
def test_host_twin_is_the_restatement(twin, name):
    assert twin[0][name] == dc.expected(name)


def test_host_table_is_bit_exact(twin):
    pen, ban = dc.table(0.8, 1.75), dc.table(np.inf, 1.75)
    assert twin[1] == [int(np.float32(v).view(np.uint32)) for v in (pen[0], pen[1], pen[63], ban[63])] and np.isinf(ban).all() and pen[0] == np.float32(0.8)
