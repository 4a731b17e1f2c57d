"""The batched decode through the C++ drop-in header include/rwkv.h (decodeBatchGreedy / decodeBatchTypical / copyState):
tests/cpp/batch_app.cpp compiles and links on a box without a GPU; on the GPU box its ids equal the Python engine's."""
import os

import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf

from support import build_app, run_app


@pytest.fixture(scope="module")
def batch_app(built, tmp_path_factory):
    return build_app("batch_app", tmp_path_factory.mktemp("cpp"))


def test_batch_app_compiles_and_links(batch_app):
    assert os.path.exists(batch_app)


def test_batch_entry_points_are_bound(built):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    for s in ("rwkv_decode_batch_greedy", "rwkv_decode_batch_typical", "rwkv_state_copy"):
        assert s in engine.ABI_SYMBOLS and hasattr(lib, s), s
    for f in ("decode_batch_greedy", "decode_batch_typical", "copy_state"):
        assert callable(getattr(engine.RWKV, f, None)), f


@pytest.mark.gpu
def test_batch_app_matches_python_engine(batch_app, tmp_path):
    from rwkv_cpp_accelerated_amd import engine
    L, D, n, steps = 2, 256, 5, 7
    t = mf.synthetic_tensors(L, D, seed=31, head_scale=30.0)
    p = str(tmp_path / "model.bin")
    mf.write_bin(p, L, D, t)
    rc, lines, raw = run_app(batch_app, [p, n, steps])
    assert rc == 0, raw
    assert lines[-1] == "batch_ok"
    rows = np.array([[int(x) for x in l.split()] for l in lines[-1 - 2 * n:-1]], np.int64)
    m = engine.RWKV(resident=True)
    m.loadFile(p, n)
    m.forward([5, 6, 7], engine.MODE_GPT)
    for s in range(1, n):
        m.copy_state(s, 0)
    m.pull_state(n)
    snap = [a.copy() for a in m.state.arrays()]
    first = [100 + s for s in range(n)]
    g = m.decode_batch_greedy(first, steps).astype(np.int64)
    for a, b in zip(m.state.arrays(), snap):
        a[:] = b
    m.push_state(n)
    tt = m.decode_batch_typical(first, steps, temp=0.9, tau=0.8, seeds=list(range(n))).astype(np.int64)
    assert np.array_equal(rows[:n], g)
    assert np.array_equal(rows[n:], tt)
    m.close()
