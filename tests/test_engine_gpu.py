"""GPU parity tests proper: the HIP engine (through the C-ABI) against the CPU oracle on the same
seeded inputs.  Run on the MI355X box with `-m gpu`."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from rwkv_cpp_accelerated_amd import modelfile as mf
import parity
from support import ROOT, eng  # noqa: F401

pytestmark = pytest.mark.gpu


def _model(eng, L, D, seed, maxGPT=1, resident=True):
    t = mf.synthetic_tensors(L, D, seed=seed)
    m = eng.RWKV(resident=resident)
    m.loadTensors(L, D, t, maxGPT=maxGPT)
    return m, t


@pytest.mark.parametrize("L,D", [(2, 64), (3, 768), (2, 1024), (2, 2048), (1, 2560), (1, 4096), (1, 5120)])
def test_token_logits_vs_oracle(eng, oracle, L, D):
    """teacher-forced single-token decode: per-step logits and state vs the CPU restatement"""
    m, t = _model(eng, L, D, seed=100 + D)
    om = oracle.from_tensors(L, D, t)
    st = om.new_state()
    toks = [11, 50276, 1, 4097, 11, 333]
    for step, tk in enumerate(toks):
        ref = om.forward([tk], st)[0]
        got = m.forward(tk)[: mf.VOCAB]
        parity.check_logits(got, ref, f"L{L} D{D} step {step}")
        parity.check_argmax(got, ref, f"L{L} D{D} step {step}")
    m.pull_state(1)
    for name, g, r in zip("xy aa bb pp dd".split(), m.state.arrays(), st):
        scale = max(1.0, np.abs(r).max())
        assert np.abs(g[: L * D] - r).max() <= 1e-4 * scale, name
    om.close(); m.close()


def test_gpt_mode_chunk_equals_token_by_token(eng, oracle):
    """GPT mode: T consecutive tokens of one sequence (rwkv.cu:227-240); logits for every position"""
    L, D, T = 2, 768, 5
    m, t = _model(eng, L, D, seed=5, maxGPT=8)
    om = oracle.from_tensors(L, D, t)
    toks = [9, 8, 7, 50000, 6]
    ref = om.forward(toks, om.new_state())
    got = m.forward(toks, eng.MODE_GPT)[: T * mf.VOCAB].reshape(T, mf.VOCAB).copy()
    for i in range(T):
        parity.check_logits(got[i], ref[i], f"pos {i}")
    m.reset_state()
    one = np.stack([m.forward(tk)[: mf.VOCAB].copy() for tk in toks])
    for i in range(T):                       # chunk (MFMA path, seq.hip.h) vs token-by-token (GEMV path)
        parity.check_logits(got[i], one[i], f"chunk vs single pos {i}")
        parity.check_argmax(got[i], one[i], f"chunk vs single pos {i}")
    m.close()
    # with the chunked path switched off a GPT-mode call is the same kernels token by token: bit for bit
    os.environ["RWKV_SEQ"] = "0"
    try:
        m2 = eng.RWKV(resident=True)
        m2.loadTensors(L, D, t, maxGPT=8)
    finally:
        del os.environ["RWKV_SEQ"]
    got2 = m2.forward(toks, eng.MODE_GPT)[: T * mf.VOCAB].reshape(T, mf.VOCAB).copy()
    assert np.array_equal(one, got2)
    om.close(); m2.close()


def test_parralel_mode_independent_slots(eng, oracle):
    """PARRALEL mode: one step of T independent sequences, state slot t (rwkv.cu:238-240)"""
    L, D, T = 2, 768, 3
    m, t = _model(eng, L, D, seed=6, maxGPT=4, resident=False)
    om = oracle.from_tensors(L, D, t)
    sp = om.new_state(slots=T)
    for rnd, toks in enumerate([[3, 4, 5], [6, 7, 3]]):
        ref = om.forward(toks, sp, mode=0)
        got = m.forward(toks, eng.MODE_PARRALEL)[: T * mf.VOCAB].reshape(T, mf.VOCAB)
        for i in range(T):
            parity.check_logits(got[i], ref[i], f"round {rnd} slot {i}")
    for g, r in zip(m.state.arrays(), sp):      # host-authoritative (drop-in) mode: state came back
        assert np.abs(g[: T * L * D] - r).max() <= 1e-4 * max(1.0, np.abs(r).max())
    om.close(); m.close()


def test_load_file_equals_load_tensors(eng, tmp_path):
    L, D = 2, 768
    t = mf.synthetic_tensors(L, D, seed=8)
    p = str(tmp_path / "model.bin")
    mf.write_bin(p, L, D, t)
    a = eng.RWKV(resident=True); a.loadFile(p)
    b = eng.RWKV(resident=True); b.loadTensors(L, D, t)
    import torch
    tt = [None if (x is None or i in mf.BUFFER_SLOTS) else torch.from_numpy(np.ascontiguousarray(x)).cuda() for i, x in enumerate(t)]
    c = eng.RWKV(resident=True); c.loadTensors(L, D, tt)
    assert (a.num_layers, a.num_embed) == (L, D)
    for tk in (5, 6):
        la = a.forward(tk).copy(); lb = b.forward(tk).copy(); lc = c.forward(tk).copy()
        assert np.array_equal(la, lb) and np.array_equal(la, lc)
    with pytest.raises(RuntimeError, match="already loaded"):
        a.loadFile(p)
    with pytest.raises(eng.RWKVError, match="Error opening file"):
        eng.RWKV().loadFile(str(tmp_path / "nope.bin"))
    with pytest.raises(RuntimeError, match="Context too large"):
        a.forward([1, 2], eng.MODE_GPT)
    for x in (a, b, c):
        x.close()


def test_state_roundtrip_and_snapshot(eng):
    """RWKVState value semantics (rwkv.h:140-242): snapshot, diverge, restore => identical logits"""
    L, D = 2, 768
    m, _ = _model(eng, L, D, seed=9, resident=False)
    for tk in (1, 2, 3):
        m.forward(tk)
    snap = m.state.getSubState(0)
    l_a = m.forward(10).copy()
    m.forward(11)
    m.state.setSubState(snap, 0)
    l_b = m.forward(10).copy()
    assert np.array_equal(l_a, l_b)
    m.close()


def test_decode_greedy_matches_host_loop(eng):
    """device-side argmax feedback == host loop of forward + argmax(out[0] banned)"""
    L, D, n = 2, 1024, 24
    m, _ = _model(eng, L, D, seed=10)
    ids = m.decode_greedy(42, n)
    last = m.logits(1).copy()
    m.reset_state()
    tk, want = 42, []
    for _ in range(n):
        lg = m.forward(tk)[: mf.VOCAB]
        tk = parity.argmax_ban0(lg); want.append(tk)
    assert list(map(int, ids)) == want
    assert np.array_equal(last, m.out[: mf.VOCAB])
    m.close()


def test_full_size_properties_7b_layer(eng):
    """BASELINE.json full width (D=4096) through size-independent properties: determinism (no float
    atomics => bit-identical reruns) and state-slot independence.  (The GEMV kernels themselves are checked one launch at a time in
    tests/test_kernels_gpu.py.)"""
    import torch
    L, D = 2, 4096
    t = mf.synthetic_tensors_torch(L, D, seed=3)
    m = eng.RWKV(resident=True); m.loadTensors(L, D, t, maxGPT=2)
    a = m.forward([7, 9], eng.MODE_PARRALEL)[: 2 * mf.VOCAB].copy()
    m.reset_state()
    b = m.forward([9, 7], eng.MODE_PARRALEL)[: 2 * mf.VOCAB].copy()
    assert np.array_equal(a[: mf.VOCAB], b[mf.VOCAB:]) and np.array_equal(a[mf.VOCAB:], b[: mf.VOCAB])
    m.reset_state()
    c = m.forward([7, 9], eng.MODE_PARRALEL)[: 2 * mf.VOCAB].copy()
    assert np.array_equal(a, c)
    m.close()


def test_pipeline_virtual_stages_equal_full_model(eng):
    """layer pipeline with all stages co-located on one GPU (same code path as the multi-GPU run minus
    the RCCL hop): chaining the stage contexts reproduces the full model's greedy ids and logits"""
    import torch
    from rwkv_cpp_accelerated_amd import pipeline
    L, D, n = 6, 768, 6
    t = mf.synthetic_tensors(L, D, seed=55)
    full = eng.RWKV(resident=True); full.loadTensors(L, D, t, maxGPT=2)
    parts = pipeline.partition_layers(L, 3, D)
    stages = [pipeline.EngineStage(t, L, D, l0, l1, n_slots=2) for l0, l1 in parts]
    assert stages[0].first and stages[-1].last and not stages[1].first and not stages[1].last
    for slot, tk0 in ((0, 17), (1, 4242)):          # two independent streams on two state slots
        tk_p = tk_f = tk0
        for step in range(n):
            # the full model on the same state slot goes through the same single-token stage entry point
            tk_f = full.stage_forward(tk_f, slot, want_pick=True)
            for i, st in enumerate(stages):
                if i > 0:
                    st.x.copy_(stages[i - 1].x); torch.cuda.synchronize()
                tk_p_next = st.forward(tk_p, slot, want_pick=st.last)
            tk_p = tk_p_next
            assert tk_p == tk_f, (slot, step)
            a = full.logits(2)[slot * mf.VOCAB:(slot + 1) * mf.VOCAB].copy()
            b = stages[-1].m.logits(2)[slot * mf.VOCAB:(slot + 1) * mf.VOCAB].copy()
            assert np.array_equal(a, b)            # bit-identical: same kernels, same data
    assert stages[1].m.bytes_per_token() == 13 * (parts[1][1] - parts[1][0]) * D * D + 168 * (parts[1][1] - parts[1][0]) * D + 40 * D
    for s in stages:
        s.m.close()
    full.close()


def test_long_decode_is_stable_and_deterministic(eng):
    """thousands of device-side steps: ids reproducible run to run, state and logits stay finite"""
    L, D, n = 4, 2048, 3000
    t = mf.synthetic_tensors(L, D, seed=21)
    m = eng.RWKV(resident=True)
    m.loadTensors(L, D, t)
    a = m.decode_greedy(17, n)
    la = m.logits(1).copy()
    m.reset_state()
    b = m.decode_greedy(17, n)
    assert np.array_equal(a, b) and np.array_equal(la, m.logits(1))
    assert np.isfinite(la).all() and a.max() < mf.VOCAB and (a != 0).all()      # token 0 is banned
    m.pull_state(1)
    for arr in m.state.arrays():
        assert np.isfinite(arr[: L * D]).all()
    with pytest.raises(eng.RWKVError):
        m.decode_greedy(17, (1 << 16) + 1)                                      # beyond the generated-id buffer
    m.close()


def test_graph_replay_equals_eager_launches(eng):
    """the captured hipGraph and plain stream launches run the same kernels: bit-identical logits"""
    L, D = 2, 1024
    t = mf.synthetic_tensors(L, D, seed=22)
    m = eng.RWKV(resident=True)
    m.loadTensors(L, D, t)
    os.environ["RWKV_GRAPH"] = "2"          # bit 0 clear: the token's kernels are launched one by one
    try:
        e = eng.RWKV(resident=True)
        e.loadTensors(L, D, t)
    finally:
        del os.environ["RWKV_GRAPH"]
    for tk in (3, 50000, 77, 3):
        assert np.array_equal(m.forward(tk)[: mf.VOCAB], e.forward(tk)[: mf.VOCAB])
    assert np.array_equal(m.decode_greedy(5, 40), e.decode_greedy(5, 40))
    m.close(); e.close()


def _pipe_worker(rank, world, port, first_tokens, L, D, seed, steps, q):
    import torch.distributed as dist
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from rwkv_cpp_accelerated_amd import pipeline
    os.environ["MASTER_ADDR"] = "127.0.0.1"; os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    l0, l1 = pipeline.partition_layers(L, world, D)[rank]
    st = pipeline.EngineStage(mf.synthetic_tensors(L, D, seed=seed), L, D, l0, l1, n_slots=world, device=0)
    picks = pipeline.run_pipeline(st, dist, rank, world, first_tokens, steps, device="cuda:0")
    if rank == world - 1:
        q.put(picks)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_pipeline_processes_with_engine_stages(eng, world):
    """bench.py's N > 1 path end to end, minus RCCL: `world` processes, each an EngineStage on its layer range
    (all on this box's one GPU), the residual hop through gloo.  Must equal single-context greedy decoding of
    every stream."""
    import socket
    import torch.multiprocessing as mp
    L, D, seed, steps = 6, 768, 77, 6
    first = [11, 222, 3333][:world]
    t = mf.synthetic_tensors(L, D, seed=seed)
    m = eng.RWKV(resident=True)
    m.loadTensors(L, D, t)
    want = np.zeros((world, steps), np.int64)
    for k, tk in enumerate(first):
        ids = []
        m.reset_state()
        cur = tk
        for _ in range(steps):
            cur = parity.argmax_ban0(m.forward(cur)[: mf.VOCAB]); ids.append(cur)
        want[k] = ids
    m.close()
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0)); port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_pipe_worker, args=(r, world, port, first, L, D, seed, steps, q)) for r in range(world)]
    [p.start() for p in procs]
    got = q.get(timeout=240)
    [p.join(timeout=60) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    assert np.array_equal(got, want)


def test_config1_169m_reference_converter_file_greedy_decode(eng, oracle, tmp_path):
    """BASELINE config 1: RWKV-4 169M (L=12, D=768), a model.bin equal to what the REFERENCE CONVERTER writes for the
    checkpoint (tests/golden/converter_169M.npz holds the sha256 of every tensor of the reference converter's own file;
    the offset vectors may differ by 4e-7, torch's vs numpy's reduction order), storygen-style greedy decode (out[0]
    banned) on the CPU path (the oracle = restated reference) and through the engine: same ids, logits within 1e-3."""
    import test_converter_cpu as tc
    from rwkv_cpp_accelerated_amd import converter
    fix = os.path.join(tc.GOLD, "converter_169M.npz")
    g = np.load(fix)
    L, D, seed = int(g["L"]), int(g["D"]), int(g["seed"])
    assert (L, D) == mf.SHAPES["169M"]
    _, _, t = converter.convert_state_dict(converter.synthetic_state_dict(L, D, seed))
    assert tc.converted_equals_reference_file(g, t) >= mf.N_TENSORS - 8
    p = str(tmp_path / "model.bin")
    mf.write_bin(p, L, D, t)
    assert os.path.getsize(p) == int(g["file_bytes"])
    m = eng.RWKV(resident=True); m.loadFile(p, 32)
    om = oracle.open_file(p)
    st = om.new_state()
    prompt = [int(x) for x in np.random.default_rng(169).integers(2, mf.VOCAB, 40)]
    ref = om.forward(prompt, st)                                   # the reference's loadContext semantics, token by token
    got = m.forward(prompt[:32], eng.MODE_GPT)                 # the engine: a 32-token chunk, then the rest
    got = m.forward(prompt[32:], eng.MODE_GPT)[: 8 * mf.VOCAB].reshape(8, mf.VOCAB)[-1]
    parity.check_logits(got, ref[-1], "169M prompt")
    tk = parity.argmax_ban0(ref[-1])
    ids_ref, ids_eng = [], []
    for step in range(48):                                         # storygen's loop with argmax (storygen.cpp:63-69)
        lr = om.forward([tk], st)[0]
        le = m.forward(tk)[: mf.VOCAB]
        parity.check_logits(le, lr, f"169M step {step}")
        parity.check_argmax(le, lr, f"169M step {step}")
        ids_ref.append(parity.argmax_ban0(lr)); ids_eng.append(parity.argmax_ban0(le))
        tk = ids_ref[-1]
    assert len(set(ids_ref)) > 8
    om.close(); m.close()


def test_abi_version_and_small_grid_is_rejected(eng, monkeypatch):
    """the library reports the C-ABI version of include/rwkv_mi355x.h; RWKV_GRID below ceil(D / 512) is refused at load"""
    assert eng.lib().rwkv_abi_version() == eng.ABI_VERSION
    monkeypatch.setenv("RWKV_GRID", "3")
    m = eng.RWKV(resident=True)
    with pytest.raises(eng.RWKVError, match="RWKV_GRID"):
        m.loadTensors(1, 2048, mf.synthetic_tensors(1, 2048, seed=3))
    m.close()
    monkeypatch.setenv("RWKV_GRID", "8")           # a small but sufficient grid still computes the same thing
    t = mf.synthetic_tensors(1, 1024, seed=4)
    a = eng.RWKV(resident=True); a.loadTensors(1, 1024, t)
    monkeypatch.delenv("RWKV_GRID")
    b = eng.RWKV(resident=True); b.loadTensors(1, 1024, t)
    la = np.array(a.forward(9)[: mf.VOCAB]); lb = np.array(b.forward(9)[: mf.VOCAB])
    assert np.abs(la.astype(np.float64) - lb).max() <= 1e-5 * np.abs(lb).max()
    assert a.resident_bytes() > 0
    a.close(); b.close()


def _decodes_like_the_oracle(eng, oracle, m, what):
    """a valid load on handle m, then two tokens against the oracle"""
    L, D = 1, 80
    t = mf.synthetic_tensors(L, D, seed=81)
    m.loadTensors(L, D, t)
    om = oracle.from_tensors(L, D, t)
    st = om.new_state()
    for tk in (5, mf.VOCAB - 1):
        parity.check_logits(m.forward(tk)[: mf.VOCAB], om.forward([tk], st)[0], what)
    om.close()


@pytest.mark.parametrize("L,D", [(1, 8), (1, 24), (1, 1032), (1, 5136), (0, 64)])
def test_a_model_shape_outside_the_accepted_set_is_refused_before_anything_is_read(eng, oracle, L, D):
    """n_embed must be a multiple of 16 up to 5120 and n_layers at least 1: anything else is RWKV_E_ARG with a message, and the handle
    takes a valid model afterwards.  The tensors have the size the call states (for n_layers 0: a one-layer model's, which is more),
    so a shape check that moved behind an upload would upload garbage and fail here instead of reading out of bounds."""
    t = mf.synthetic_tensors(max(L, 1), D, seed=5)
    m = eng.RWKV(resident=True)
    with pytest.raises(eng.RWKVError, match=r"unsupported model shape.*status -1"):
        m.loadTensors(L, D, t)
    assert not m.ready
    del t
    _decodes_like_the_oracle(eng, oracle, m, f"after the refusal of L{L} D{D}")
    m.close()


def test_the_smallest_grid_is_exact_at_the_widest_model(eng, oracle, monkeypatch):
    """RWKV_GRID = 9 at D = 5120 is one workgroup short of 512 channels each (10 is accepted: test_kernels_gpu.py)"""
    monkeypatch.setenv("RWKV_GRID", "9")
    m = eng.RWKV(resident=True)
    with pytest.raises(eng.RWKVError, match=r"RWKV_GRID=9 is too small.*need >= 10.*status -1"):
        m.loadTensors(1, 5120, mf.synthetic_tensors(1, 5120, seed=6))
    assert m.debug_grid() == 9
    _decodes_like_the_oracle(eng, oracle, m, "after the refusal of RWKV_GRID=9")       # (9 workgroups are enough for D = 80)
    m.close()


def test_load_file_streams_through_pinned_staging(eng, tmp_path):
    """rwkv_load_file (rwkv.cu:638-717): a model.bin read through two pinned staging buffers in 32 MiB pieces, no device wait
    per tensor -- the context must compute exactly what a context loaded from the same tensors in memory computes.  D = 2048,
    L = 3: the 4D x D matrices (16 MiB) and the embedding table (412 MB) span several pieces."""
    L, D = 3, 2048
    t = mf.synthetic_tensors(L, D, seed=77)
    path = str(tmp_path / "model.bin")
    mf.write_bin(path, L, D, [np.zeros(n, dtype=dt) if x is None else x for x, n, dt in zip(t, mf.sizes(L, D), mf.DTYPES)])
    a = eng.RWKV(resident=True); a.loadTensors(L, D, t)
    b = eng.RWKV(resident=True); b.loadFile(path)
    for tk in (3, 50000, 17, 17):
        la = np.array(a.forward(tk)[: mf.VOCAB]); lb = np.array(b.forward(tk)[: mf.VOCAB])
        assert np.array_equal(la, lb)
    a.close(); b.close()


@pytest.fixture(scope="module")
def fault_libs(built, tmp_path_factory):
    """a variant of the engine with a fault built in (the loader loses a group)"""
    import shutil
    import subprocess
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    src = os.path.join(ROOT, "rwkv-cpp-accelerated_amd", "csrc", "engine.hip")
    d = tmp_path_factory.mktemp("fault_libs")
    libs = {"drop": (str(d / "lib_drop.so"), "-DRWKV_TEST_DROP_GROUP=1")}
    procs = [subprocess.Popen([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-shared", "-Wno-unused-result", flag, src, "-o", lib])
             for lib, flag in libs.values()]
    for pr in procs:
        assert pr.wait(timeout=900) == 0
    return {k: v[0] for k, v in libs.items()}



@pytest.mark.parametrize("tile", ["15"])
def test_a_lost_ring_hand_off_fails_the_call_instead_of_returning_garbage(fault_libs, tile):
    """every wait of the tile-form kernels' LDS ring is bounded; one that gives up is recorded and reported (kernels.hip.h ring_report,
    engine.hip device_check): a variant of the engine whose loader wave never issues a workgroup's last pair of units
    (-DRWKV_TEST_DROP_GROUP=1, built here with hipcc) must fail the forward with RWKV_E_DEVICE, and the context must be usable
    for error reporting afterwards -- no hang, no silently wrong logits.  Runs in a subprocess (RWKV_LIB selects the variant) with
    the tile-form kernels a 4096-wide model gets by default."""
    import subprocess
    import sys
    lib = fault_libs["drop"]
    code = (
        "import sys, numpy as np\n"
        f"sys.path.insert(0, {ROOT!r})\n"
        "import torch\n"
        "from rwkv_cpp_accelerated_amd import engine, modelfile as mf\n"
        "L, D = 2, 4096\n"
        "m = engine.RWKV(resident=True); m.loadTensors(L, D, mf.synthetic_tensors(L, D, seed=5))\n"
        "try:\n"
        "    m.forward(7)\n"
        "    print('NOERROR')\n"
        "except engine.RWKVError as e:\n"
        "    print('RWKVERROR', str(e)[-120:], '|', str(e)[:120])\n"
    )
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, RWKV_LIB=lib, RWKV_TILE=tile), capture_output=True, text=True, timeout=600)
    assert "RWKVERROR" in out.stdout and "device-side wait gave up" in out.stdout and "status -3" in out.stdout, out.stdout[-400:] + out.stderr[-400:]


def test_a_retired_environment_variable_is_reported_not_silently_ignored(built, monkeypatch, capfd):
    """RWKV_RING selected the LDS-ring form of the row-form decode kernels, which is gone: a context created with it set still
    loads and decodes, and says on stderr that the variable is ignored (engine.hip RETIRED_ENV)."""
    monkeypatch.setenv("RWKV_RING", "13")
    import torch
    from rwkv_cpp_accelerated_amd import engine
    L, D = 1, 768
    m = engine.RWKV(resident=True)
    m.loadTensors(L, D, mf.synthetic_tensors(L, D, seed=3))
    assert np.isfinite(np.array(m.forward(7)[: mf.VOCAB])).all()
    m.close()
    assert "RWKV_RING is retired and ignored" in capfd.readouterr().err


@pytest.mark.parametrize("tile", ["0", "15"])
def test_two_contexts_decoding_at_once_are_independent(built, tile, monkeypatch):
    """two contexts of one process, a stream and a host thread each, greedy-decoding AT THE SAME TIME: their kernels interleave on the CUs
    (every kernel owns its CU's whole LDS for its lifetime and a tile-form kernel zeroes its ring's control block on entry): ids equal to
    the same decode run alone, no RWKV_E_DEVICE from a lost hand-off."""
    import threading
    monkeypatch.setenv("RWKV_TILE", tile)       # "0": the row-form register kernels; "15": the tile-form kernels a 4096-wide model gets by default
    import torch
    from rwkv_cpp_accelerated_amd import engine
    L, D, steps = 4, 4096, 96
    ms, alone = [], []
    for i in range(2):
        m = engine.RWKV(resident=True)
        m.loadTensors(L, D, mf.synthetic_tensors(L, D, seed=31 + i))
        ms.append(m)
    for i, m in enumerate(ms):
        alone.append(m.decode_greedy(5 + i, steps).copy())
    for rep in range(3):
        outs, errs = [None, None], []

        def run(i):
            try:
                outs[i] = ms[i].decode_greedy(5 + i, steps)
            except Exception as e:      # noqa: BLE001
                errs.append(repr(e))
        for m in ms:                    # same starting point as the run alone
            m.reset_state()
        th = [threading.Thread(target=run, args=(i,)) for i in range(2)]
        for x in th:
            x.start()
        for x in th:
            x.join()
        assert not errs, errs
        for i in range(2):
            assert np.array_equal(outs[i], alone[i]), (rep, i)
    for m in ms:
        m.close()
    torch.cuda.synchronize()


def test_tile_form_decode_is_the_row_form_bit_for_bit_on_one_weight_image(built, monkeypatch):
    """A 4096-wide model on 256 CUs decodes in TILE form by default (csrc/tile.hip.h: the four per-layer kernels stream the MFMA B-operand
    image the chunk path uses, v_mfma_i32_16x16x64_i8 on signed limbs, exact integer sums met in LDS) and holds ONLY that image of the per-layer
    matrices.  Every row value is the same exact integer as in row form (RWKV_TILE=0), so greedy ids AND logits must be identical, step
    after step -- also on a second state slot (PARRALEL mode through the token-by-token path, RWKV_SEQ=0) and on a context that owns a layer
    range (pipeline stage) -- and the resident bytes must be those of ONE copy of the matrices."""
    import torch
    from rwkv_cpp_accelerated_amd import engine
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("tile form is chosen where a workgroup owns one 16-channel block: D = 4096 on 256 CUs")
    L, D = 3, 4096
    t = mf.synthetic_tensors(L, D, seed=77)
    monkeypatch.setenv("RWKV_TILE", "0")
    row = engine.RWKV(resident=True); row.loadTensors(L, D, t, maxGPT=2)
    monkeypatch.delenv("RWKV_TILE")
    til = engine.RWKV(resident=True); til.loadTensors(L, D, t, maxGPT=2)
    weights = 13 * L * D * D + mf.VOCAB * D
    assert til.resident_bytes() < row.resident_bytes() - 0.9 * (weights - mf.VOCAB * D), (til.resident_bytes(), row.resident_bytes())
    tk = 9
    for step in range(12):
        a = row.forward(tk)[: mf.VOCAB].copy(); b = til.forward(tk)[: mf.VOCAB].copy()
        assert np.array_equal(a, b), step
        tk = parity.argmax_ban0(a)
    assert np.array_equal(row.decode_greedy(tk, 16), til.decode_greedy(tk, 16))
    row.close(); til.close()
    # two state slots, token by token (RWKV_SEQ=0 keeps PARRALEL mode on the decode kernels): slot 1's state offset in the tile epilogues
    monkeypatch.setenv("RWKV_SEQ", "0")
    outs = []
    for tile in ("0", None):
        if tile is None:
            monkeypatch.delenv("RWKV_TILE", raising=False)
        else:
            monkeypatch.setenv("RWKV_TILE", tile)
        m = engine.RWKV(resident=True); m.loadTensors(L, D, t, maxGPT=2)
        o = []
        for pair in ([5, 900], [17, 33], [2, 40000]):
            o.append(m.forward(pair, engine.MODE_PARRALEL)[: 2 * mf.VOCAB].copy())
        outs.append(o)
        m.close()
    for x, y in zip(*outs):
        assert np.array_equal(x, y)
    monkeypatch.delenv("RWKV_SEQ")
    # contexts that own a layer range (pipeline stages): the stages' kernels in tile form, chained on this one GPU
    from rwkv_cpp_accelerated_amd import pipeline
    st = []
    for tile in ("0", None):
        if tile is None:
            monkeypatch.delenv("RWKV_TILE", raising=False)
        else:
            monkeypatch.setenv("RWKV_TILE", tile)
        stages = [pipeline.EngineStage(t, L, D, l0, l1, n_slots=1) for l0, l1 in ((0, 1), (1, 3))]
        picks, tk = [], 21
        for step in range(6):
            for i, sg in enumerate(stages):
                if i > 0:
                    sg.x.copy_(stages[i - 1].x); torch.cuda.synchronize()
                nxt = sg.forward(tk, 0, want_pick=sg.last)
            tk = nxt
            picks.append(tk)
        st.append((picks, stages[-1].m.logits(1)[: mf.VOCAB].copy()))
        for sg in stages:
            sg.m.close()
    assert st[0][0] == st[1][0] and np.array_equal(st[0][1], st[1][1]), (st[0][0], st[1][0])


@pytest.mark.gpu
@pytest.mark.parametrize("D,default_mask", [(5120, 15), (2048, 13), (4096, 15)])
def test_each_decode_class_is_resident_in_the_one_layout_it_streams(built, monkeypatch, D, default_mask):
    """RWKV_TILE is a mask over the four per-layer decode classes (rwkv_decode_form).  A class in tile form streams 16-row tiles at
    4096 channels and 4-row tiles at 5120 / 2048 (five / two tiles per class and workgroup, csrc/tile.hip.h); its row form is not kept, a
    class in row form keeps no tile image unless the chunk path needs one: the resident bytes of a max_ctx = 1 context are ONE copy of
    the matrices whatever the mask.  Every mask gives the same logits bit for bit (the same exact integers reach the same epilogues), and
    the default is what was measured faster on this part: all four classes at 4096 and 5120, all but att_out at 2048."""
    import torch
    from rwkv_cpp_accelerated_amd import engine
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the tile forms are laid out for 256 workgroups")
    L = 2
    t = mf.synthetic_tensors(L, D, seed=5 + D)
    weights = 13 * L * D * D + mf.VOCAB * D
    ref, sizes = None, {}
    for mask in (0, None, 4, 9, 15):
        if mask is None:
            monkeypatch.delenv("RWKV_TILE", raising=False)
        else:
            monkeypatch.setenv("RWKV_TILE", str(mask))
        m = engine.RWKV(resident=True); m.loadTensors(L, D, t, maxGPT=1)
        assert m.decode_form() == (default_mask if mask is None else mask)
        sizes[mask] = m.resident_bytes()
        out, tk = [], 11
        for step in range(6):
            a = m.forward(tk)[: mf.VOCAB].copy()
            out.append(a); tk = parity.argmax_ban0(a)
        out.append(m.decode_greedy(tk, 8))
        m.close()
        if ref is None:
            ref = out
        else:
            for x, y in zip(ref, out):
                assert np.array_equal(x, y), mask
    for mask, b in sizes.items():
        assert abs(b - sizes[0]) < 0.02 * weights, sizes


@pytest.mark.gpu
@pytest.mark.parametrize("D,default_mask", [(2048, 13), (4096, 15)])
def test_the_load_keeps_the_images_both_paths_need_whatever_the_mask(built, monkeypatch, D, default_mask):
    """With max_ctx > 1 the chunk path's 16-row tile image of every class is resident beside whatever the decode kernels stream, so the
    load has three cases per class: row form + image (class in row form), the image alone (tile form at 4096, where the decode kernels
    stream the chunk path's image), image + a decode-only image of 4-row tiles (tile form at 2048).  Whatever the mask, six greedy
    forward steps, decode_greedy and a 5-token GPT-mode call give the same bits, and the resident bytes are what the layouts say: at
    4096 a class in tile form drops its row form -- L D^2 Q bytes, Q = 3, 1, 5, 4 for K/V/R, att_out, ffn k/r, ffn_v -- and nothing
    else changes; at 2048 a 4-row image replaces a row form of the same size.  (max_ctx is 5, not 2: the smallest context that holds the
    5-token call; the byte counts asserted do not depend on it.)"""
    import torch
    from rwkv_cpp_accelerated_amd import engine
    if torch.cuda.get_device_properties(0).multi_processor_count != 256:
        pytest.skip("the tile forms are laid out for 256 workgroups")
    L, Q = 2, (3, 1, 5, 4)
    t = mf.synthetic_tensors(L, D, seed=9 + D)
    ref, sizes = None, {}
    for mask in (0, 5, None):
        if mask is None:
            monkeypatch.delenv("RWKV_TILE", raising=False)
        else:
            monkeypatch.setenv("RWKV_TILE", str(mask))
        m = engine.RWKV(resident=True); m.loadTensors(L, D, t, maxGPT=5)
        mask = default_mask if mask is None else mask
        assert m.decode_form() == mask
        sizes[mask] = m.resident_bytes()
        out, tk = [], 11
        for step in range(6):
            a = m.forward(tk)[: mf.VOCAB].copy()
            out.append(a); tk = parity.argmax_ban0(a)
        out.append(m.decode_greedy(tk, 8))
        out.append(m.forward([7, 50000, 11, 4242, 3], engine.MODE_GPT)[: 5 * mf.VOCAB].copy())
        m.close()
        if ref is None:
            ref = out
        else:
            for x, y in zip(ref, out):
                assert np.array_equal(x, y), mask
    for mask, b in sizes.items():
        print(f"D {D} mask {mask}: resident bytes {b} (row form - this: {sizes[0] - b})")
        dropped = L * D * D * sum(q for k, q in enumerate(Q) if mask >> k & 1) if D == 4096 else 0
        assert sizes[0] - b == dropped, sizes
