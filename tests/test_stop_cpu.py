"""Stop sequences and budgets, as far as a box without a GPU can check them: the C++ twin stop_scan (include/rwkv_sampler.h) agrees exactly
with the Python restatement (tests/stop_cases.py) on the planted strings and on 200 random ones; the new symbols are declared, exported and
bound and the structs have the header's layout; NULL arguments are RWKV_E_ARG.  (rwkv_create needs a device, so the RWKV_E_STATE of an
unloaded context is checked by tests/test_stop_gpu.py.)"""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import stop_cases as sc

from support import E_ARG, ROOT, build_app, rwkv_mod, syntax_only  # noqa: F401

NEW = ("rwkv_decode_batch_until", "rwkv_debug_stop_scan")


@pytest.fixture(scope="module")
def scan_app(tmp_path_factory):
    return build_app("stop_scan_app", tmp_path_factory.mktemp("cpp"), link=False, extra=("-Wall",))


def run_twin(exe, path, cases):
    """cases: (first, ids, stops, max_new, history) -> [(len, reason, history)] of the C++ twin"""
    with open(path, "w") as f:
        for first, ids, stops, max_new, history in cases:
            h = [] if history is None else list(history)
            rec = [first, max_new or 0, len(h), *h, len(ids), *ids, len(stops)]
            for q in stops:
                rec += [len(q), *q]
            f.write(" ".join(str(int(v)) for v in rec) + "\n")
    out = subprocess.run([exe, path], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0, out.stderr
    rows = [[int(v) for v in l.split()] for l in out.stdout.splitlines()]
    assert len(rows) == len(cases)
    return [(r[0], r[1], r[3:3 + r[2]]) for r in rows]


def check(exe, path, cases):
    got = run_twin(exe, path, cases)
    for g, (first, ids, stops, max_new, history) in zip(got, cases):
        assert g == sc.stop_scan(ids, first, stops, max_new, history), (first, ids, stops, max_new, history)


def test_twin_agrees_on_the_planted_strings(scan_app, tmp_path):
    cases = [(first, ids, call["stops"], max_new, None) for call in sc.PLANTED.values() for first, ids, max_new in call["streams"]]
    ids, firsts, stops, max_new = sc.many_streams()
    cases += [(int(firsts[s]), [int(v) for v in ids[s]], stops, max_new[s], None) for s in range(len(ids))]
    check(scan_app, str(tmp_path / "planted.txt"), cases)


def test_twin_agrees_on_200_random_strings(scan_app, tmp_path):
    rng = np.random.default_rng(2024)
    cases = [sc.random_case(rng) for _ in range(200)]
    assert sum(sc.stop_scan(i, f, s, m, h)[1] >= 2 for f, i, s, m, h in cases) >= 50       # matches are frequent
    check(scan_app, str(tmp_path / "random.txt"), cases)


def test_twin_continues_a_history_across_a_split(scan_app, tmp_path):
    firsts, ids = sc.keep_streams()
    for s in range(len(ids)):
        full = sc.stop_scan(ids[s], firsts[s], [sc.KEEP_SEQ])
        a = run_twin(scan_app, str(tmp_path / "a.txt"), [(firsts[s], list(ids[s][:12]), [sc.KEEP_SEQ], None, None)])[0]
        assert a[:2] == (12, 0)
        b = run_twin(scan_app, str(tmp_path / "b.txt"), [(int(ids[s][11]), list(ids[s][12:]), [sc.KEEP_SEQ], None, a[2])])[0]
        assert (12 + b[0], b[1]) == full[:2] and full[1] == 2 and b[2] == full[2]


def test_the_planted_strings_hold_what_they_claim():
    r = {k: [sc.stop_scan(ids, first, call["stops"], mx)[:2] for first, ids, mx in call["streams"]] for k, call in sc.PLANTED.items()}
    assert r["self_overlap"] == [(2, 2), (1, 2), (6, 2)]
    assert r["suffix_of_another"] == [(4, 2), (4, 3), (2, 2)]
    assert r["suffix_listed_first"] == [(4, 2), (2, 4)]
    assert r["last_step"] == [(sc.STEPS, 2), (sc.STEPS, 3), (sc.STEPS, 0)]
    assert r["first_token"] == [(1, 2), (sc.STEPS, 0), (2, 2)]
    assert r["len_1_and_8"] == [(6, 3), (1, 3), (sc.STEPS, 0)] and r["len_8_alone"] == [(10, 2), (7, 2), (16, 2), (12, 2)]
    assert r["ids_1_and_50276"] == [(1, 4), (3, 2), (2, 2), (5, 4)]
    assert r["budget_1"] == [(1, 1), (1, 2), (3, 2), (2, 1), (sc.STEPS, 0), (sc.STEPS - 1, 1)]
    assert r["budget_only"] == [(1 + s % 5, 1) for s in range(7)]
    assert r["sixteen"] == [(j + 1 + 1 + j % 8, 2 + j) for j in range(16)]
    assert sc.bound(12, 4096) == 24 and sc.bound(1, 4096) == 16 and sc.bound(9, 16) == 16 and sc.bound(8, 4096) == 16


def test_symbols_structs_and_constants_agree(built):
    from rwkv_cpp_accelerated_amd import engine
    with open(os.path.join(ROOT, "include", "rwkv_mi355x.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(rwkv_[a-z0-9_]+)\s*\(", hdr))
    lib = engine.lib()
    assert set(NEW) <= declared and set(NEW) <= set(engine.ABI_SYMBOLS) and all(hasattr(lib, s) for s in NEW)
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert set(NEW) <= {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert C.sizeof(engine.Pick) == 48 and C.sizeof(engine.StopParams) == 40
    assert [n for n, _ in engine.Pick._fields_] == ["kind", "temp", "tau", "typical_flags", "nucleus"]
    assert [n for n, _ in engine.StopParams._fields_] == ["seq_ids", "seq_len", "n_seqs", "flags", "max_new", "reserved"]
    assert (engine.Pick.nucleus.offset, engine.StopParams.max_new.offset, engine.StopParams.reserved.offset) == (16, 24, 32)
    for name, val in (("MAX_SEQS", 16), ("MAX_LEN", 8), ("POLL", 8), ("KEEP", 1)):
        assert re.search(rf"#define RWKV_STOP_{name} {val}u\b", hdr) and getattr(engine, "STOP_" + name) == val
    assert (sc.MAX_SEQS, sc.MAX_LEN, sc.POLL) == (engine.STOP_MAX_SEQS, engine.STOP_MAX_LEN, engine.STOP_POLL)
    assert re.search(r"RWKV_PICK_GREEDY = 0, RWKV_PICK_TYPICAL = 1, RWKV_PICK_NUCLEUS = 2", hdr)
    assert (engine.PICK_GREEDY, engine.PICK_TYPICAL, engine.PICK_NUCLEUS) == (0, 1, 2)
    assert re.search(r"#define RWKV_MI355X_ABI_VERSION 6\b", hdr) and lib.rwkv_abi_version() == 6       # additions alone do not bump it
    for f in ("decode_batch_until", "debug_stop_scan"):
        assert callable(getattr(engine.RWKV, f, None)), f


def test_null_arguments_are_bad_arguments(built):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    one, ln = (C.c_uint64 * 1)(1), (C.c_uint32 * 1)()
    pk = engine.Pick(engine.PICK_GREEDY, 1.0, 0.8, 0, engine.nucleus_params())
    sp, _alive = engine.stop_params([[5]])
    assert lib.rwkv_decode_batch_until(None, one, 1, 1, C.byref(pk), None, C.byref(sp), one, ln, None, None) == E_ARG
    assert lib.rwkv_debug_stop_scan(None, one, one, 1, 1, C.byref(sp), ln, ln) == E_ARG


def test_cpp_header_and_pybind_offer_the_wrappers(rwkv_mod, tmp_path):
    src = tmp_path / "use_until.cpp"
    src.write_text('#include "rwkv.h"\n'
                   "unsigned use(RWKV &m) {\n"
                   "    RWKV::Stop stop; stop.sequences = {{187, 187}}; stop.max_new = {40, 60};\n"
                   "    RWKV::Until r = m.decodeBatchUntil({1, 2}, 64, RWKV::Pick::nucleus(RWKV::Nucleus{}), {7, 8}, stop);\n"
                   "    r = m.decodeBatchUntil({1, 2}, 64, RWKV::Pick::greedy(), {}, stop);\n"
                   "    r = m.decodeBatchUntil({1, 2}, 64, RWKV::Pick::typical(0.9f, 0.8f), {7, 8}, stop);\n"
                   "    std::vector<unsigned long long> h;\n"
                   "    return r.len[0] + r.reason[1] + (unsigned)r.steps_run + stop_scan({1, 2}, 3, stop.sequences, 0, h).len;\n"
                   "}\n")
    syntax_only(src)
    assert callable(getattr(rwkv_mod, "decodeUntil", None))
