"""Constrained decoding, as far as a box without a GPU can check it: the entry points are declared, exported and bound (ctypes, pybind, C++),
tests/cpp/constrain_app.cpp compiles and links, and the HOST TWINS of include/rwkv_sampler.h -- constrained_row, constraint_next, constraint_trie and
the one validator constraint_check, reached through the pybind module -- are held to the numpy restatement of tests/constraint_cases.py, bit for
bit.  The same inputs run once through a stand-alone host program built with -fsanitize=address,undefined (its own main, no Python, nothing
preloaded).  (rwkv_create needs a device, so the status codes of a context are checked by the GPU suite; a NULL context is checked here.)"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import constraint_cases as cc

from support import CSRC, E_ARG, ROOT, build_app, rwkv_mod, same_bits  # noqa: F401

V = cc.V


def test_entry_points_are_declared_exported_and_bound(built):
    from rwkv_cpp_accelerated_amd import engine
    hdr = open(os.path.join(ROOT, "include", "rwkv_mi355x.h")).read()
    lib = engine.lib()
    for s, nargs in (("rwkv_constraint_set", 2), ("rwkv_constraint_clear", 1), ("rwkv_constraint_state_set", 4), ("rwkv_constraint_state_get", 4),
                     ("rwkv_pick_constrained", 9), ("rwkv_debug_constrained_row", 3), ("rwkv_decode_batch_constrained", 13)):
        assert s + "(" in hdr and s in engine.ABI_SYMBOLS and hasattr(lib, s), s
        assert len(getattr(lib, s).argtypes) == nargs
    assert "#define RWKV_CONSTRAINT_MAX_STATES 4096u" in hdr and engine.CONSTRAINT_MAX_STATES == 4096
    assert "#define RWKV_CONSTRAINT_MAX_EDGES (1u << 24)" in hdr and engine.CONSTRAINT_MAX_EDGES == 1 << 24
    assert "#define RWKV_CONSTRAINT_MAX_BIAS 300u" in hdr and engine.CONSTRAINT_MAX_BIAS == 300
    assert "#define RWKV_STOP_CONSTRAINT 32u" in hdr and engine.STOP_CONSTRAINT == 32
    assert C.sizeof(engine.Automaton) == 40 and C.sizeof(engine.Bias) == 24 and C.sizeof(engine.ConstrainParams) == 48
    for f in ("constraint_set", "constraint_clear", "constraint_state_get", "constraint_state_set", "pick_constrained", "decode_batch_constrained"):
        assert callable(getattr(engine.RWKV, f, None)), f
    assert callable(engine.constraint_trie)
    cpp = open(os.path.join(ROOT, "include", "rwkv.h")).read()
    for f in ("setConstraint(", "clearConstraint(", "decodeConstrained(", "pickConstrained("):
        assert f in cpp, f
    twins = open(os.path.join(ROOT, "include", "rwkv_sampler.h")).read()
    for f in ("constrained_row(", "constraint_next(", "constraint_check(", "constraint_trie("):
        assert f in twins, f
    for out in ("beam search under a constraint", "typical sampling under a constraint", "log-probs under the constrained distribution",
                "compiling a grammar or regex", "applying the mask inside the pick kernels"):
        assert out in " ".join(hdr.replace(" * ", " ").split()), out                        # the header says what is out of scope
    src = open(os.path.join(CSRC, "constrain.hip.h")).read()
    assert "constexpr unsigned CN_WORDS" in src and cc.kernel_constants()[0] >= 1


def test_a_null_context_is_a_bad_argument(built):
    from rwkv_cpp_accelerated_amd import engine
    lib = engine.lib()
    u32 = (C.c_uint32 * 4)()
    a = engine.Automaton(1, 0, 0, u32, None, None)
    assert lib.rwkv_constraint_set(None, C.byref(a)) == E_ARG and lib.rwkv_constraint_clear(None) == E_ARG
    assert lib.rwkv_constraint_state_set(None, 0, 1, u32) == E_ARG and lib.rwkv_constraint_state_get(None, 0, 1, u32) == E_ARG
    pk = engine.Pick(engine.PICK_GREEDY, 1.0, 0.8, 0, engine.nucleus_params())
    tok = C.c_uint64(0)
    assert lib.rwkv_pick_constrained(None, 0, 0, C.byref(pk), None, 0.5, 1, C.byref(tok), None) == E_ARG
    assert lib.rwkv_debug_constrained_row(None, 0, None) == E_ARG
    cp = engine.ConstrainParams(None, None, None, None, None, 0)
    out, ln = (C.c_uint64 * 4)(), (C.c_uint32 * 2)()
    assert lib.rwkv_decode_batch_constrained(None, out, 1, 2, C.byref(pk), None, C.byref(cp), None, None, out, ln, None, None) == E_ARG


def test_pybind_module_has_the_constraint_functions(rwkv_mod):
    for f in ("setConstraint", "clearConstraint", "decodeConstrained", "constraintCheck", "constrainedRow", "constraintNext", "constraintTrie"):
        assert callable(getattr(rwkv_mod, f, None)), f


def test_constrain_app_compiles_and_links(built, tmp_path):
    app = build_app("constrain_app", tmp_path)
    syms = subprocess.run(["nm", "-D", "--undefined-only", app], capture_output=True, text=True).stdout
    assert "rwkv_constraint_set" in syms and "rwkv_decode_batch_constrained" in syms and "rwkv_pick_constrained" in syms


# ---- the twins against numpy ----------------------------------------------------------------------------------------------------
BIASES = [None, {}, {1: 2.5, V - 1: -1.25}, {31: -np.inf, 33: 7.0}, {100: 1000.0}, {i: (-1) ** i * 0.5 * i for i in range(1, 601, 2)}]


@pytest.mark.parametrize("name", list(cc.PLANTED_STATES))
def test_constrained_row_is_numpy_where_bit_for_bit(rwkv_mod, name):
    a, q = cc.planted_automaton(), cc.PLANTED_STATES[name]
    m = cc.allowed_mask(a, q)
    assert not m[0] and m.sum() == a[0][q + 1] - a[0][q]
    for r, bias in enumerate(BIASES):
        l = cc.planted_row(m, r)
        want = cc.constrained(l, m, bias)
        kw = {} if bias is None else dict(zip(("bias_tok", "bias_val"), _arrays(bias)))
        got = np.asarray(rwkv_mod.constrainedRow(l, a[0], a[1], a[2], q, **kw))
        assert got.dtype == np.float32 and same_bits(got, want), (name, r)
        assert np.isneginf(got[~m]).all() and np.isneginf(got[0])
        assert np.signbit(want[m][want[m] == 0]).sum() == 0                                 # -0.0 + 0 is +0.0: the add is made
        live = m.copy()
        for t, v in (bias or {}).items():
            if np.isneginf(v):
                live[t] = False
        assert np.isfinite(got[live]).all() and cc.argmax_low(got) in np.flatnonzero(live)


def _arrays(bias):
    ids = sorted(bias)
    return np.array(ids, np.uint32), np.array([bias[i] for i in ids], np.float32)


def test_the_implicit_state_and_a_terminal_state_allow_everything_but_id_0(rwkv_mod):
    l = (np.random.default_rng(3).standard_normal(V) * 2).astype(np.float32)
    m = np.ones(V, bool); m[0] = False
    want = cc.constrained(l, m, {7: -np.inf})
    assert same_bits(np.asarray(rwkv_mod.constrainedRow(l, bias_tok=np.array([7], np.uint32), bias_val=np.array([-np.inf], np.float32))), want)
    rp, tk, nx = cc.csr([[(5, 1)], []])                                                     # state 1 is terminal
    assert same_bits(np.asarray(rwkv_mod.constrainedRow(l, rp, tk, nx, 1)), cc.constrained(l, m))
    assert same_bits(cc.allowed_mask((rp, tk, nx), 1), m)
    w = cc.mask_words(m)
    assert w[0] == 0xFFFFFFFE and w[-1] == 0x1F and (w[1:-1] == 0xFFFFFFFF).all() and w.size == 1572


def test_constraint_next_on_first_last_and_only_edges(rwkv_mod):
    a = cc.planted_automaton()
    nxt = lambda q, g: int(rwkv_mod.constraintNext(a[0], a[1], a[2], q, g))
    assert nxt(cc.P_ONE, 1) == 1                                                            # the only edge of a row
    assert [nxt(cc.P_TRIPLE, g) for g in (31, 32, 33)] == [3, 4, 5]                         # first, middle, last edge
    assert [nxt(cc.P_TRIPLE2, g) for g in (31, 32, 33)] == [6, 0, 1]                        # the adjacent row: the same ids, another next
    assert nxt(cc.P_TAIL, 50272) == 0 and nxt(cc.P_TAIL, V - 1) == 0 and nxt(cc.P_LAST, V - 1) == 2
    assert nxt(cc.P_ALL, 1) == 1 and nxt(cc.P_ALL, V - 1) == (V - 1) % 6
    assert nxt(cc.P_TRIPLE, 30) == cc.P_TRIPLE and nxt(cc.P_TRIPLE, 34) == cc.P_TRIPLE and nxt(cc.P_ONE, 2) == cc.P_ONE   # no edge: the state stays
    rng = np.random.default_rng(1)
    la = cc.loop_automaton()
    for q in range(6):
        row = la[1][la[0][q]:la[0][q + 1]]
        for g in [int(row[0]), int(row[-1])] + [int(v) for v in rng.choice(row, 3)]:
            assert int(rwkv_mod.constraintNext(la[0], la[1], la[2], q, g)) == cc.next_state(la, q, g)


def test_constraint_trie_accepts_exactly_the_given_sequences(rwkv_mod):
    """Accepting means: the sequence leads from state 0 to a state WITHOUT edges, where the stream ends.  Shared prefixes are merged.  A choice that
    is a proper prefix of another one ends in a state that has edges, so it is NOT accepted as an end: a stream on it goes on to an extension."""
    from rwkv_cpp_accelerated_amd import engine
    got = tuple(np.asarray(x) for x in rwkv_mod.constraintTrie(cc.CHOICES))
    py = engine.constraint_trie(cc.CHOICES)
    for g, p in zip(got, py):
        assert g.dtype == np.uint32 and same_bits(g, p)
    row_ptr, tok, nxt = got
    assert rwkv_mod.constraintCheck(len(row_ptr) - 1, row_ptr, tok, nxt) is None
    # states: root, 100, 200*, 201, 300*, 301*, 5000, 6000, 7000, 8000* -- the prefix 100 (and 100 201) is shared
    assert len(row_ptr) - 1 == 10 and tok[row_ptr[0]:row_ptr[1]].tolist() == [100, 5000]
    for ch in cc.CHOICES:
        assert cc.trie_accepts(got, ch), ch
    for bad in ([100], [100, 201], [100, 200, 300], [200], [5000, 6000, 7000], [100, 201, 302], [5000, 6000, 7000, 8000, 1]):
        assert not cc.trie_accepts(got, bad), bad
    leaves = [q for q in range(10) if row_ptr[q] == row_ptr[q + 1]]
    assert len(leaves) == 4
    # one choice is a prefix of another: the shorter one is a path, not an end; the longer one is accepted; skipped: empty choices, id 0, id >= V
    pre = tuple(np.asarray(x) for x in rwkv_mod.constraintTrie([[7, 8], [7, 8, 9], [], [0, 5], [V]]))
    assert len(pre[0]) - 1 == 4 and not cc.trie_accepts(pre, [7, 8]) and cc.trie_accepts(pre, [7, 8, 9])
    for g, p in zip(pre, engine.constraint_trie([[7, 8], [7, 8, 9], [], [0, 5], [V]])):
        assert same_bits(g, p)
    assert rwkv_mod.constraintCheck(4, *pre) is None


@pytest.mark.parametrize("i", range(len(cc.malformed())))
def test_constraint_check_rejects_each_malformed_input_by_name(rwkv_mod, i):
    rule, kw = cc.malformed()[i]
    assert rwkv_mod.constraintCheck(**kw) == rule


def test_constraint_check_accepts_the_well_formed(rwkv_mod):
    for kw in cc.well_formed():
        assert rwkv_mod.constraintCheck(**kw) is None


# ---- the same inputs under the host sanitizers ------------------------------------------------------------------------------------
SAN_MAIN = r'''
#include <cstdio>
#include <cstring>
#include <string>
#include "rwkv_sampler.h"
// reads "case" records from stdin: name, S (or -1), row_ptr, tok, next, bias tok, bias val (hex floats), expected rule ("-": well formed)
static std::vector<unsigned> read_u(FILE *f) { unsigned n = 0; fscanf(f, "%u", &n); std::vector<unsigned> v(n); for (auto &x : v) fscanf(f, "%u", &x); return v; }
static std::vector<float> read_f(FILE *f) { unsigned n = 0; fscanf(f, "%u", &n); std::vector<float> v(n); for (auto &x : v) { char b[64]; fscanf(f, "%63s", b); x = strtof(b, nullptr); } return v; }
int main()
{
    int bad = 0, n = 0;
    long long S;
    while (fscanf(stdin, "%lld", &S) == 1) {
        const std::vector<unsigned> rp = read_u(stdin), tk = read_u(stdin), nx = read_u(stdin), bt = read_u(stdin);
        const std::vector<float> bv = read_f(stdin);
        char want[64]; int has_b = 0;
        fscanf(stdin, "%d %63s", &has_b, want);
        const constraint_view a{(unsigned long long)S, rp.data(), tk.size(), tk.data(), nx.data()};
        const bias_view b{bt.size(), bt.data(), bv.data()};
        const char *rule = constraint_check(S >= 0 ? &a : nullptr, has_b ? &b : nullptr);
        if (std::string(rule ? rule : "-") != want) { printf("case %d: %s, expected %s\n", n, rule ? rule : "-", want); bad++; }
        if (!rule && S >= 0) {       // a well-formed automaton: every state's row, with the bias when there is one, and the advance along every edge of it
            std::vector<float> l(50277), c(50277);
            for (int i = 0; i < 50277; i++) l[i] = (float)((i * 2654435761u) % 1000) * 0.01f - 5.0f;
            for (unsigned q = 0; q < (unsigned)S && q < 8; q++) {
                constrained_row(l.data(), &a, q, has_b ? &b : nullptr, c.data());
                if (c[0] != -INFINITY) bad++;
                for (unsigned e = rp[q]; e < rp[q + 1]; e += 1 + (rp[q + 1] - rp[q]) / 16) if (constraint_next(&a, q, tk[e]) != nx[e]) bad++;
            }
        }
        n++;
    }
    const constraint_automaton t = constraint_trie({{100, 200}, {100, 201, 300}, {100, 201, 301}, {5000, 6000, 7000, 8000}, {}, {0}, {7, 8}, {7, 8, 9}});
    const constraint_view tv{t.states(), t.row_ptr.data(), t.tok.size(), t.tok.data(), t.next.data()};
    if (constraint_check(&tv, nullptr) || t.states() != 13) bad++;
    printf("%d cases, %d bad\n", n, bad);
    return bad ? 1 : 0;
}
'''


def test_the_host_code_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program (its own main, no Python, nothing preloaded) runs every malformed and well-formed input of this suite through
    constraint_check, and the well-formed automata through constrained_row, constraint_next and constraint_trie"""
    src, exe = tmp_path / "san.cpp", tmp_path / "san"
    src.write_text(SAN_MAIN)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I" + os.path.join(ROOT, "include"), str(src), "-o", str(exe)])
    lines = []
    arr = lambda v, fmt=str: " ".join([str(len(v))] + [fmt(x) for x in v])
    cases = [(rule, kw) for rule, kw in cc.malformed()] + [("-", kw) for kw in cc.well_formed()]
    for rule, kw in cases:
        S = kw.get("S", -1)
        rp = kw.get("row_ptr", np.zeros(0, np.uint32))
        if S >= 0 and len(rp) != S + 1 and 0 < S <= 4096:
            continue
        bt, bv = kw.get("bias_tok"), kw.get("bias_val")
        lines.append(" ".join([str(S), arr(rp), arr(kw.get("tok", [])), arr(kw.get("next", [])), arr(bt if bt is not None else []),
                               arr(bv if bv is not None else [], lambda x: float(x).hex() if np.isfinite(x) else str(float(x))),
                               "1" if bt is not None else "0", rule]))
    out = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=120)
    print(out.stdout[-400:], out.stderr[-2000:])
    assert out.returncode == 0 and out.stdout.strip().endswith(f"{len(lines)} cases, 0 bad") and "runtime error" not in out.stderr
