"""What the feature suites share, written once: paths and status codes, the `eng` / `rwkv_mod` fixtures, contexts and their state (load,
start_state, snapshot / restore, rows, slots, plant_rows), the test programs of tests/cpp (build_app, run_app, headers_compile, model_file)
and the harness of the refused-call tables (GuardContexts, check_refused).  A plain module, imported like sampler_cases: a suite takes the
fixtures by name (`from support import eng, rwkv_mod`).  TEST INFRASTRUCTURE: nothing here is imported by the product."""
import ctypes as C
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import sampler_cases

from rwkv_cpp_accelerated_amd import modelfile as mf

# ---- paths and statuses -----------------------------------------------------------------------------------------------------------
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rwkv-cpp-accelerated_amd", "csrc")
INCLUDE = os.path.join(ROOT, "include")
V = mf.VOCAB
NAMES = "xy aa bb pp dd".split()                 # the five state arrays, in the order of RWKV.state.arrays()


def _statuses():
    """enum rwkv_status of include/rwkv_mi355x.h"""
    with open(os.path.join(INCLUDE, "rwkv_mi355x.h")) as f:
        body = re.search(r"enum rwkv_status \{(.*?)\};", f.read(), re.S).group(1)
    return {k: int(v) for k, v in re.findall(r"RWKV_(\w+) = (-?\d+)", body)}


E_ARG, E_IO, E_DEVICE, E_STATE = (_statuses()[k] for k in ("E_ARG", "E_IO", "E_DEVICE", "E_STATE"))


# ---- fixtures ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def eng(built):
    import torch
    assert torch.cuda.is_available(), "these tests need the GPU box"
    from rwkv_cpp_accelerated_amd import engine
    engine.lib()
    return engine


@pytest.fixture(scope="module")
def rwkv_mod(built):
    """the pybind module `rwkv` (csrc/pybind_module.cpp)"""
    assert built["pybind"], "pybind module not built"
    if CSRC not in sys.path:
        sys.path.insert(0, CSRC)
    import rwkv
    return rwkv


# ---- contexts and state -----------------------------------------------------------------------------------------------------------
def load(eng, L, D, seed, max_ctx, tensors=None, **synthetic_kw):
    """a resident context on the synthetic model of `seed` (or on `tensors`)"""
    m = eng.RWKV(resident=True)
    m.loadTensors(L, D, mf.synthetic_tensors(L, D, seed=seed, **synthetic_kw) if tensors is None else tensors, maxGPT=max_ctx)
    return m


def snapshot(m, n):
    """the five state arrays of slots 0 .. n - 1 as bit patterns: uint64 [n][L D]"""
    m.pull_state(n)
    per = m.num_layers * m.num_embed
    return [a[: n * per].copy().view(np.uint64).reshape(n, per) for a in m.state.arrays()]


def restore(m, snap):
    """a snapshot back onto the slots it was taken from"""
    n = len(snap[0])
    for a, s in zip(m.state.arrays(), snap):
        a[: s.size] = s.view(np.float64).reshape(-1)
    m.push_state(n)


def start_state(eng, m, n):
    """distinct state in slots 0 .. n - 1 (three PARRALEL steps of different tokens); returns its snapshot"""
    m.reset_state()
    rng = np.random.default_rng(5)
    for _ in range(3):
        m.forward([int(v) for v in rng.integers(1, V, n)], eng.MODE_PARRALEL)
    return snapshot(m, n)


def rows(m, n):
    """logits rows 0 .. n - 1 as bit patterns: uint32 [n][V]"""
    return m.logits(n).copy().view(np.uint32).reshape(n, V)


def slots(m, n, counts):
    """what a decode loop leaves per slot: the five state arrays [n][L D], the logits rows [n][V] and (counts) the count vectors [n][V]"""
    m.pull_state(n)
    per = m.num_layers * m.num_embed
    out = [a[: n * per].reshape(n, per).copy() for a in m.state.arrays()]
    out.append(m.logits(n).reshape(n, V).copy())
    if counts:
        out.append(np.stack([m.penalty_get(s) for s in range(n)]))
    return out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8))


def same_state(got, want, what, slots=slice(None)):
    """two snapshots agree bit for bit on `slots`"""
    for name, g, w in zip(NAMES, got, want):
        assert np.array_equal(g[slots], w[slots]), f"{what}: {name}"


def firsts_of(n):
    return [int(v) for v in np.random.default_rng(3).integers(1, V, n)]


def seeds_of(n):
    return [1000 + 7 * s for s in range(n)]


def plant_rows(m, rows, n_rows):
    """rows: {logits row: f32 [V]}, copied into the device logits buffer of a context with n_rows rows"""
    import torch
    view = sampler_cases.logits_view(m, n_rows)
    for r, vec in rows.items():
        view[r].copy_(torch.from_numpy(np.array(vec, np.float32)).cuda())          # (a copy: the cases are read-only)
    torch.cuda.synchronize()


# ---- apps and bindings ------------------------------------------------------------------------------------------------------------
LINK = ["-L" + CSRC, "-lrwkv_mi355x", "-Wl,-rpath," + CSRC]          # against the engine library, found again at run time


def build_app(name, outdir, link=True, opt="-O1", extra=()):
    """tests/cpp/<name>.cpp against include/ and (link) the engine library: no GPU needed to compile and link; returns the executable"""
    exe = os.path.join(str(outdir), name)
    subprocess.check_call(["g++", "-std=c++17", opt, *extra, os.path.join(ROOT, "tests", "cpp", name + ".cpp"), "-I" + INCLUDE,
                           *(LINK if link else []), "-o", exe])
    return exe


def run_app(exe, args, timeout=120):
    """(returncode, the lines it printed without the n_layers / n_embed banner of the loader, everything it printed)"""
    out = subprocess.run([exe, *[str(a) for a in args]], capture_output=True, text=True, timeout=timeout)
    lines = [l for l in out.stdout.splitlines() if l.strip() and not l.startswith(("n_layers", "n_embed"))]
    return out.returncode, lines, out.stdout + out.stderr


def syntax_only(src, cc="g++", std="-std=c++17", extra=("-Wall",)):
    """`src` compiles against include/ (nothing is emitted)"""
    out = subprocess.run([cc, std, "-fsyntax-only", *extra, "-I" + INCLUDE, str(src)], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-3000:]


def headers_compile(tmp_path):
    """the C header as C11 and C++17, the C++ header as C++17"""
    for hdr, std, cc in (("rwkv_mi355x.h", "-std=c11", "gcc"), ("rwkv_mi355x.h", "-std=c++17", "g++"), ("rwkv.h", "-std=c++17", "g++")):
        src = tmp_path / ("t.c" if cc == "gcc" else "t.cpp")
        src.write_text(f'#include "{hdr}"\nint main(void) {{ return 0; }}\n')
        syntax_only(src, cc, std)


def model_file(tmp_path_factory, tag, L, D, seed, **kw):
    """a synthetic model written as a model file; returns its path"""
    p = str(tmp_path_factory.mktemp(tag) / "model.bin")
    mf.write_bin(p, L, D, mf.synthetic_tensors(L, D, seed=seed, **kw))
    return p


# ---- refused calls ----------------------------------------------------------------------------------------------------------------
class GuardContexts:
    """The contexts that a table of refused calls names, all on the synthetic L x D model of seed 4100: "M" a loaded whole model with a
    history on slots 0 .. 4 and three logits rows, "U" created but never loaded, "S" a stage context (layers [0, 1)); of `extra`, "P" a whole
    model with a one-rank pipeline transport (max_ctx 32) and "W" a whole model of width 80, which has no chunk path.  `counts`: the count
    vector to plant on each slot of M; with them a snapshot covers the counts too, and check_refused holds resident_bytes as well."""
    FIRST, N = 11, 4

    def __init__(self, eng, L, D, max_ctx, extra=(), counts=None):
        self.lib, self.max_ctx, self.per, self.with_counts = eng.lib(), max_ctx, L * D, counts is not None
        t = mf.synthetic_tensors(L, D, seed=4100)
        self.models = {k: eng.RWKV(resident=True) for k in ("M", "U", "S") + tuple(extra)}
        self.models["M"].loadTensors(L, D, t, maxGPT=max_ctx)
        self.models["S"].set_layer_range(0, 1)
        self.models["S"].loadTensors(L, D, t, maxGPT=max_ctx)
        if "P" in extra:
            self.models["P"].loadTensors(L, D, t, maxGPT=32)
            self.models["P"].pipe_init(eng.RWKV.pipe_unique_id(), 0, 1)
        if "W" in extra:
            self.models["W"].loadTensors(L, 80, mf.synthetic_tensors(L, 80, seed=4100), maxGPT=max_ctx)
        self.h = {k: m._h for k, m in self.models.items()}
        m = self.models["M"]
        m.forward([5, 40000, 77, 9, 1234], eng.MODE_PARRALEL)         # a history on slots 0 .. 4
        m.forward([7, 50000, 11], eng.MODE_GPT)                       # and three logits rows
        if self.with_counts:
            for s in range(max_ctx):
                m.penalty_set(s, counts[s])
        self.state0 = self.snapshot()[0]
        self.ids0 = self.decode()
        self.restore()

    def snapshot(self):
        """(the five state arrays, the logits buffer, the counts or None) of M as bit patterns, through the C ABI alone"""
        st = [np.zeros(self.max_ctx * self.per) for _ in range(5)]
        lg = np.zeros(self.max_ctx * V, np.float32)
        ptr = lambda x: C.c_void_p(x.ctypes.data)
        assert self.lib.rwkv_get_output(self.h["M"], ptr(lg), *[ptr(s) for s in st], self.max_ctx) == 0
        counts = np.stack([self.models["M"].penalty_get(s) for s in range(self.max_ctx)]).view(np.uint32) if self.with_counts else None
        return [s.view(np.uint64) for s in st], lg.view(np.uint32), counts

    def decode(self):
        out = (C.c_uint64 * self.N)()
        assert self.lib.rwkv_decode_greedy(self.h["M"], self.FIRST, self.N, out) == 0, self.lib.rwkv_last_error()
        return list(out)

    def restore(self):
        assert self.lib.rwkv_set_state(self.h["M"], *[C.c_void_p(s.ctypes.data) for s in self.state0], self.max_ctx) == 0

    def close(self):
        for m in self.models.values():
            m.close()


def check_refused(ctx, entry, call_args, status, text):
    """the call answers `status` and a message that holds `text`, and has launched nothing: M's state, logits (counts, resident bytes) are
    bit-identical afterwards and a greedy decode from them gives the ids it gave before"""
    state, logits, counts = ctx.snapshot()
    resident = ctx.models["M"].resident_bytes() if ctx.with_counts else None
    rc = int(getattr(ctx.lib, entry)(*call_args))
    err = ctx.lib.rwkv_last_error().decode()
    print(f"{entry}: status {rc}, {err!r}")
    assert rc == status, err
    assert text in err, err
    state1, logits1, counts1 = ctx.snapshot()
    for name, x, y in zip(NAMES, state, state1):
        assert np.array_equal(x, y), name
    assert np.array_equal(logits, logits1)
    if ctx.with_counts:
        assert np.array_equal(counts, counts1)
        assert ctx.models["M"].resident_bytes() == resident
    assert ctx.decode() == ctx.ids0
    ctx.restore()
