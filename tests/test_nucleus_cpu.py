"""The planted nucleus cases of tests/nucleus_cases.py WITHOUT a GPU: (1) the cap on excused draws holds for every case and run from the
reference alone, so that tests/test_nucleus_gpu.py cannot hide a failure behind an excuse; (2) the reference agrees with a literal numpy
sort-and-cumsum transcription of the recipe on the cases without ties; (3) the host twin include/rwkv_sampler.h nucleus_u / nucleus_count
-- a stand-alone program (tests/cpp/nucleus_app.cpp), built with AddressSanitizer and UBSan where the toolchain has their runtime -- agrees
with the reference on every draw that is not excused, and with the f32 count update bit for bit; (4) header, engine.ABI_SYMBOLS and the
ctypes structure agree on the five new entry points."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import nucleus_cases as nc

from support import ROOT, build_app, syntax_only

RUNS = nc.all_runs()
IDS = [f"{label}-t{r.temp}-p{r.top_p}-k{r.top_k}-{'ban0' if r.ban0 else 'noban'}-pen{r.presence}/{r.frequency}" for (label, _, r, _, _) in RUNS]
NEW = ["rwkv_sample_nucleus", "rwkv_decode_nucleus", "rwkv_decode_batch_nucleus", "rwkv_penalty_set", "rwkv_penalty_get"]


@pytest.fixture(scope="module")
def app(tmp_path_factory):
    """(path, sanitized): with -fsanitize=address,undefined where that links (the sanitizer runtime is installed), plain otherwise"""
    outdir = tmp_path_factory.mktemp("nucc")
    san = ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-fno-omit-frame-pointer")
    try:
        exe = build_app("nucleus_app", outdir, link=False, opt="-O2", extra=("-g",) + san)
        print("nucleus_app: built with -fsanitize=address,undefined")
        return exe, True
    except subprocess.CalledProcessError:
        exe = build_app("nucleus_app", outdir, link=False, opt="-O2", extra=("-g",))
        print("nucleus_app: the sanitizer runtime is not installed; built without")
        return exe, False


def test_the_uniforms_are_the_66_of_the_typical_cases():
    assert len(nc.US) == 66 and nc.MAX_EXCUSED == 2


@pytest.mark.parametrize("label,lname,run,counted,shift", RUNS, ids=IDS)
def test_at_most_two_draws_are_excused(label, lname, run, counted, shift):
    n = nc.excused_count(lname, run, counted, shift)
    print(f"{label} {run}: {n} of {len(nc.US)} excused, eps {nc.ref_of(lname, run, counted, shift).eps:.3g}")
    assert n <= nc.MAX_EXCUSED


def test_the_cases_hold_what_they_claim():
    assert nc.logits_of("a") is not nc.logits_of("b") and float(nc.logits_of("c").std()) > 7.5
    l = nc.penalised(nc.logits_of("c"), None, 0, 0, False)
    p = np.exp(l - l.max()); p /= p.sum()
    assert p.max() < 0.3 and int((nc.ref_of("c", nc.Run(1, 0.8)).w > 0).sum()) == 13
    # the ties: top_p 0.5 and top_k 3 both keep every tied, unbanned id, and nothing else
    for k in (2, 50, 1025):
        for run in nc.CASES[f"d{k}"].runs:
            ids = nc.sc.tie_ids(k, run.ban0)
            live = ids[1:] if run.ban0 else ids
            assert np.nonzero(nc.ref_of(f"d{k}", run).w > 0)[0].tolist() == live.tolist(), (k, run)
    # the penalties re-order the top and push penalised tokens below the cut
    c = nc.counts_of("a")
    top = np.argsort(-nc.logits_of("a").astype(np.float64), kind="stable")[:12]
    assert (c[top] == np.array(nc.PEN_COUNTS, np.float32)).all() and int((c > 0).sum()) == 12
    plain = nc.ref_of("a", nc.Run(1, 0.9))
    for pr, fr in ((0.4, 0.4), (5, 2)):
        pen = nc.ref_of("a", nc.Run(1, 0.9, 0, False, pr, fr), True)
        lp = nc.penalised(nc.logits_of("a"), c, pr, fr, False)
        assert np.argsort(-lp, kind="stable")[:12].tolist() != top.tolist()
        assert any(plain.w[t] > 0 and pen.w[t] == 0 for t in top) or pr < 1
    assert any(plain.w[t] > 0 and nc.ref_of("a", nc.Run(1, 0.9, 0, False, 5, 2), True).w[t] == 0 for t in top)
    # case f: -99 still is the largest logit; case e: one token carries everything
    assert nc.ref_of("f", nc.Run(1, 0.5, 0, True)).pick(0.5) == 0 and nc.ref_of("e", nc.Run(1, 0.5)).pick(0.5) == 25000
    # the row case: the counts of another slot give another distribution in every row
    for (n, _, slot) in nc.ROW_CASE:
        for run in nc.ROW_RUNS:
            for (m, _, other) in nc.ROW_CASE:
                if other != slot:
                    wrong = nc.reference(nc.logits_of(n, run.ban0), run.temp, run.top_p, run.top_k, nc.counts_of(m, other), run.presence, run.frequency, run.ban0)
                    assert not np.array_equal(nc.ref_of(n, run, True, slot).w, wrong.w), (n, m, run)


def literal(logits, run, counts):
    """the recipe word for word in linear space: softmax, sort descending, cumsum, cut, top-k, temperature, running sum"""
    l = nc.penalised(logits, counts, run.presence, run.frequency, run.ban0)
    p = np.exp(l - l.max()); p /= p.sum()
    order = np.argsort(-p, kind="stable")
    cum = np.cumsum(p[order])
    pos = min(int((cum < float(np.float32(run.top_p))).sum()), len(p) - 1)
    keep = p >= p[order[pos]]
    if 0 < run.top_k < len(p):
        keep &= p >= p[order[run.top_k - 1]]
    t = float(np.float32(run.temp))
    w = np.where(keep, np.exp((l - l.max()) / t), 0.0)
    return np.cumsum(w)


@pytest.mark.parametrize("label,lname,run,counted,shift", [r for r in RUNS if not r[1].startswith("d")], ids=[i for i, r in zip(IDS, RUNS) if not r[1].startswith("d")])
def test_reference_equals_the_literal_transcription(label, lname, run, counted, shift):
    r = nc.ref_of(lname, run, counted, shift)
    c = literal(nc.logits_of(lname, run.ban0), run, nc.counts_of(lname, shift) if counted else None)
    bad = []
    for u in nc.US:
        got = min(int(np.searchsorted(c, u * c[-1], side="right")), r.last)
        if got != r.pick(u) and not r.excused(u):
            bad.append((u, got, r.pick(u)))
    assert not bad, f"(u, literal, reference): {bad[:5]}"


@pytest.mark.parametrize("label,lname,run,counted,shift", RUNS, ids=IDS)
def test_host_twin_agrees_with_the_reference(app, tmp_path, label, lname, run, counted, shift):
    exe, _ = app
    lp, cp = str(tmp_path / "logits.bin"), str(tmp_path / "counts.bin")
    nc.logits_of(lname, run.ban0).tofile(lp)
    if counted:
        nc.counts_of(lname, shift).tofile(cp)
    out = subprocess.run([exe, lp, cp if counted else "-", repr(float(run.temp)), repr(float(run.top_p)), str(int(run.top_k)), repr(float(run.presence)),
                          repr(float(run.frequency)), str(int(run.ban0))] + [repr(u) for u in nc.US], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    got = [int(x) for x in out.stdout.split()]
    r = nc.ref_of(lname, run, counted, shift)
    bad = [(u, g, r.pick(u)) for u, g in zip(nc.US, got) if g != r.pick(u) and not r.excused(u)]
    assert len(got) == len(nc.US) and not bad, f"(u, nucleus_u, reference): {bad[:5]}"


@pytest.mark.parametrize("decay", [0.996, 1.0, 0.0])
def test_host_count_update_is_the_f32_restatement(app, tmp_path, decay):
    exe, _ = app
    cp = str(tmp_path / "counts.bin")
    c = np.array(nc.counts_of("a"), np.float32)
    c.tofile(cp)
    picks = [int(np.nonzero(c)[0][0]), 0, nc.V - 1, 0, 7]
    out = subprocess.run([exe, "--count", cp, repr(decay)] + [str(g) for g in picks], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, (out.returncode, out.stderr[-2000:])
    for g in picks:
        c = nc.count_update(c, g, decay)
    assert np.array_equal(np.fromfile(cp, np.float32).view(np.uint32), c.view(np.uint32))


def test_header_symbols_and_struct_agree():
    from rwkv_cpp_accelerated_amd import engine
    with open(os.path.join(ROOT, "include", "rwkv_mi355x.h")) as f:
        hdr = f.read()
    declared = set(re.findall(r"\b(rwkv_[a-z0-9_]+)\s*\(", hdr))
    assert set(NEW) <= declared and set(NEW) <= set(engine.ABI_SYMBOLS) and declared == set(engine.ABI_SYMBOLS)
    assert ctypes.sizeof(engine.NucleusParams) == 32
    assert [n for n, _ in engine.NucleusParams._fields_] == ["temp", "top_p", "top_k", "presence", "frequency", "decay", "flags", "reserved"]
    assert re.search(r"#define RWKV_MI355X_ABI_VERSION 6\b", hdr) and engine.ABI_VERSION == 6
    assert (engine.NUCLEUS_BAN0, engine.NUCLEUS_KEEP, engine.NUCLEUS_UPDATE) == (1, 2, 4)
    for name, val in (("BAN0", 1), ("KEEP", 2), ("UPDATE", 4)):
        assert re.search(rf"#define RWKV_NUCLEUS_{name} {val}u\b", hdr)


def test_cpp_header_offers_the_wrappers(tmp_path):
    src = tmp_path / "use_nucleus.cpp"
    src.write_text('#include "rwkv.h"\n'
                   "int use(RWKV &m) {\n"
                   "    RWKV::Nucleus s{1.0f, 0.9f, 40, 0.4f, 0.4f, 0.996f};\n"
                   "    int t = m.sampleNucleus(s, 0.5, true, true, 0, 0);\n"
                   "    std::vector<unsigned long long> a = m.decodeNucleus(t, 8, s, 3, true), b = m.decodeBatchNucleus({1, 2}, 8, {3, 4}, s);\n"
                   "    m.setPenaltyCounts(0, m.getPenaltyCounts(1));\n"
                   "    std::vector<float> c(50277);\n"
                   "    nucleus_count(c.data(), nucleus_u(m.out, c.data(), 1.0f, 0.9f, 40, 0.5, 0.4f, 0.4f, true), 0.996f);\n"
                   "    return (int)(a.size() + b.size());\n"
                   "}\n")
    syntax_only(src, extra=())


def test_library_exports_the_new_entry_points(built):
    from rwkv_cpp_accelerated_amd import engine
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if ln.strip()}
    assert set(NEW) <= exported
