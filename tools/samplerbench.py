"""time the device-side typical sampler and the sampled generation loop (tuning aid)"""
import os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
from rwkv_cpp_accelerated_amd import engine, modelfile as mf
L, D = mf.SHAPES[sys.argv[1] if len(sys.argv) > 1 else "7B"]
if len(sys.argv) > 2: L = int(sys.argv[2])
t = mf.synthetic_tensors_torch(L, D, seed=0)
m = engine.RWKV(resident=True); m.loadTensors(L, D, t)
for tk in (5, 6, 7): m.forward(tk)
n = 256
m.decode_greedy(9, 16)
t0 = time.perf_counter(); m.decode_greedy(9, n); tg = time.perf_counter() - t0
for recipe in (False, True):      # default: what the reference computes (no selection); recipe: the documented cut (radix select)
    mode = "recipe" if recipe else "default"
    m.sample_typical(0.9, 0.8, 0.3, recipe=recipe)
    t0 = time.perf_counter()
    for i in range(200): m.sample_typical(0.9, 0.8, (i + 0.5) / 200, recipe=recipe)
    print("%s: sample_typical (launch + sync + 8-byte copy): %.1f us" % (mode, (time.perf_counter() - t0) / 200 * 1e6))
    m.decode_typical(9, 16, recipe=recipe)
    t0 = time.perf_counter(); m.decode_typical(9, n, seed=1, recipe=recipe); tt = time.perf_counter() - t0
    print("%s: decode %d tokens: greedy %.3f ms/token, typical %.3f ms/token (sampler adds %.1f us)" % (mode, n, tg / n * 1e3, tt / n * 1e3, (tt - tg) / n * 1e6))
# nucleus leg: the recipe loop, alternated with the two forms of decode_nucleus (top-p alone does the recipe's three selection passes; the
# full form adds the top-k select and the read + write pass over the stream's counts), REPS rounds; us added per token over greedy of the
# same round, and the spread of each leg over the rounds
REPS = int(os.environ.get("SAMPLERBENCH_REPS", "3"))
legs = [("greedy", lambda: m.decode_greedy(9, n)),
        ("typical recipe", lambda: m.decode_typical(9, n, seed=1, recipe=True)),
        ("nucleus top_p 0.9", lambda: m.decode_nucleus(9, n, temp=1.0, top_p=0.9, seed=1)),
        ("nucleus top_p 0.9 top_k 40 pen 0.4/0.4/0.996", lambda: m.decode_nucleus(9, n, temp=1.0, top_p=0.9, top_k=40, presence=0.4, frequency=0.4, decay=0.996, seed=1))]
for _, f in legs: f()
added = {name: [] for name, _ in legs[1:]}
for rep in range(REPS):
    ms = {}
    for name, f in legs:
        t0 = time.perf_counter(); f(); ms[name] = (time.perf_counter() - t0) / n * 1e3
    for name in added: added[name].append((ms[name] - ms["greedy"]) * 1e3)
    print("round %d: " % rep + ", ".join("%s %.4f ms/token" % (k, v) for k, v in ms.items()))
for name, v in added.items():
    print("%s: adds %s us/token over greedy (min %.1f, max %.1f)" % (name, " ".join("%.1f" % x for x in v), min(v), max(v)))
m.close()
