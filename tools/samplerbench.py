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
m.close()
